"""Shared by tests/test_empty_tiles_host.py and tests/test_gpu_empty_tiles.py: wide frames of the Cornell box's parts, so that there
are 8x8 tiles beside the subject that no camera ray can hit anything from (qaray_amd/csrc/hip/qa_emptytile.h, option "empty_tiles").
Every scene satisfies the last-cast predicate (no light, texture, reflective or refractive lobe or absorption; the only emitters
planes and spheres), so its frames run on qa_integrate_lastcast."""
import numpy as np

from cast_cost_util import BOX_NODE
from last_cast_util import GLOW, LIGHT_MTL

BOX = "example_project12_box.xml"
BOX_GLOW = GLOW % ("5", "0", "0.255", "24.445")   # the box's own emissive plane

# a plane rotated about two axes under a non-uniform scale, beside the box: the pyramid meets a slanted, stretched quad
TILTED_PLANE = """<object type="plane" name="tilted" material="light">
      <scale x="7" y="1.5" z="1"/>
      <rotate angle="35" x="1"/>
      <rotate angle="20" z="1"/>
      <translate x="17" y="2" z="16"/>
    </object>
    """
# glow spheres of radius 0.01 some 50 and some 5000 units from the camera at (0, -65, 11), both beside the box as the camera sees
# it: in their own space the origin stands at 5e3 and 5e5, where the discriminant of the sphere test cancels
FAR_SPHERES = """<object type="sphere" name="near" material="light">
      <scale value="0.01"/>
      <translate x="18" y="-18.4" z="11"/>
    </object>
    <object type="sphere" name="far" material="light">
      <scale value="0.01"/>
      <translate x="-2000" y="4520" z="300"/>
    </object>
    """
# the mesh under two nested groups, both transformed (a chain of three levels)
NESTED = """<object name="outer">
      <rotate angle="12" z="1"/>
      <translate x="3" y="4" z="1"/>
      <object name="inner">
        <scale x="1" y="0.8" z="1.1"/>
        <rotate angle="-8" x="1"/>
        """ + BOX_NODE + """</object>
    </object>
    """


def _camera(pos=(0, -65, 11), target=(0, 0, 11), extra=""):
    return ('<camera>\n    <position x="%g" y="%g" z="%g"/>\n    <target x="%g" y="%g" z="%g"/>\n    <up x="0" y="0" z="1"/>\n    <fov value="30"/>\n    '
            % (*pos, *target) + extra + '<width value="608"/>\n    <height value="600"/>\n  </camera>')


def _scene(objects, head="", camera=None):
    return "<xml>\n  <scene>\n    " + head + objects + LIGHT_MTL + "</scene>\n\n  " + (camera or _camera()) + "\n</xml>\n"


SCENES = {
    "box": _scene(BOX_NODE + BOX_GLOW),
    "tilted_plane": _scene(BOX_NODE + BOX_GLOW + TILTED_PLANE),
    "far_spheres": _scene(BOX_NODE + BOX_GLOW + FAR_SPHERES),
    "nested_groups": _scene(NESTED + BOX_GLOW),
    "coloured_background": _scene(BOX_NODE + BOX_GLOW, '<background r="0.25" g="0.5" b="0.125"/>\n    '),
    # the camera stands in the room: inside the mesh's bounds no tile is empty
    "camera_inside": _scene(BOX_NODE + BOX_GLOW, camera=_camera((5, 9, 14), (-7, -6, 2))),
    "depth_of_field": _scene(BOX_NODE + BOX_GLOW, camera=_camera(extra='<focaldist value="65"/>\n    <dof value="0.8"/>\n    ')),
}
NO_EMPTY_TILE = ("camera_inside", "depth_of_field")


def scene_blob(directory, name, size):
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    p = directory / f"{name}_{size[0]}x{size[1]}.xml"
    p.write_text(SCENES[name])
    return load_scene_blob(str(p), size=size, asset_root=SCENES_DIR)


def nan_background(blob):
    """`blob` with a background component that is not a number: no tile of it may be called empty."""
    from qaray_amd import hip
    hip.blob_backdrop(blob)[0]["color"][1] = np.nan
    return blob


def background_of(blob):
    from qaray_amd import hip
    return np.array(hip.blob_backdrop(blob)[0]["color"], np.float32)


def tile_all(per_pixel, size):
    """bool [h, w] -> bool [tiles y, tiles x]: every pixel of the 8x8 tile (ragged ones: of its part inside the frame)."""
    w, h = size
    ty, tx = (h + 7) // 8, (w + 7) // 8
    padded = np.ones((ty * 8, tx * 8), bool)
    padded[:h, :w] = per_pixel
    return padded.reshape(ty, 8, tx, 8).all(axis=(1, 3))
