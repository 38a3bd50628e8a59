"""Shared by tests/test_last_cast_host.py and tests/test_gpu_last_cast.py: scenes for the last-cast query of resident scenes
without lights (qaray_amd/csrc/hip/qa_kernel.h lastCastQuery) - the Cornell box's parts put together in ways the query must get
right - and blobs on which its scene predicate (qa_scene_build.cpp PlanLastCast) must fail."""
from cast_cost_util import BOX_NODE

# the box's emissive plane as its file has it (below the mesh's light quad, world z = 24.68), and variations
GLOW = """<object type="plane" name="lightPlane" material="light">
      <scale value="%s"/>
      <translate x="%s" y="%s" z="%s"/>
    </object>
    """
# upright, facing the camera, behind the blocks as the floor sees it: part of it is hidden by them
GLOW_UPRIGHT = """<object type="plane" name="lightPlane" material="light">
      <rotate angle="90" x="1"/>
      <scale value="4"/>
      <translate x="-2" y="9" z="4"/>
    </object>
    """
GLOW_SPHERE = """<object type="sphere" name="bulb" material="light">
      <scale value="2.5"/>
      <translate x="3" y="-2" z="17"/>
    </object>
    """
LIGHT_MTL = """<material type="blinn" name="light">
      <emission value="15"/>
      <specular value="0"/>
    </material>
    """
CAMERA = """<camera>
    <position x="0" y="-65" z="11"/>
    <target x="0" y="0" z="11"/>
    <up x="0" y="0" z="1"/>
    <fov value="30"/>
    <width value="608"/>
    <height value="600"/>
  </camera>"""


def _scene(objects, head=""):
    return "<xml>\n  <scene>\n    " + head + objects + LIGHT_MTL + "</scene>\n\n  " + CAMERA + "\n</xml>\n"


# name -> scene text.  Every one satisfies the predicate: no light, no texture, no reflective / refractive lobe, no absorption,
# the only emitter a plane or sphere
SCENES = {
    # the glow plane in the plane of the mesh's light quad and larger than it: a bounce ray that meets the quad meets both at one place
    "coplanar_after": _scene(BOX_NODE + GLOW % ("5", "0", "0.255", "24.68")),
    "coplanar_before": _scene(GLOW % ("5", "0", "0.255", "24.68") + BOX_NODE),
    # the box's own plane, before the mesh in node order instead of after it
    "glow_before_mesh": _scene(GLOW % ("5", "0", "0.255", "24.445") + BOX_NODE),
    "glow_sphere": _scene(BOX_NODE + GLOW_SPHERE),
    "glow_sphere_and_plane": _scene(GLOW_SPHERE + BOX_NODE + GLOW % ("5", "0", "0.255", "24.445")),
    "glow_behind_blocks": _scene(BOX_NODE + GLOW_UPRIGHT),
    # the box is open towards the camera: bounce rays leave it, and what they add is the environment's colour without a draw
    "open_environment": _scene(BOX_NODE + GLOW % ("5", "0", "0.255", "24.445"), '<environment r="0.4" g="0.3" b="0.2"/>\n    '),
}


def scene_blob(directory, name, size):
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    p = directory / f"{name}_{size[0]}x{size[1]}.xml"
    p.write_text(SCENES[name])
    return load_scene_blob(str(p), size=size, asset_root=SCENES_DIR)


def mesh_materials(blob):
    """Indices into the material table of the materials the box's mesh node can be shaded with."""
    from qaray_amd import hip
    inst, sets = hip.blob_table(blob, "instances"), hip.blob_table(blob, "mtlsets")
    k = [k for k in range(len(inst)) if inst[k]["obj_type"] == 3][0]
    ms = sets[inst[k]["mtlset"]]
    return list(range(int(ms["first"]), int(ms["first"]) + (int(ms["count"]) if ms["multi"] else 1)))


def spoil(blob, how):
    """`blob` (the box) changed in place so that the predicate fails."""
    from qaray_amd import hip
    mats, inst = hip.blob_table(blob, "materials"), hip.blob_table(blob, "instances")
    wall = mesh_materials(blob)[1]
    if how == "reflective":
        mats[wall]["reflection"]["color"] = 0.375
    elif how == "absorbing":
        mats[wall]["absorption"] = (0.0, 0.25, 0.0)
    elif how == "emissive_mesh":
        mats[wall]["emission"]["color"] = (0.0, 0.0, 0.5)
    elif how == "no_material":
        k = [k for k in range(len(inst)) if inst[k]["obj_type"] == 2][0]
        inst[k]["mtlset"] = -1
    else:
        raise ValueError(how)
    return blob


SPOILED = ("reflective", "absorbing", "emissive_mesh", "no_material")
