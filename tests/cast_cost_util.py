"""Shared by tests/test_cast_cost_host.py and tests/test_gpu_cast_cost.py: scene texts built on the Cornell box's file
(example_project12_box.xml) and camera poses for them."""
import os

BOX = "example_project12_box.xml"

BOX_NODE = """<object type="obj" name="examples/cornell_box.obj">
      <translate x="-278" y="-274.4" z="-279.1"/>
      <scale value="0.05"/>
      <rotate angle="90" x="1"/>
      <rotate angle="180" z="1"/>
      <translate x="0" y="0" z="11"/>
    </object>
    """
# a sphere, a rotated plane and the box's mesh under a non-uniform scale; no light (the box's emissive plane stays)
MIXED = """<object type="sphere" name="ball" material="grey">
      <scale value="3"/>
      <translate x="-7" y="-6" z="2"/>
    </object>
    <object type="plane" name="tilted" material="grey">
      <rotate angle="35" x="1"/>
      <rotate angle="20" z="1"/>
      <scale value="6"/>
      <translate x="7" y="2" z="4"/>
    </object>
    <object type="obj" name="examples/cornell_box.obj">
      <translate x="-278" y="-274.4" z="-279.1"/>
      <scale x="0.05" y="0.035" z="0.06"/>
      <rotate angle="90" x="1"/>
      <rotate angle="180" z="1"/>
      <translate x="0" y="0" z="9"/>
    </object>
    <material type="blinn" name="grey">
      <diffuse value="0.7"/>
      <specular value="0"/>
    </material>
    """
# a plane before the mesh in the scene graph that covers part of it
SCREEN = """<object type="plane" name="screen">
      <rotate angle="90" x="1"/>
      <scale value="6"/>
      <translate x="-5" y="-20" z="8"/>
    </object>
    """

# camera poses (position, target, up): the file's | in the room | beside the box, half of it behind | under the mesh's light quad
# (world z = 24.68), looking up at it a little off the vertical
CAMERAS = {"outside": None, "inside": ((5, 9, 14), (-7, -6, 2), (0, 0, 1)), "beside": ((-16, -2, 11), (-15, 30, 13), (0, 0, 1)),
           "under_the_light": ((1.5, -2, 3), (0, 0, 24.68), (0, 1, 0))}


def scene_text(objects, camera="outside"):
    """The Cornell box's file with `objects` in place of its mesh node (the emissive plane stays) and the camera at `camera`."""
    from qaray_amd.host import SCENES_DIR
    text = open(os.path.join(SCENES_DIR, BOX)).read()
    a, b = text.index("<object type=\"obj\""), text.index("<object type=\"plane\"")
    text = text[:a] + objects + text[b:]
    if CAMERAS[camera] is not None:
        pos, target, up = CAMERAS[camera]
        a, b = text.index("<position"), text.index("<fov")
        text = text[:a] + '<position x="%g" y="%g" z="%g"/>\n    <target x="%g" y="%g" z="%g"/>\n    <up x="%g" y="%g" z="%g"/>\n    ' % (*pos, *target, *up) + text[b:]
    return text


def scene_blob(directory, objects, size, camera="outside"):
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    p = directory / f"scene_{camera}_{size[0]}x{size[1]}.xml"
    p.write_text(scene_text(objects, camera))
    return load_scene_blob(str(p), size=size, asset_root=SCENES_DIR)
