"""Shared by tests/test_leaf_sweep_host.py and tests/test_gpu_leaf_sweep.py: scenes without lights whose meshes have no leaf table
that the last-cast query could sweep (qaray_amd/csrc/hip/qa_kernel.h sweepLeaves) - an own tree that is one leaf, and one of more
than QA_TILE_LEAF_CAP = 64 leaves - next to the Cornell box's mesh, which has one.  The meshes are written as .obj files here."""
import os
import shutil

from cast_cost_util import BOX_NODE
from last_cast_util import LIGHT_MTL

GREY = """<material type="blinn" name="grey">
      <diffuse value="0.7"/>
      <specular value="0"/>
    </material>
    """
GLOW = """<object type="plane" name="lightPlane" material="light">
      <scale value="%s"/>
      <translate x="%s" y="%s" z="%s"/>
    </object>
    """
CAMERA = """<camera>
    <position x="%s" y="%s" z="%s"/>
    <target x="%s" y="%s" z="%s"/>
    <up x="0" y="0" z="1"/>
    <fov value="40"/>
    <width value="608"/>
    <height value="600"/>
  </camera>"""
MESH = """<object type="obj" name="%s" material="grey">
    </object>
    """


def _scene(objects, camera):
    return "<xml>\n  <scene>\n    " + objects + LIGHT_MTL + GREY + "</scene>\n\n  " + CAMERA % camera + "\n</xml>\n"


def grid_obj(origin, du, dv, nu, nv):
    """A parallelogram of nu x nv cells, two triangles each, as the text of an .obj file."""
    lines = []
    for j in range(nv + 1):
        for i in range(nu + 1):
            lines.append("v %.9g %.9g %.9g" % tuple(origin[a] + du[a] * i / nu + dv[a] * j / nv for a in range(3)))
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i + 1
            b, c, d = a + 1, a + nu + 2, a + nu + 1
            lines.append("f %d %d %d" % (a, b, c))
            lines.append("f %d %d %d" % (a, c, d))
    return "\n".join(lines) + "\n"


def confetti_obj(origin, du, dv, nu, nv):
    """nu x nv separate triangles, one in every cell of a parallelogram and smaller than it: the own tree (at most two triangles a
    leaf, split where that is cheaper) gives every one a leaf of its own."""
    lines = []
    for j in range(nv):
        for i in range(nu):
            for (a, b) in ((0.1, 0.1), (0.8, 0.1), (0.1, 0.8)):
                lines.append("v %.9g %.9g %.9g" % tuple(origin[k] + du[k] * (i + a) / nu + dv[k] * (j + b) / nv for k in range(3)))
    for t in range(nu * nv):
        lines.append("f %d %d %d" % (3 * t + 1, 3 * t + 2, 3 * t + 3))
    return "\n".join(lines) + "\n"


# name -> (objects, camera, the .obj files it needs: name -> text)
FLOOR = grid_obj((-18.0, -45.0, -3.0), (36.0, 0.0, 0.0), (0.0, 30.0, 0.0), 1, 1)          # 2 triangles: one leaf
# 70 triangles, 70 leaves: more than a leaf table holds (a tessellated quad of that many leaves would be some 140 triangles, and a
# mesh of that size no longer fits the LDS-resident image)
WALL = confetti_obj((-9.0, 6.0, 0.0), (18.0, 0.0, 0.0), (0.0, 0.0, 16.0), 7, 10)
GROUND = grid_obj((-14.0, -14.0, 0.0), (28.0, 0.0, 0.0), (0.0, 28.0, 0.0), 1, 1)
SCENES = {
    # the box (18 leaves: swept) and a floor in front of it whose own tree is one leaf (walked)
    "one_leaf": (BOX_NODE + MESH % "floor.obj" + GLOW % ("5", "0", "0.255", "24.445"), (0, -90, 20, 0, -12, 8), {"floor.obj": FLOOR}),
    # a wall of more than 64 leaves on a ground of one leaf under the emissive plane: no mesh of the scene is swept
    "many_leaves": (MESH % "ground.obj" + MESH % "wall.obj" + GLOW % ("6", "0", "-4", "18"), (0, -50, 14, 0, 0, 7), {"ground.obj": GROUND, "wall.obj": WALL}),
}


def scene_blob(directory, name, size):
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    objects, camera, objs = SCENES[name]
    root = directory / f"leaf_sweep_{name}"
    (root / "examples").mkdir(parents=True, exist_ok=True)
    for f in ("cornell_box.obj", "cornell_box.mtl"):
        shutil.copy(os.path.join(SCENES_DIR, "examples", f), str(root / "examples" / f))
    for f, text in objs.items():
        (root / f).write_text(text)
    p = root / f"{name}_{size[0]}x{size[1]}.xml"
    p.write_text(_scene(objects, camera))
    return load_scene_blob(str(p), size=size, asset_root=str(root))
