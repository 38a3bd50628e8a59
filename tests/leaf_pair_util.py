"""Shared by tests/test_leaf_pair_host.py and tests/test_gpu_leaf_pair.py: a scene without lights with two meshes whose leaf tables
the last-cast query sweeps a leaf per turn (qaray_amd/csrc/hip/qa_kernel.h sweepLeaves) - the Cornell box, and in
front of it a floor of five triangles: an odd count, so one leaf of its own tree holds a single triangle, and some leaf ends at
the mesh's last record."""
import os
import shutil

from cast_cost_util import BOX_NODE
from leaf_sweep_util import GLOW, MESH, _scene, grid_obj

# three cells, two triangles each, without the last one
ODD_FLOOR = "\n".join(grid_obj((-18.0, -45.0, -3.0), (36.0, 0.0, 0.0), (0.0, 30.0, 0.0), 3, 1).splitlines()[:-1]) + "\n"
assert sum(ln.startswith("f ") for ln in ODD_FLOOR.splitlines()) == 5
OBJECTS = BOX_NODE + MESH % "odd_floor.obj" + GLOW % ("5", "0", "0.255", "24.445")
CAMERA = (0, -90, 20, 0, -12, 8)


def odd_floor_blob(directory, size):
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    root = directory / "leaf_pair_odd_floor"
    (root / "examples").mkdir(parents=True, exist_ok=True)
    for f in ("cornell_box.obj", "cornell_box.mtl"):
        shutil.copy(os.path.join(SCENES_DIR, "examples", f), str(root / "examples" / f))
    (root / "odd_floor.obj").write_text(ODD_FLOOR)
    p = root / f"odd_floor_{size[0]}x{size[1]}.xml"
    p.write_text(_scene(OBJECTS, CAMERA))
    return load_scene_blob(str(p), size=size, asset_root=str(root))
