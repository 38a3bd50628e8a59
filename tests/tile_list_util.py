"""Shared by tests/test_tile_cull_host.py and tests/test_gpu_tile_lists.py: the Cornell box (example_project12_box.xml) with its
mesh node posed five ways relative to the camera - what the per-tile leaf lists of camera rays (qa_tilecull.h) must get right."""
import numpy as np

from scene_edit_util import rotation, scene_path, xml_camera

BOX = "example_project12_box.xml"
POSES = ("box", "scaled_rotated", "origin_in_bounds", "origin_in_leaf", "partly_behind")
# points of the mesh's own space (cornell_box.obj: 0 .. 556): its centre, a point inside the short block (a leaf of the own
# tree with volume), a point of the room inside no leaf box, a point beside the left wall
CENTRE, IN_LEAF, IN_ROOM, BESIDE = (278.0, 274.4, 279.6), (160.0, 80.0, 250.0), (400.0, 400.0, 100.0), (-30.0, 274.4, 279.6)


def mesh_node(blob):
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    return inst, [k for k in range(len(inst)) if inst[k]["obj_type"] == 3][0]


def pose_blob(pose, size):
    """The box scene flattened at `size` with the mesh node's tm / itm / pos rewritten for `pose`."""
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob(BOX, size=size)
    if pose == "box":
        return blob
    inst, k = mesh_node(blob)
    tm0 = inst[k]["tm"].reshape(3, 3).T.astype(np.float64)   # column-major storage
    pos0 = inst[k]["pos"].astype(np.float64)
    cam = np.array(xml_camera(scene_path(BOX))["pos"], np.float64)
    if pose == "scaled_rotated":      # non-uniform scale of the mesh's axes, then a rotation; the centre stays where it was
        T = rotation(25.0, (1, 2, 3)).astype(np.float64) @ tm0 @ np.diag([1.0, 1.6, 0.6])
        pos = tm0 @ np.array(CENTRE) + pos0 - T @ np.array(CENTRE)
    elif pose == "origin_in_bounds":  # the camera stands in the room
        T = rotation(10.0, (0, 0, 1)).astype(np.float64) @ tm0 * 2.0
        pos = cam - T @ np.array(IN_ROOM)
    elif pose == "origin_in_leaf":    # the camera stands inside the short block
        T = rotation(-15.0, (0, 1, 1)).astype(np.float64) @ tm0 * 3.0
        pos = cam - T @ np.array(IN_LEAF)
    elif pose == "partly_behind":     # the camera stands beside the box and looks along its wall: half of it lies behind
        T = rotation(5.0, (0, 0, 1)).astype(np.float64) @ tm0
        pos = cam - T @ np.array(BESIDE)
    else:
        raise ValueError(pose)
    T32 = T.astype(np.float32)
    inst[k]["tm"] = T32.T.reshape(9)
    inst[k]["itm"] = np.linalg.inv(T32.astype(np.float64)).astype(np.float32).T.reshape(9)
    inst[k]["pos"] = pos.astype(np.float32)
    return blob
