"""Cross-stream ordering of the bake entries, on the stall-and-check harness of tests/stream_order_util.py and in the pattern of
tests/test_gpu_ao_stream_order.py (DESIGN.md "Streams: who waits for whom"): one stream is held busy, the call on the other must have
waited for it - by the order of two events, and by the bits of both results against the same two calls run serially.

qa_bake_texels_device goes through LaunchSceneKernel as qa_ao_points_device does: behind the context's last frame and last edit
(lastFrame, lastEdit), and a later edit waits for it (it reads the instance table an edit rewrites).

The table of tests/stream_order_util.py lists the entries that take a `hip_stream`; the entries here call theirs `stream` and have
their table here: CASES (test -> the entries it puts on a late or a waiting stream) and EXEMPT (entry -> why there is nothing to
order).  tests/test_bake_stream_closure.py holds the header to the two, without a GPU."""
import numpy as np
import pytest

import bake_util as B
import stream_order_util as U
from test_gpu_stream_order import H, W, _moved_node, filled, frame_of, warm_frame

pytestmark = pytest.mark.gpu

CASES = {
    "test_the_map_right_after_an_edit_is_the_moved_nodes": ("qa_bake_texels_device",),   # lastEdit (and lastFrame behind it)
    "test_a_later_edit_waits_for_the_map": ("qa_bake_texels_device",),                    # lastFrame, the other way
}
EXEMPT = {
    "qa_bake_dilate_device": "touches no state of the context: one kernel over the caller's picture and face plane",
}

TW, TH = 64, 48   # texels


@pytest.fixture(scope="module")
def streams():
    import torch
    dev = torch.device("cuda", 0)
    a = torch.cuda.Stream(dev)
    U.calibrate(a)
    b = U.concurrency_control(a, [torch.cuda.Stream(dev) for _ in range(4)])
    yield a, b
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def blob(tmp_path_factory):
    """A floor and, last in the node order (the node _moved_node moves), a domed chart: point lights only"""
    floor = '<object type="plane" name="floor" material="m"><scale value="12"/></object>'
    objects = floor + B.mesh_node("dome.obj", '<rotate angle="20" z="1"/><translate z="1"/>')
    return B.write_scene(tmp_path_factory.mktemp("bake_order"), objects, {"dome.obj": B.grid_obj(6, 5, seed=2, height=B.dome)}, size=(W, H))


def setup_of(blob):
    def setup():
        from qaray_amd import hip
        c = hip.Context(0)
        mine = blob.copy()
        c.upload_scene(mine)
        st = {"ctx": c, "blob": mine, "close": c.close}
        st["old"], st["new"] = _moved_node(mine)
        st["node"] = st["old"][0]
        return st
    return setup


def bake(st, s):
    import torch
    return st["ctx"].bake_texels_device(st["node"], TW, TH, point=filled(s, (TH, TW, 3), torch.float32), normal=filled(s, (TH, TW, 3), torch.float32),
                                        face=filled(s, (TH, TW), torch.int32), bary=filled(s, (TH, TW, 2), torch.float32), stream=s.cuda_stream)


def warm(st, s):
    warm_frame(st, s)
    st["ctx"].edit_instances(*st["old"])   # (an edit that changes nothing: the pinned ring is made here)
    bake(st, s)


def moved_then_bake(st, s):
    st["ctx"].edit_instances(*st["new"])
    return bake(st, s)


def test_the_map_right_after_an_edit_is_the_moved_nodes(streams, blob):
    """The node is moved while the frame the edit must wait for is held on a; the map on b right after holds the moved node's points"""
    from qaray_amd import hip
    a, b = streams
    _, new, _ = U.ordered("edit_instances_bake", setup_of(blob), frame_of(1), moved_then_bake, a, b, warm=warm)
    moved = blob.copy()
    k, rec = _moved_node(blob)[1]
    hip.blob_table(moved, "instances")[k:k + 1] = rec
    want = hip.bake_texels_host(moved, k, TW, TH)
    assert all(np.array_equal(new[p].view(np.uint32), want[p].view(np.uint32)) for p in hip.BAKE_PLANES)
    before = hip.bake_texels_host(blob, k, TW, TH)
    assert np.array_equal(before["face"], want["face"]) and not np.array_equal(before["point"], want["point"])


def test_a_later_edit_waits_for_the_map(streams, blob):
    """The map is held on a; the edit that follows on the context's stream, and the map of the moved node on b, come after it: the held
    map is the node's before the move"""
    from qaray_amd import hip
    a, b = streams
    old, new, _ = U.ordered("bake_edit_instances", setup_of(blob), bake, moved_then_bake, a, b, warm=warm)
    k = _moved_node(blob)[0][0]
    want = hip.bake_texels_host(blob, k, TW, TH)
    assert all(np.array_equal(old[p].view(np.uint32), want[p].view(np.uint32)) for p in hip.BAKE_PLANES)
    assert not np.array_equal(old["point"], new["point"])
