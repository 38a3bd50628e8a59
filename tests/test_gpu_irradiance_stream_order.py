"""Cross-stream ordering of the irradiance entry, on the stall-and-check harness of tests/stream_order_util.py and in the pattern of
tests/test_gpu_ao_stream_order.py (DESIGN.md "Streams: who waits for whom"): one stream is held busy, the call on the other must have
waited for it - by the order of two events, and by the bits of both results against the same two calls run serially.

qa_irradiance_points_device is launched as qa_radiance_rays_device is (LaunchRayBatch): behind the context's last frame and last edit
(lastFrame, lastEdit), and it records lastFrame, so that a later edit waits for it (it reads the tables an edit rewrites).

The table of tests/stream_order_util.py lists the entries that take a `hip_stream`; the entry here calls its `stream` and has its
table here: CASES (test -> the entries it puts on a late or a waiting stream) and EXEMPT (entry -> why there is nothing to order).
tests/test_irradiance_stream_closure.py holds the header to the two, without a GPU."""
import numpy as np
import pytest

import stream_order_util as U
from test_gpu_stream_order import BOX3, H, REGION, W, _moved_node, filled, frame_of, new_ctx, warm_frame

pytestmark = pytest.mark.gpu

CASES = {
    "test_frame_and_points_wait_for_each_other": ("qa_irradiance_points_device",),               # lastFrame, both ways
    "test_points_right_after_an_edit_see_the_edited_scene": ("qa_irradiance_points_device",),   # lastEdit (and lastFrame behind it)
    "test_a_later_edit_waits_for_the_points": ("qa_irradiance_points_device",),                  # lastFrame, the other way
}
EXEMPT = {}

N = H * W
SPP, BOUNCES = 2, 2


@pytest.fixture(scope="module")
def streams():
    import torch
    dev = torch.device("cuda", 0)
    a = torch.cuda.Stream(dev)
    U.calibrate(a)
    b = U.concurrency_control(a, [torch.cuda.Stream(dev) for _ in range(4)])
    yield a, b
    torch.cuda.synchronize()


def setup():
    """The lit box with the node _moved_node moves; points on the surfaces the frame's first samples see, normals towards the camera"""
    import torch
    st = new_ctx(BOX3)
    st["old"], st["new"] = _moved_node(st["blob"])
    c = st["ctx"]
    r = c.camera_sample_rays_device(REGION, 0, 1, outputs=("origins", "dirs"))
    d = r["dirs"].reshape(-1, 3)
    got = c.cast_rays_device(r["origins"].reshape(-1, 3), d, normal=torch.empty((N, 3), device="cuda"), point=torch.empty((N, 3), device="cuda"))
    c.synchronize()
    st["points"], st["normals"] = got["point"], -got["normal"] * torch.sign((got["normal"] * d).sum(dim=1, keepdim=True))
    torch.cuda.synchronize()
    return st


def points(st, s):
    import torch
    rgb, ns = st["ctx"].irradiance_points_device(st["points"], st["normals"], SPP, BOUNCES, rgb=filled(s, (N, 3), torch.float32),
                                                 ns=filled(s, (N,), torch.int32), stream=s.cuda_stream)
    return {"rgb": rgb, "ns": ns}


def warm(st, s):
    warm_frame(st, s)
    st["ctx"].edit_instances(*st["old"])   # (an edit that changes nothing: the pinned ring is made here)
    points(st, s)


def moved_then_points(st, s):
    st["ctx"].edit_instances(*st["new"])
    return points(st, s)


def on_the_scene_as_uploaded():
    import torch
    st = setup()
    try:
        out = points(st, torch.cuda.current_stream())
        st["ctx"].synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        st["close"]()


def test_frame_and_points_wait_for_each_other(streams):
    a, b = streams
    U.ordered("frame_irradiance_points frame->points", setup, frame_of(1), points, a, b, warm=warm)
    U.ordered("frame_irradiance_points points->frame", setup, points, frame_of(2), a, b, warm=warm)


def test_points_right_after_an_edit_see_the_edited_scene(streams):
    """The node is moved while the frame the edit must wait for is held on a; the points on b right after are lit by the moved scene"""
    a, b = streams
    _, new, _ = U.ordered("edit_instances_irradiance_points", setup, frame_of(1), moved_then_points, a, b, warm=warm)
    old = on_the_scene_as_uploaded()
    assert (new["ns"] == SPP).all() and (new["rgb"] > 0).any()
    # the light at the same points of the scene before the edit differs, so a call that had read the old tables would show
    assert not np.array_equal(old["rgb"].view(np.uint32), new["rgb"].view(np.uint32))


def test_a_later_edit_waits_for_the_points(streams):
    """The points are held on a; the edit that follows on the context's stream, and the points of the moved scene on b, come after
    them: the held call saw the scene before the move"""
    a, b = streams
    old, new, _ = U.ordered("irradiance_points_edit_instances", setup, points, moved_then_points, a, b, warm=warm)
    want = on_the_scene_as_uploaded()
    assert np.array_equal(old["rgb"].view(np.uint32), want["rgb"].view(np.uint32)) and (old["ns"] == SPP).all()
    assert not np.array_equal(old["rgb"].view(np.uint32), new["rgb"].view(np.uint32))
