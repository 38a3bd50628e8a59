"""Cross-stream ordering of the ambient-occlusion entries, on the stall-and-check harness of tests/stream_order_util.py and in the
pattern of tests/test_gpu_idmatte_stream_order.py (DESIGN.md "Streams: who waits for whom"): one stream is held busy, the call on the
other must have waited for it - by the order of two events, and by the bits of both results against the same two calls run serially.

qa_ao_region_device and qa_ao_points_device go through LaunchSceneKernel as qa_matte_region_device and qa_occluded_device do (lastFrame
both ways, lastEdit); qa_progressive_ao_device waits for the frame's last pass (prog.done).

The table of tests/stream_order_util.py lists the entries that take a `hip_stream` and belongs to tests/test_gpu_stream_order.py; the
entries here call theirs `stream` and have their table here: CASES (test -> the entries it puts on a late or a waiting stream) and
EXEMPT (entry -> why there is nothing to order).  tests/test_ao_stream_closure.py holds the header to the two, without a GPU."""
import numpy as np
import pytest

import stream_order_util as U
from test_gpu_stream_order import BOX3, H, REGION, SPP, W, _advance, _moved_node, _prog_state, _progressive, filled, frame_of, new_ctx, warm_frame, warmed

pytestmark = pytest.mark.gpu

CASES = {
    "test_frame_and_ao_wait_for_each_other": ("qa_ao_region_device",),                          # lastFrame, both ways
    "test_ao_right_after_an_edit_sees_the_edited_scene": ("qa_ao_region_device",),              # lastEdit
    "test_the_progressive_ao_waits_for_the_frames_last_pass": ("qa_progressive_ao_device",),    # prog.done
    "test_ao_at_points_waits_behind_an_edit": ("qa_ao_points_device",),                         # lastEdit (and lastFrame behind it)
}
EXEMPT = {
    "qa_ao_grey_device": "touches no state of the context: one kernel over the caller's planes",
}

K, RADIUS = 4, 6.0


@pytest.fixture(scope="module")
def streams():
    import torch
    dev = torch.device("cuda", 0)
    a = torch.cuda.Stream(dev)
    U.calibrate(a)
    b = U.concurrency_control(a, [torch.cuda.Stream(dev) for _ in range(4)])
    yield a, b
    torch.cuda.synchronize()


def ao(c, s, region=REGION, spp=SPP):
    import torch
    h, w = region[3] - region[1], region[2] - region[0]
    return c.ao_device(region, spp, K, RADIUS, open=filled(s, (h, w), torch.int32), rays=filled(s, (h, w), torch.int32),
                       ao=filled(s, (h, w), torch.float32), stream=s.cuda_stream)


def _moved_setup():
    st = new_ctx(BOX3)
    st["old"], st["new"] = _moved_node(st["blob"])
    return st


def test_frame_and_ao_wait_for_each_other(streams):
    a, b = streams
    call = lambda st, s: ao(st["ctx"], s)   # noqa: E731
    setup = lambda: new_ctx(BOX3)   # noqa: E731
    U.ordered("frame_ao frame->pass", setup, frame_of(1), call, a, b, warm=warmed(call))
    U.ordered("frame_ao pass->frame", setup, call, frame_of(2), a, b, warm=warmed(call))


def test_ao_right_after_an_edit_sees_the_edited_scene(streams):
    """The node is moved while the frame the edit must wait for is held on a; the planes on b right after are the moved scene's"""
    a, b = streams

    def warm(st, s):
        warm_frame(st, s)
        st["ctx"].edit_instances(*st["old"])   # (an edit that changes nothing: the pinned ring is made here)
        ao(st["ctx"], s)

    def consumer(st, s):
        st["ctx"].edit_instances(*st["new"])
        return ao(st["ctx"], s)

    _, new, _ = U.ordered("edit_instances_ao", _moved_setup, frame_of(1), consumer, a, b, warm=warm)
    # the planes of the scene before the edit differ, so a pass that had read the old tables would show
    st = _moved_setup()
    try:
        old = st["ctx"].ao(REGION, SPP, K, RADIUS)
    finally:
        st["close"]()
    assert not np.array_equal(old["open"].view(np.int32), new["open"]) or not np.array_equal(old["rays"].view(np.int32), new["rays"])


def test_the_progressive_ao_waits_for_the_frames_last_pass(streams):
    import torch
    a, b = streams

    def reader(st, s):
        return st["p"].ao_device(K, RADIUS, open=filled(s, (H, W), torch.int32), rays=filled(s, (H, W), torch.int32),
                                 ao=filled(s, (H, W), torch.float32), stream=s.cuda_stream)
    # (warm: the reader once on the fresh frame, as the other readers of a progressive frame are warmed)
    _, got, _ = U.ordered("progressive_ao", _progressive(), _advance(4), reader, a, b, warm=reader, finish=_prog_state)
    # the pass that was held had finished: the pixels hold their four samples (a pixel whose samples all hit shows all of them)
    assert got["rays"].max() == 4 * K and (got["rays"] % K == 0).all()


def test_ao_at_points_waits_behind_an_edit(streams):
    """Points on the surfaces the frame's first samples see; the node is moved under a held frame, the points form on b follows"""
    import torch
    a, b = streams
    n = H * W

    def setup():
        st = _moved_setup()
        c = st["ctx"]
        r = c.camera_sample_rays_device(REGION, 0, 1, outputs=("origins", "dirs"))
        got = c.cast_rays_device(r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3), normal=torch.empty((n, 3), device="cuda"),
                                 point=torch.empty((n, 3), device="cuda"))
        c.synchronize()
        st["points"], st["normals"] = got["point"], -got["normal"] * torch.sign((got["normal"] * r["dirs"].reshape(-1, 3)).sum(dim=1, keepdim=True))
        torch.cuda.synchronize()
        return st

    def points(st, s):
        return st["ctx"].ao_points_device(st["points"], st["normals"], 8, RADIUS, open=filled(s, (n,), torch.int32),
                                          ao=filled(s, (n,), torch.float32), stream=s.cuda_stream)

    def warm(st, s):
        warm_frame(st, s)
        st["ctx"].edit_instances(*st["old"])
        points(st, s)

    def consumer(st, s):
        st["ctx"].edit_instances(*st["new"])
        return points(st, s)

    _, new, _ = U.ordered("edit_instances_ao_points", setup, frame_of(1), consumer, a, b, warm=warm)
    st = setup()
    try:
        old = points(st, torch.cuda.current_stream())
        st["ctx"].synchronize()
        old = old["open"].cpu().numpy()
    finally:
        st["close"]()
    # the counts at the same points of the scene before the edit differ, so a pass that had read the old tables would show
    assert not np.array_equal(old, new["open"])
