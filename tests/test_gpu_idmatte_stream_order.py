"""Cross-stream ordering of the id matte's entries, on the stall-and-check harness of tests/stream_order_util.py and in the pattern of
tests/test_gpu_stream_order.py (DESIGN.md "Streams: who waits for whom"): one stream is held busy, the call on the other must have
waited for it - by the order of two events, and by the bits of both results against the same two calls run serially.

qa_idmatte_region_device goes through LaunchSceneKernel as qa_matte_region_device does (lastFrame both ways, lastEdit);
qa_progressive_idmatte_device waits for the frame's last pass (prog.done).  qa_idmatte_select_device touches no state of the context.

The table of tests/stream_order_util.py lists the entries that take a `hip_stream` and belongs to tests/test_gpu_stream_order.py; the id
matte's entries call theirs `stream` and have their table here: CASES (test -> the entries it puts on a late or a waiting stream) and
EXEMPT (entry -> why there is nothing to order).  tests/test_idmatte_stream_closure.py holds the header to the two, without a GPU."""
import numpy as np
import pytest

import stream_order_util as U
from test_gpu_stream_order import BOX3, H, REGION, SPP, W, _advance, _moved_node, _prog_state, _progressive, filled, frame_of, new_ctx, warm_frame, warmed

pytestmark = pytest.mark.gpu

CASES = {
    "test_frame_and_id_matte_wait_for_each_other": ("qa_idmatte_region_device",),                   # lastFrame, both ways
    "test_an_id_matte_right_after_an_edit_sees_the_edited_scene": ("qa_idmatte_region_device",),    # lastEdit
    "test_the_progressive_id_matte_waits_for_the_frames_last_pass": ("qa_progressive_idmatte_device",),   # prog.done
}
EXEMPT = {
    "qa_idmatte_select_device": "touches no state of the context: one kernel over the caller's planes, the id list in its arguments",
}


@pytest.fixture(scope="module")
def streams():
    import torch
    dev = torch.device("cuda", 0)
    a = torch.cuda.Stream(dev)
    U.calibrate(a)
    b = U.concurrency_control(a, [torch.cuda.Stream(dev) for _ in range(4)])
    yield a, b
    torch.cuda.synchronize()


def idmatte(c, s, key="node", region=REGION, spp=SPP):
    import torch
    h, w = region[3] - region[1], region[2] - region[0]
    return c.idmatte_device(region, spp, key, ids=filled(s, (h, w, 8), torch.int32), counts=filled(s, (h, w, 8), torch.int32),
                            other=filled(s, (h, w), torch.int32), samples=filled(s, (h, w), torch.int32), stream=s.cuda_stream)


def test_frame_and_id_matte_wait_for_each_other(streams):
    a, b = streams
    call = lambda st, s: idmatte(st["ctx"], s)   # noqa: E731
    setup = lambda: new_ctx(BOX3)   # noqa: E731
    U.ordered("frame_idmatte frame->pass", setup, frame_of(1), call, a, b, warm=warmed(call))
    U.ordered("frame_idmatte pass->frame", setup, call, frame_of(2), a, b, warm=warmed(call))


def test_an_id_matte_right_after_an_edit_sees_the_edited_scene(streams):
    """The node is moved while the frame the edit must wait for is held on a; the id matte on b right after is the moved scene's"""
    a, b = streams

    def setup():
        st = new_ctx(BOX3)
        st["old"], st["new"] = _moved_node(st["blob"])
        return st

    def warm(st, s):
        warm_frame(st, s)
        st["ctx"].edit_instances(*st["old"])   # (an edit that changes nothing: the pinned ring is made here)
        idmatte(st["ctx"], s)

    def consumer(st, s):
        st["ctx"].edit_instances(*st["new"])
        return idmatte(st["ctx"], s)

    _, new, _ = U.ordered("edit_instances_idmatte", setup, frame_of(1), consumer, a, b, warm=warm)
    # the matte of the scene before the edit differs, so a pass that had read the old tables would show
    st = setup()
    try:
        old = st["ctx"].idmatte(REGION, SPP, "node")
    finally:
        st["close"]()
    assert not np.array_equal(old["ids"], new["ids"]) or not np.array_equal(old["counts"].view(np.int32), new["counts"])


def test_the_progressive_id_matte_waits_for_the_frames_last_pass(streams):
    import torch
    a, b = streams

    def reader(st, s):
        return st["p"].idmatte_device("node", ids=filled(s, (H, W, 8), torch.int32), counts=filled(s, (H, W, 8), torch.int32),
                                      other=filled(s, (H, W), torch.int32), samples=filled(s, (H, W), torch.int32), stream=s.cuda_stream)
    # (warm: the reader once on the fresh frame, as the other readers of a progressive frame are warmed)
    _, got, _ = U.ordered("progressive_idmatte", _progressive(), _advance(4), reader, a, b, warm=reader, finish=_prog_state)
    assert (got["samples"] == 4).all()   # the pass that was held had finished: every pixel holds its four samples
