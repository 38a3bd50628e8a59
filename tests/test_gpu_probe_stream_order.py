"""Cross-stream ordering of the light-probe entries, on the stall-and-check harness of tests/stream_order_util.py and in the pattern of
tests/test_gpu_irradiance_stream_order.py (DESIGN.md "Streams: who waits for whom"): one stream is held busy, the call on the other
must have waited for it - by the order of two events, and by the bits of both results against the same two calls run serially.

qa_probe_sh_device traces its chunks through qa_radiance_rays_device (LaunchRayBatch): behind the context's last frame and last edit
(lastFrame, lastEdit).  Its scratch is one per context: the call waits for lastFrame before the first kernel writes it and records
lastFrame behind its last reduction, so that a later edit - and a later probe call on another stream - waits for it.

The two shading entries read and write only arrays of the caller's: there is nothing of the context's to order.

The table of tests/stream_order_util.py lists the entries that take a `hip_stream`; the entries here call it `stream` and have their
table here: CASES (test -> the entries it puts on a late or a waiting stream) and EXEMPT (entry -> why there is nothing to order).
tests/test_probe_stream_closure.py holds the header to the two, without a GPU."""
import numpy as np
import pytest

import stream_order_util as U
from test_gpu_stream_order import BOX3, H, REGION, W, _moved_node, filled, frame_of, new_ctx, warm_frame

pytestmark = pytest.mark.gpu

CASES = {
    "test_frame_and_probes_wait_for_each_other": ("qa_probe_sh_device",),               # lastFrame, both ways
    "test_probes_right_after_an_edit_see_the_edited_scene": ("qa_probe_sh_device",),   # lastEdit (and lastFrame behind it)
    "test_a_later_edit_waits_for_the_probes": ("qa_probe_sh_device",),                  # lastFrame, the other way
    "test_two_probe_calls_share_the_scratch_in_turn": ("qa_probe_sh_device",),          # lastFrame: the scratch
}
EXEMPT = {
    "qa_probe_shade_device": "reads the caller's coefficients, normals and index and writes the caller's rgb: no buffer of the context's is touched",
    "qa_probe_grid_shade_device": "reads the caller's coefficients, points and normals and writes the caller's rgb: no buffer of the context's is touched",
}

N, M = 64, 2
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
    """The lit box with the node _moved_node moves; probes at the midpoints of 64 camera rays that hit, spread over the frame"""
    import torch
    st = new_ctx(BOX3)
    st["old"], st["new"] = _moved_node(st["blob"])
    c = st["ctx"]
    n = H * W
    r = c.camera_sample_rays_device(REGION, 0, 1, outputs=("origins", "dirs"))
    o, d = r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3)
    got = c.cast_rays_device(o, d, t=torch.empty((n,), device="cuda"))
    c.synchronize()
    hit = torch.nonzero(got["t"] < 1e30).reshape(-1)
    pick = hit[torch.linspace(0, len(hit) - 1, N).long()]
    st["points"] = (o[pick] + 0.5 * got["t"][pick, None] * d[pick]).contiguous()
    torch.cuda.synchronize()
    return st


def probes(st, s, seed=1):
    import torch
    return st["ctx"].probe_sh_device(st["points"], M, SPP, BOUNCES, seed, sh=filled(s, (N, 9, 3), torch.float32), hits=filled(s, (N,), torch.int32),
                                     tmin=filled(s, (N,), torch.float32), chunk_rays=16 * 6 * M * M, stream=s.cuda_stream)


def warm(st, s):
    warm_frame(st, s)
    st["ctx"].edit_instances(*st["old"])   # (an edit that changes nothing: the pinned ring is made here)
    probes(st, s)                          # (and the scratch)


def moved_then_probes(st, s):
    st["ctx"].edit_instances(*st["new"])
    return probes(st, s)


def on_the_scene_as_uploaded():
    import torch
    st = setup()
    try:
        out = probes(st, torch.cuda.current_stream())
        st["ctx"].synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        st["close"]()


def test_frame_and_probes_wait_for_each_other(streams):
    a, b = streams
    U.ordered("frame_probe_sh frame->probes", setup, frame_of(1), probes, a, b, warm=warm)
    U.ordered("frame_probe_sh probes->frame", setup, probes, frame_of(2), a, b, warm=warm)


def test_probes_right_after_an_edit_see_the_edited_scene(streams):
    """The node is moved while the frame the edit must wait for is held on a; the probes on b right after see the moved scene"""
    a, b = streams
    _, new, _ = U.ordered("edit_instances_probe_sh", setup, frame_of(1), moved_then_probes, a, b, warm=warm)
    old = on_the_scene_as_uploaded()
    assert (new["sh"] != 0).any()
    # the light at the same probes of the scene before the edit differs, so a call that had read the old tables would show
    assert not np.array_equal(old["sh"].view(np.uint32), new["sh"].view(np.uint32))


def test_a_later_edit_waits_for_the_probes(streams):
    """The probes are held on a; the edit that follows on the context's stream, and the probes of the moved scene on b, come after
    them: the held call saw the scene before the move"""
    a, b = streams
    old, new, _ = U.ordered("probe_sh_edit_instances", setup, probes, moved_then_probes, a, b, warm=warm)
    want = on_the_scene_as_uploaded()
    assert np.array_equal(old["sh"].view(np.uint32), want["sh"].view(np.uint32)) and np.array_equal(old["hits"], want["hits"])
    assert not np.array_equal(old["sh"].view(np.uint32), new["sh"].view(np.uint32))


def test_two_probe_calls_share_the_scratch_in_turn(streams):
    """Two calls with different seeds, four chunks each, on two streams: the second writes the scratch only once the first has
    reduced its last chunk - both have the bits of the serial run"""
    a, b = streams
    first, second, _ = U.ordered("probe_sh_probe_sh", setup, probes, lambda st, s: probes(st, s, seed=2), a, b, warm=warm)
    assert not np.array_equal(first["sh"].view(np.uint32), second["sh"].view(np.uint32))
