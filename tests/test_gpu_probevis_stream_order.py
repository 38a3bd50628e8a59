"""Cross-stream ordering of the probe-visibility entries: the four cases of tests/test_gpu_probe_stream_order.py - its scene, its
probes, its harness (tests/stream_order_util.py) - with qa_probevis_sh_device in qa_probe_sh_device's place.  The call is that call
with one more kernel per chunk, on the same stream, behind the chunk's reduction and before the next chunk's rays overwrite the
scratch: it waits for lastFrame and lastEdit and records lastFrame exactly as the plain call does, and the moments - which are read
from the scratch - are the output that would show a chunk overwritten too early.

qa_probevis_grid_shade_device reads and writes only arrays of the caller's.

CASES (test -> the entries it puts on a late or a waiting stream) and EXEMPT (entry -> why there is nothing to order);
tests/test_probevis_stream_closure.py holds the header to the two, without a GPU."""
import numpy as np
import pytest

import stream_order_util as U
from test_gpu_probe_stream_order import BOUNCES, M, N, SPP, setup, streams  # noqa: F401  (streams: the module's fixture)
from test_gpu_stream_order import filled, frame_of, warm_frame

pytestmark = pytest.mark.gpu

CASES = {
    "test_frame_and_probes_wait_for_each_other": ("qa_probevis_sh_device",),               # lastFrame, both ways
    "test_probes_right_after_an_edit_see_the_edited_scene": ("qa_probevis_sh_device",),   # lastEdit (and lastFrame behind it)
    "test_a_later_edit_waits_for_the_probes": ("qa_probevis_sh_device",),                  # lastFrame, the other way
    "test_two_probe_calls_share_the_scratch_in_turn": ("qa_probevis_sh_device",),          # lastFrame: the scratch, which the moments read
}
EXEMPT = {
    "qa_probevis_grid_shade_device": "reads the caller's coefficients, moments, points and normals and writes the caller's rgb: no buffer of the context's is touched",
}

D, DMAX = 2, 1.0e4   # (beyond every distance of the scene: nothing is clamped but the misses, so a moved node moves the moments)


def probes(st, s, seed=1):
    import torch
    return st["ctx"].probevis_sh_device(st["points"], D, DMAX, M, SPP, BOUNCES, seed, sh=filled(s, (N, 9, 3), torch.float32),
                                        hits=filled(s, (N,), torch.int32), tmin=filled(s, (N,), torch.float32),
                                        moments=filled(s, (N, 6, D, D, 2), torch.float32), chunk_rays=16 * 6 * M * M, stream=s.cuda_stream)


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


def differ(a, b, key):
    return not np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32))


def test_frame_and_probes_wait_for_each_other(streams):  # noqa: F811
    a, b = streams
    U.ordered("frame_probevis_sh frame->probes", setup, frame_of(1), probes, a, b, warm=warm)
    U.ordered("frame_probevis_sh probes->frame", setup, probes, frame_of(2), a, b, warm=warm)


def test_probes_right_after_an_edit_see_the_edited_scene(streams):  # noqa: F811
    """The node is moved while the frame the edit must wait for is held on a; the probes on b right after see the moved scene"""
    a, b = streams
    _, new, _ = U.ordered("edit_instances_probevis_sh", setup, frame_of(1), moved_then_probes, a, b, warm=warm)
    old = on_the_scene_as_uploaded()
    assert (new["sh"] != 0).any() and (new["moments"] > 0).any()
    # the same probes of the scene before the edit see other light and other distances: a call that had read the old tables would show
    assert differ(old, new, "sh") and differ(old, new, "moments")


def test_a_later_edit_waits_for_the_probes(streams):  # noqa: F811
    """The probes are held on a; the edit that follows on the context's stream, and the probes of the moved scene on b, come after
    them: the held call saw the scene before the move"""
    a, b = streams
    old, new, _ = U.ordered("probevis_sh_edit_instances", setup, probes, moved_then_probes, a, b, warm=warm)
    want = on_the_scene_as_uploaded()
    assert not differ(old, want, "sh") and not differ(old, want, "moments") and np.array_equal(old["hits"], want["hits"])
    assert differ(old, new, "sh") and differ(old, new, "moments")


def test_two_probe_calls_share_the_scratch_in_turn(streams):  # noqa: F811
    """Two calls with different seeds, four chunks each, on two streams: the second writes the scratch only once the first has
    reduced and pooled its last chunk - both have the bits of the serial run.  (The seed moves the light, not the first hits: the
    moments of the two calls are equal, their coefficients are not.)"""
    a, b = streams
    first, second, _ = U.ordered("probevis_sh_probevis_sh", setup, probes, lambda st, s: probes(st, s, seed=2), a, b, warm=warm)
    assert differ(first, second, "sh")
