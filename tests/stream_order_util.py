"""Cross-stream ordering of a context's shared buffers: the stall-and-check harness of tests/test_gpu_stream_order.py, and the case
table it and tests/test_stream_order_closure.py are generated from (DESIGN.md "Streams: who waits for whom").

A case pairs a producer on stream a with a consumer on stream b that share state of one context.  Submitted back to back from one
thread, two short calls give the serial result whether or not the library orders them, so a lost wait would go unnoticed.  Here
stream a is first held busy (hold), so the producer really is late: a consumer that does not wait for it finishes first, which the
event order shows (ordered, step 3), and reads or tramples state the producer has not written yet, which the data show (step 4).

Importing this module imports neither torch nor qaray_amd: the closure test reads the table without a GPU."""
import time

# ---- the case table: case -> the entries of include/qaray_hip.h whose hip_stream argument the case puts on a late or a waiting
# stream.  The cases are the functions tests/test_gpu_stream_order.py registers under these names, run in this order (the two
# lifetime cases last: they end a scene and a context under a held frame)
CASES = {
    # frame <-> frame: lastFrame
    "frame_frame_box12": ("qa_render_region_device",),
    "frame_frame_box3": ("qa_render_region_device",),
    "frame_frame_object7": ("qa_render_region_device",),
    "frame_frame_chunked": ("qa_render_region_device",),
    "frame_frame_reshaped": ("qa_render_region_device",),
    "frame_frame_halton_grows": ("qa_render_region_device",),
    "frame_frame_stats": ("qa_render_region_device",),
    "frame_strips": ("qa_render_strips_device", "qa_render_region_device"),
    # frame <-> the read-only passes (LaunchSceneKernel and its like): lastFrame, both ways
    "frame_gbuffer": ("qa_gbuffer_region_device",),
    "frame_matte": ("qa_matte_region_device",),
    "frame_cast_rays": ("qa_cast_rays_device",),
    "frame_occluded": ("qa_occluded_device",),
    "frame_radiance_rays": ("qa_radiance_rays_device",),
    "frame_camera_rays": ("qa_camera_rays_device",),
    "frame_camera_sample_rays": ("qa_camera_sample_rays_device",),
    # edit <-> everything: lastEdit
    "edit_lights": ("qa_render_region_device", "qa_gbuffer_region_device"),
    "edit_camera": ("qa_render_region_device", "qa_gbuffer_region_device"),
    "edit_instances": ("qa_render_region_device", "qa_gbuffer_region_device"),
    "edit_under_held_context_stream": ("qa_scene_edit_texels_device", "qa_render_region_device", "qa_gbuffer_region_device"),
    "edit_after_empty_tiles": ("qa_empty_tiles_device",),
    # texture edit from device memory: texSource, lastEdit
    "edit_texels_device": ("qa_scene_edit_texels_device", "qa_render_region_device"),
    # the progressive frame: prog.done
    "progressive_readers": ("qa_progressive_advance", "qa_progressive_read_device", "qa_progressive_gbuffer_device", "qa_progressive_denoise_device",
                            "qa_progressive_denoise_guided_device", "qa_progressive_display_device", "qa_progressive_matte_device",
                            "qa_progressive_tile_levels_device"),
    "progressive_advance_advance": ("qa_progressive_advance",),
    "progressive_one_shot_between": ("qa_progressive_advance", "qa_render_region_device"),
    "progressive_tile_passes": ("qa_progressive_advance_tiles", "qa_progressive_advance_tiles_device", "qa_progressive_advance_adaptive",
                                "qa_progressive_tile_error_device"),
    # display, denoise, reproject: lastDisplay, lastDenoise, lastReproject
    "display_display": ("qa_display_device",),
    "denoise_denoise": ("qa_denoise_device", "qa_denoise_guided_device", "qa_denoise_variance_device"),
    "denoise_planes_grow": ("qa_denoise_device",),
    "reproject_reproject": ("qa_progressive_reproject_device", "qa_progressive_reproject_motion_device", "qa_progressive_reproject_moments_device"),
    # the host forms under a held device form of the same unit: lastFrame, the synchronize each ends with
    "host_forms": ("qa_render_region_device", "qa_cast_rays_device", "qa_occluded_device", "qa_radiance_rays_device", "qa_gbuffer_region_device",
                   "qa_matte_region_device"),
    # two contexts share nothing
    "two_contexts": ("qa_render_region_device",),
    # lifetime: the waits before memory is freed
    "upload_under_frame": ("qa_render_region_device",),
    "close_under_frame": ("qa_render_region_device",),
}

# entries with a hip_stream that no case needs, and why
EXEMPT = {
    "qa_reproject_device": "touches no state of the context: it reads and writes the caller's planes only, so there is nothing to order",
    "qa_reproject_motion_device": "as qa_reproject_device (the motion table is the caller's too)",
    "qa_reproject_moments_device": "as qa_reproject_device",
    "qa_matte_rgba_device": "touches no state of the context: one kernel over the caller's planes",
}

HOLD_FACTOR, HOLD_FLOOR_MS, HOLD_CAP_MS = 10.0, 20.0, 300.0

_cycles_per_ms = None
LOG = []   # every line say() printed, in order (the run's record: profiles/stream_order.txt)


def say(line):
    LOG.append(line)
    print("[stream-order] " + line, flush=True)


def _sleep_ms(stream, cycles):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate(stream):
    """Cycles of torch.cuda._sleep per millisecond, once per process: two sleeps of different length, timed with events; the slope
    (the launch's own time cancels).  Nothing about the clock is assumed: the lengths grow until the longer one takes 4 ms."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        short, long_ = 100_000, 500_000
        _sleep_ms(stream, short)   # (the kernel's first launch loads its code)
        while True:
            t0, t1 = _sleep_ms(stream, short), _sleep_ms(stream, long_)
            if t1 >= 4.0 or long_ >= 1 << 40:
                break
            short, long_ = short * 4, long_ * 4
        assert t1 > t0 > 0.0, f"torch.cuda._sleep does not scale with its argument: {short} cycles {t0} ms, {long_} cycles {t1} ms"
        _cycles_per_ms = (long_ - short) / (t1 - t0)
        say(f"calibration: sleep({short}) {t0:.3f} ms, sleep({long_}) {t1:.3f} ms -> {_cycles_per_ms:.0f} cycles per ms")
    return _cycles_per_ms


def hold(stream, ms):
    """Keeps `stream` busy for about `ms` milliseconds -> the event behind the hold (query() is False while it still runs)"""
    import torch
    cycles = int(ms * calibrate(stream))
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        end = torch.cuda.Event()
        end.record()
    return end


def hold_ms_for(consumer_ms):
    """The length of a case's hold: 10 x the consumer call's own time (submission and execution, as measured just before), so that
    both fall well inside it; at least 20 ms, at most 300 ms"""
    return min(max(HOLD_FACTOR * consumer_ms, HOLD_FLOOR_MS), HOLD_CAP_MS)


def runs_beside(a, b):
    """An unrelated kernel on b, submitted during a 50 ms hold on a: is it complete while the hold still runs?"""
    import torch
    x = torch.zeros(256, device=torch.device("cuda", a.device_index))
    with torch.cuda.stream(b):
        x.add_(1.0)   # (b's first use makes its queue, which may take longer than the hold: not what is asked here)
    torch.cuda.synchronize()
    end = hold(a, 50.0)
    with torch.cuda.stream(b):
        x.add_(1.0)
    b.synchronize()
    beside = not end.query()
    a.synchronize()
    assert float(x.sum().item()) == 512.0
    return beside


def concurrency_control(a, candidates):
    """Do the two streams of the module really run side by side?  If they shared a hardware queue, a kernel on b would wait for a
    hold on a whatever the library does, and every ordered() case would pass vacuously.  The runtime deals its hardware queues out
    to streams as it sees fit, so b is the first of `candidates` (streams of torch's pool) that passes runs_beside(a, b); if none
    does, the module fails here -> b"""
    for i, b in enumerate(candidates):
        beside = runs_beside(a, b)
        say(f"concurrency control: candidate {i} for b: add_ on b complete during a 50 ms hold on a: {beside}")
        if beside:
            return b
    raise AssertionError("no stream runs side by side with stream a (a kernel on b waited for a hold on a): they share a hardware queue, and every case "
                         "of this module would pass vacuously")


def _host(v):
    """A result as bytes-comparable host data: tensors and arrays to numpy, containers element by element"""
    if v is None or isinstance(v, (int, float, str, bool)):
        return v
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_host(x) for x in v]
    if hasattr(v, "detach"):
        return v.detach().cpu().numpy().copy()
    return v


def differences(x, y, path=""):
    """-> the paths at which two _host() results differ bit for bit"""
    import numpy as np
    if isinstance(x, dict):
        return [d for k in x for d in differences(x[k], y[k], f"{path}.{k}")] if isinstance(y, dict) and x.keys() == y.keys() else [path + " (keys)"]
    if isinstance(x, list):
        return [d for i, (p, q) in enumerate(zip(x, y)) for d in differences(p, q, f"{path}[{i}]")] if isinstance(y, list) and len(x) == len(y) else [path + " (length)"]
    if isinstance(x, np.ndarray):
        same = isinstance(y, np.ndarray) and x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        return [] if same else [path]
    return [] if x == y else [path]


def ordered(name, setup, producer, consumer, a, b, blocking=False, waits=True, warm=True, serial=None, finish=None):
    """The core check.  setup() -> a fresh state (contexts, inputs; its "close" entry, if any, is called at the end); producer(state,
    stream) and consumer(state, stream) enqueue on the torch stream they are given and return their outputs (tensors, arrays, dicts
    or lists of them); finish(state), if given, returns more to compare once both streams are drained (host reads, counters).

    First the serial run, on a state of its own: warm-up, producer, consumer, all on stream a - the reference, and where the
    consumer's own time is measured (an event pair around it on a, and the wall time of the call, whichever is longer).  Then, on a
    fresh state:
      1. a hold on a, the producer on a, the event pa behind it;
      2. the consumer on b, the event cb behind it;
      3. cb is synchronised, and pa must then be complete: the consumer cannot have finished before the producer (waits=False:
         the two share nothing, and nothing is asserted here);
      4. both calls' data are bit for bit the serial run's.
    The hold must still run when the consumer returns (blocking=True, a consumer that blocks the host by design: when it is
    called) - a failure, not a skip: otherwise steps 3 and 4 would pass whatever the library does.
    warm: the producer runs once on a before the hold, in both runs (what a context does on a first call only - allocations, the
    tile order's upload and its synchronize - must not block the producer behind the hold); a callable runs instead; False: nothing.
    serial: a callable(state, stream) -> (producer's, consumer's) results that replaces the serial run's two calls.
    -> (producer's, consumer's, finish's) results of the serial run, as host data"""
    import torch

    def run(concurrent, hold_ms=0.0):
        st = setup()
        try:
            if callable(warm):
                warm(st, a)
            elif warm:
                producer(st, a)
            torch.cuda.synchronize()
            if not concurrent:
                if serial:
                    rp, rc = serial(st, a)
                    ms = 0.0
                else:
                    rp = producer(st, a)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(a)
                    t0 = time.perf_counter()
                    rc = consumer(st, a)
                    wall = (time.perf_counter() - t0) * 1e3
                    e1.record(a)
                    e1.synchronize()
                    ms = max(e0.elapsed_time(e1), wall)
                torch.cuda.synchronize()
                kept.append((rp, rc))   # (until the comparison: the concurrent run's outputs then come from other memory)
                return _host(rp), _host(rc), _host(finish(st)) if finish else None, ms
            end = hold(a, hold_ms)
            rp = producer(st, a)
            pa = torch.cuda.Event()
            pa.record(a)
            if blocking:
                assert not end.query(), f"{name}: the {hold_ms:.0f} ms hold on a ended before the consumer was called: the case shows nothing"
            rc = consumer(st, b)
            if not blocking:
                assert not end.query(), f"{name}: the {hold_ms:.0f} ms hold on a ended before the consumer returned: the case shows nothing"
            cb = torch.cuda.Event()
            cb.record(b)
            cb.synchronize()
            if waits:
                assert pa.query(), f"{name}: EVENT ORDER: the consumer on b finished before the producer on a had: it did not wait for it"
            torch.cuda.synchronize()
            return _host(rp), _host(rc), _host(finish(st)) if finish else None, 0.0
        finally:
            torch.cuda.synchronize()
            if st.get("close"):
                st["close"]()

    kept = []
    sp, sc, sf, ms = run(False)
    hold_ms = hold_ms_for(ms)
    say(f"{name}: consumer {ms:.3f} ms -> hold {hold_ms:.0f} ms")
    cp, cc, cf, _ = run(True, hold_ms)
    bad = differences(sp, cp, "producer") + differences(sc, cc, "consumer") + differences(sf, cf, "finish")
    assert not bad, f"{name}: DATA: differs from the serial run at {bad}"
    return sp, sc, sf
