"""Temporal reprojection on the device (qa_reproject_device, qa_progressive_reproject_device: qa_reproject.hip): the device build of
qa_reproject_dev.h equals the host build (qa_test_reproject_host, pinned to a restatement of the specification and to an analytic
scene by tests/test_reproject_host.py) bit for bit, on plain frames and on a progressive frame's slabs; the frames it reads are
never changed; on the renderer's own guide planes the history lands on the surface it came from; a turntable of 4-spp frames
through hip.TemporalPreview ends nearer the converged frame than its last raw frame."""
import os

import numpy as np
import pytest

import reproject_util as ru
from conftest import ensure_assets
from reproject_util import BOUND, bits, call, inputs, restate

pytestmark = pytest.mark.gpu

BOX = "example_project12_box.xml"
SIZES = ((1, 1), (7, 5), (33, 17), (67, 45))   # one thread; less than a tile; three tiles by two, ragged; the host test's frame
ORIGINS = ((0, 0), (5, 3))


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def to_device(a):
    import torch
    dev = torch.device("cuda", 0)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)


def device(ctx, a, ids=True, stream=None, alias=False, **kw):
    """Context.reproject_device on a dict of reproject_util.inputs() -> (out, length) as numpy; every input is compared bitwise
    afterwards (the current colour too unless the output was written over it)."""
    import torch
    host_side = [*a["cur"], *a["hist"], a["ids"], a["hist_ids"]]
    t = [to_device(x) for x in host_side]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out, length = ctx.reproject_device(tuple(t[0:3]), tuple(t[3:6]), a["c0"], a["c1"], origin=a["origin"], ids=t[6] if ids else None,
                                       hist_ids=t[7] if ids else None, out=t[0] if alias else None,
                                       stream=stream.cuda_stream if stream is not None else None, **kw)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    for k, (x, y) in enumerate(zip(t, host_side)):
        if not (alias and k == 0):
            assert np.array_equal(bits(x.cpu().numpy()), bits(y)), k
    return out.cpu().numpy(), length.cpu().numpy()


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("out", "length")):
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, (what, name, len(bad), bad[:5])


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_host_bit_for_bit(ctx, w, h, origin):
    import torch
    from qaray_amd import hip
    side = torch.cuda.Stream()
    for still in (False, True):
        a = inputs(w, h, origin, seed=100 * w + h + origin[0], still=still)
        for ids in (True, False):
            want = call(hip.reproject_host, a, ids)
            for stream in (None, side):
                for alias in (False, True):
                    assert_same(device(ctx, a, ids, stream, alias), want, (still, ids, stream is not None, alias))


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_edges_equal_the_host_bit_for_bit(ctx, name, a):
    from qaray_amd import hip
    for ids in (True, False):
        out, length = device(ctx, a, ids)
        assert_same((out, length), call(hip.reproject_host, a, ids), (name, ids))
        fin = np.isfinite(a["cur"][0]).all(-1)
        assert np.isfinite(length).all() and np.isfinite(out[fin]).all()


def test_parameters_reach_the_kernel(ctx):
    from qaray_amd import hip
    a = inputs(seed=21)
    for kw in (dict(depth_tolerance=0.0), dict(depth_tolerance=0.5, max_history=2.5), dict(params=hip.ReprojectParams.of(max_history=7))):
        assert_same(device(ctx, a, True, **kw), call(hip.reproject_host, a, True, **kw), kw)
    loose, tight = device(ctx, a, False, depth_tolerance=0.5)[1], device(ctx, a, False, depth_tolerance=0.0)[1]
    assert (loose > 4).sum() > (tight > 4).sum()


def test_a_smaller_frame_after_a_larger_one_gives_the_same_bits():
    from qaray_amd import hip
    c = hip.Context(0)   # (its own context, as the filter's test of its working planes)
    try:
        small, large = inputs(7, 5, (30, 28), seed=31), inputs(seed=32)
        first = device(c, small)
        assert_same(device(c, large), call(hip.reproject_host, large), "large")
        assert_same(device(c, small), first, "small again")
        assert_same(first, call(hip.reproject_host, small), "small")
    finally:
        c.close()


def test_refused_calls_on_the_device(ctx):
    from qaray_amd import hip
    a = inputs(seed=41)
    t = [to_device(x) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])]
    cur, hist = tuple(t[0:3]), tuple(t[3:6])
    for kw in (dict(out=t[3]), dict(out_length=t[5]), dict(out_length=t[4]), dict(out_length=t[1]), dict(ids=t[6]), dict(hist_ids=t[7]),
               dict(max_history=0.0), dict(depth_tolerance=-1.0)):
        with pytest.raises(hip.HipError) as e:
            ctx.reproject_device(cur, hist, a["c0"], a["c1"], **kw)
        assert e.value.code == -1, kw
    with pytest.raises(hip.HipError):   # a side beyond 2^24
        ctx.reproject_device(cur, hist, a["c0"], a["c1"], origin=(1 << 24, 0))
    assert ctx.reproject_device(cur, hist, a["c0"], a["c1"], out=t[0])[0] is t[0]   # in place: allowed
    ctx.synchronize()


def turned(pos, target, degrees):
    """pos turned about the z axis through target (the box and the texture scene have z up)."""
    p, t = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    a = np.radians(degrees)
    d = p - t
    return t + np.array([d[0] * np.cos(a) - d[1] * np.sin(a), d[0] * np.sin(a) + d[1] * np.cos(a), d[2]])


def host_scene(name, size):
    from qaray_amd.host import SCENES_DIR, HostScene
    ensure_assets()
    return HostScene(os.path.join(SCENES_DIR, name), size=size)


def test_progressive_frames_are_reprojected_from_their_slabs_and_not_changed(ctx):
    import torch
    from qaray_amd import hip
    hs = host_scene("custom_textures.xml", (64, 48))
    pos, target, up = (2.0, -38.0, 14.0), (0.0, 0.0, 3.0), (0.0, 0.0, 1.0)
    hs.set_camera(pos, target, up)
    cam0 = hs.camera().copy()
    ctx.upload_scene(hs.flatten())
    region = (5, 3, 52, 43)
    with ctx.progressive(region, 4) as prog:
        prog.advance(4)
        rgb0, depth0, ns0 = prog.read()
        ids0 = prog.gbuffer_device(ids=torch.empty((40, 47, 2), dtype=torch.int32, device="cuda"))["ids"]
        ctx.synchronize()
        hs.set_camera(turned(pos, target, 2.0), target, up)
        cam1 = hs.camera().copy()
        ctx.edit_camera(cam1)
        history = (rgb0, depth0, ns0.astype(np.float32))
        dev_history = tuple(to_device(x) for x in history)
        with pytest.raises(hip.HipError):   # stale: the pixels are the old camera's
            prog.reproject_device(dev_history, cam0)
        prog.restart()
        prog.advance(4)
        before = prog.read()
        ids1 = prog.gbuffer_device(ids=torch.empty((40, 47, 2), dtype=torch.int32, device="cuda"))["ids"]
        ctx.synchronize()
        side = torch.cuda.Stream()
        for with_ids in (True, False):
            kw = dict(ids=ids1.cpu().numpy(), hist_ids=ids0.cpu().numpy()) if with_ids else {}
            want = hip.reproject_host(before, history, cam0, cam1, origin=(5, 3), **kw)
            assert (want[1] > 4).mean() > 0.5    # most of the frame finds its history
            for stream in (None, side):
                out, length = prog.reproject_device(dev_history, cam0, hist_ids=ids0 if with_ids else None, stream=stream.cuda_stream if stream else None)
                stream.synchronize() if stream else ctx.synchronize()
                assert_same((out.cpu().numpy(), length.cpu().numpy()), want, (with_ids, stream is not None))
        after = prog.read()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, after))
        for x, y in zip(dev_history, history):
            assert np.array_equal(bits(x.cpu().numpy()), bits(y))
    hs.close()


BOX_POS, BOX_TARGET, BOX_UP = (0.0, -65.0, 11.0), (0.0, 0.0, 11.0), (0.0, 0.0, 1.0)


def test_the_renderers_own_planes_carry_albedo_to_the_surface_it_came_from(ctx):
    hs = host_scene(BOX, (64, 64))
    region = (0, 0, 64, 64)
    views = []
    ctx.upload_scene(hs.flatten())
    for degrees in (0.0, 3.0):
        hs.set_camera(turned(BOX_POS, BOX_TARGET, degrees), BOX_TARGET, BOX_UP)
        cam = hs.camera().copy()
        ctx.edit_camera(cam)
        views.append((cam, ctx.gbuffer(region)))
    hs.close()
    (cam0, g0), (cam1, g1) = views
    a = dict(c0=cam0, c1=cam1, cur=(np.zeros((64, 64, 3), np.float32), g1["depth"], np.ones((64, 64), np.uint32)),
             hist=(g0["albedo"], g0["depth"], np.full((64, 64), 63, np.float32)), origin=(0, 0), ids=g1["ids"], hist_ids=g0["ids"])
    out, length = device(ctx, a, True, max_history=64)
    R = call(restate, a, True, max_history=64)
    has = length > 1.5
    ch = out.astype(np.float64) * (64.0 / 63.0)
    full = has & R["has"] & (R["taps"] == 4) & ~R["undecided"]
    hit = g1["depth"] != ru.MISS
    assert full.sum() > 0.5 * hit.sum()
    assert np.abs(ch - g1["albedo"])[full].max() <= BOUND * g1["albedo"].max()
    share, want = has[hit].mean(), R["has"][hit].mean()
    print(f"view-1 hit pixels with history: {share:.4f} on the device, {want:.4f} in the restatement; all four taps: {full.sum()} pixels")
    assert want > 0.8 and abs(share - want) <= 0.02


def luma(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def test_a_turntable_of_previews_ends_nearer_the_converged_frame(ctx):
    """Measured on one MI355X: RMSE of luma to the 256-spp frame 0.9286 for the last raw 4-spp frame, 0.5280 for the accumulated one
    (raw / sqrt(8), what eight still frames would give: 0.3283; the midpoint asserted below: 0.6285); mean length 31.0."""
    import torch
    from qaray_amd import hip
    hs = host_scene(BOX, (64, 64))
    region = (0, 0, 64, 64)
    ctx.upload_scene(hs.flatten())
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream()
    rgb = torch.empty((64, 64, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((64, 64), dtype=torch.float32, device=dev)
    ns = torch.empty((64, 64), dtype=torch.int32, device=dev)
    ids = torch.empty((64, 64, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tp = hip.TemporalPreview(ctx, region)
    sync = hip.TemporalPreview(ctx, region)   # the same pushes without a stream of the caller's
    for k in range(8):
        hs.set_camera(turned(BOX_POS, BOX_TARGET, float(k)), BOX_TARGET, BOX_UP)
        cam = hs.camera().copy()
        ctx.edit_camera(cam)
        seed = 1000 + k
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=seed, stream=s.cuda_stream)
        ctx.gbuffer_device(region, seed, ids=ids, stream=s.cuda_stream)
        acc, length = tp.push(cam, rgb, depth, ns, ids, stream=s.cuda_stream)
        s.synchronize()
        if k == 0:
            assert np.array_equal(bits(acc.cpu().numpy()), bits(rgb.cpu().numpy())) and np.array_equal(length.cpu().numpy(), ns.cpu().numpy())
        if k < 3:
            acc2, length2 = sync.push(cam, rgb, depth, ns, ids)
            assert torch.equal(acc2, acc) and torch.equal(length2, length)
    raw, accumulated, lengths = rgb.cpu().numpy(), acc.cpu().numpy(), length.cpu().numpy()
    hs.close()
    converged = ctx.render_region(region, 256, seed=77)[0]
    rmse = lambda x: float(np.sqrt(np.mean((luma(x.astype(np.float64)) - luma(converged.astype(np.float64))) ** 2)))   # noqa: E731
    e_raw, e_acc = rmse(raw), rmse(accumulated)
    print(f"luma RMSE to the 256-spp frame: raw 4-spp {e_raw:.4f}, accumulated {e_acc:.4f}, raw / sqrt(8) {e_raw / np.sqrt(8):.4f}; "
          f"mean length {lengths.mean():.1f}")
    assert lengths.max() <= 32.001 and lengths.mean() > 16   # (eight frames of 4; the weighted mean of equal lengths rounds)
    assert e_acc < e_raw
    assert e_acc < 0.5 * (e_raw + e_raw / np.sqrt(8.0))
    tp.reset()
    acc, length = tp.push(cam, rgb, depth, ns, ids, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(bits(acc.cpu().numpy()), bits(raw)) and np.array_equal(length.cpu().numpy(), ns.cpu().numpy())
