"""Reprojection with luminance moments and a shortened length on the device (qa_reproject_moments_device,
qa_progressive_reproject_moments_device: the kernel qa_reproject_k<2> of qa_reproject.hip): the device build of
qa_reproject_moments_dev.h equals the host build (qa_test_reproject_moments_host, pinned to a restatement of the specification by
tests/test_reproject_moments_host.py) bit for bit on every output plane; on a progressive frame's slabs; and through
hip.TemporalPreview on the renderer's own frames, where the shortened length lets go of the history a light edit made wrong."""
import os

import numpy as np
import pytest

import reproject_motion_util as mu
import reproject_util as ru
from conftest import ensure_assets
from reproject_moments_util import call_moments, moments_inputs
from reproject_motion_util import call_motion
from reproject_util import bits

pytestmark = pytest.mark.gpu

# a lone pixel; a partial 16x16 tile on both axes; three tiles by three, ragged, the clamp's halo crossing tile borders at r = 1 and 3
SIZES = ((1, 1), (17, 13), (33, 35))
ORIGINS = ((0, 0), (5, 3))
FLAGS = (dict(moments=True), dict(motion=False, clamp=True, shorten=True, clamp_radius=1),
         dict(motion=False, clamp=True, moments=True, clamp_radius=3, clamp_gamma=0.5, min_frames=2.0),
         dict(clamp=True, moments=True, shorten=True, clamp_radius=3, shorten_rate=0.5), dict(clamp=True, moments=True, shorten=True, clamp_radius=1))
NAMES = ("out", "length", "moments", "variance")


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def host(a, motion=True, **kw):
    from qaray_amd import hip
    return call_moments(hip.reproject_moments_host, a, motion=motion, **kw)


def device(ctx, a, motion=True, stream=None, **kw):
    """Context.reproject_moments_device on a dict of moments_inputs() -> the four planes as numpy (None for a plane that was not
    written); every input is compared bitwise afterwards."""
    import torch
    host_side = [*a["cur"], *a["hist"], a["ids"], a["hist_ids"]] + ([a["hist_moments"]] if a.get("hist_moments") is not None else [])
    t = [to_device(x) for x in host_side]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    res = ctx.reproject_moments_device(tuple(t[0:3]), tuple(t[3:6]), a["c0"], a["c1"], origin=a["origin"], ids=t[6], hist_ids=t[7],
                                       hist_moments=t[8] if len(t) > 8 else None, motion=a["motion"] if motion else None,
                                       stream=stream.cuda_stream if stream is not None else None, **kw)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    for k, (x, y) in enumerate(zip(t, host_side)):
        assert np.array_equal(bits(x.cpu().numpy()), bits(y)), k
    return tuple(None if x is None else x.cpu().numpy() for x in res)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            bad = np.argwhere(bits(g) != bits(w))
            assert bad.size == 0, (what, name, len(bad), bad[:5])


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_host_bit_for_bit(ctx, w, h, origin):
    import torch
    side = torch.cuda.Stream()
    for still in (False, True):
        a = moments_inputs(w=w, h=h, origin=origin, seed=100 * w + h + origin[0], still=still)
        a["motion"] = mu.all_moved_motion()
        for flags in FLAGS:
            want = host(a, **flags)
            assert want[2] is not None or not flags.get("moments")
            for stream in (None, side):
                assert_same(device(ctx, a, stream=stream, **flags), want, (still, flags, stream is not None))
        no_plane = dict(a, hist_moments=None)
        assert_same(device(ctx, no_plane, **FLAGS[3]), host(no_plane, **FLAGS[3]), (still, "no moments plane"))


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_edges_equal_the_host_bit_for_bit_with_all_four_flags(ctx, name, a):
    h, w = a["cur"][1].shape
    mom = np.random.default_rng(5).random((h, w, 2), dtype=np.float32)
    mom[h // 2, w // 2] = np.nan
    a = dict(a, motion=mu.all_moved_motion(), hist_moments=mom)
    for flags in (dict(clamp=True, moments=True, shorten=True, clamp_radius=2), dict(clamp=True, moments=True, shorten=True, clamp_radius=3, shorten_rate=4.0)):
        got = device(ctx, a, **flags)
        assert_same(got, host(a, **flags), (name, flags))
        fin = np.isfinite(a["cur"][0]).all(-1)
        assert np.isfinite(got[1]).all() and np.isfinite(got[0][fin]).all() and np.isfinite(got[2]).all() and np.isfinite(got[3]).all()


def test_new_flags_off_on_the_device_are_the_motion_call(ctx):
    a = moments_inputs(seed=7)
    t = [to_device(x) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])]
    for flags in (dict(), dict(clamp=True, clamp_radius=2), dict(motion=a["motion"], clamp=True)):
        want = ctx.reproject_motion_device(tuple(t[0:3]), tuple(t[3:6]), a["c0"], a["c1"], ids=t[6], hist_ids=t[7], **flags)
        got = ctx.reproject_moments_device(tuple(t[0:3]), tuple(t[3:6]), a["c0"], a["c1"], ids=t[6], hist_ids=t[7], hist_moments=to_device(a["hist_moments"]),
                                           **flags)
        ctx.synchronize()
        assert got[2] is None and got[3] is None
        assert_same(tuple(x.cpu().numpy() for x in got[:2]), tuple(x.cpu().numpy() for x in want), flags.keys())


def test_ids_outside_the_table_never_address_it(ctx):
    a = moments_inputs(seed=23)
    a["motion"] = mu.all_moved_motion()
    count = len(a["motion"])
    word = np.array([-1, count, count + 7, np.iinfo(np.int32).min, 0, 1, 2, np.iinfo(np.int32).max], np.int32)
    a["ids"][..., 0] = word[np.random.default_rng(5).integers(0, len(word), a["ids"].shape[:2])]
    a["hist_ids"][...] = a["ids"]    # (so that pixels of every id keep taps)
    flags = dict(clamp=True, moments=True, shorten=True)
    assert_same(device(ctx, a, **flags), host(a, **flags), "all ids")
    one = dict(a, motion=a["motion"][:1])
    assert_same(device(ctx, one, **flags), host(one, **flags), "one record")
    assert (bits(host(one, **flags)[0]) != bits(host(a, **flags)[0])).any()


def test_parameters_reach_the_kernel(ctx):
    from qaray_amd import hip
    a = moments_inputs(seed=21)
    base = dict(clamp=True, moments=True, shorten=True)
    for kw in (dict(base, min_frames=1.5), dict(base, shorten_rate=3.0, clamp_gamma=2.0), dict(base, depth_tolerance=0.5, max_history=2.5),
               dict(params=hip.ReprojectMomentsParams.of(max_history=7, clamp=True, clamp_radius=3, moments=True, shorten=True, min_frames=2, shorten_rate=0.25))):
        assert_same(device(ctx, a, **kw), host(a, **kw), kw)
    few, many = device(ctx, a, **dict(base, min_frames=1.0)), device(ctx, a, **dict(base, min_frames=5.0))
    assert_same(few[:3], many[:3], "min_frames changes the variance alone")
    assert ((few[3] >= 0) & (many[3] == -1)).mean() > 0.1
    slow, fast = device(ctx, a, **dict(base, shorten_rate=0.0)), device(ctx, a, **dict(base, shorten_rate=4.0))
    assert (bits(slow[1]) != bits(fast[1])).mean() > 0.3 and (fast[1] <= slow[1]).all()


def test_refused_calls_on_the_device(ctx):
    from qaray_amd import hip
    a = moments_inputs(seed=41)
    t = [to_device(x) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"], a["hist_moments"])]
    cur, hist = tuple(t[0:3]), tuple(t[3:6])
    for kw in (dict(shorten=True), dict(clamp=True, shorten=True, shorten_rate=-1.0), dict(moments=True, min_frames=0.5), dict(moments=True, out_moments=t[8]),
               dict(moments=True, out_variance=t[5]), dict(moments=True, clamp=True, out=t[0]), dict(motion=a["motion"], moments=True),
               dict(clamp=True, clamp_radius=4)):
        with pytest.raises(hip.HipError) as e:
            ctx.reproject_moments_device(cur, hist, a["c0"], a["c1"], hist_moments=t[8], **kw)
        assert e.value.code == -1, kw
    p = hip.ReprojectMomentsParams.default()
    p.flags = 16
    with pytest.raises(hip.HipError) as e:
        ctx.reproject_moments_device(cur, hist, a["c0"], a["c1"], params=p)
    assert e.value.code == -1 and "flags" in str(e.value)
    assert ctx.reproject_moments_device(cur, hist, a["c0"], a["c1"], hist_moments=t[8], moments=True, out=t[0])[0] is t[0]   # in place without the clamp
    ctx.synchronize()


def test_a_smaller_frame_after_a_larger_one_gives_the_same_bits():
    from qaray_amd import hip
    c = hip.Context(0)   # (its own context, as the old calls' tests)
    try:
        flags = dict(clamp=True, clamp_radius=3, moments=True, shorten=True)
        small, large = moments_inputs(w=7, h=5, origin=(30, 28), seed=31), moments_inputs(seed=32)
        first = device(c, small, **flags)
        assert_same(device(c, large, **flags), host(large, **flags), "large")
        assert_same(device(c, small, **flags), first, "small again")
        assert_same(first, host(small, **flags), "small")
    finally:
        c.close()


def host_scene(name, size):
    from qaray_amd.host import SCENES_DIR, HostScene
    ensure_assets()
    return HostScene(os.path.join(SCENES_DIR, name), size=size)


def test_progressive_frames_equal_the_plain_call_and_are_not_changed(ctx):
    import torch
    from qaray_amd import hip
    hs = host_scene(mu.PREVIEW_SCENE, (64, 48))
    blob = hs.flatten()
    cam = hs.camera().copy()
    hs.close()
    ctx.upload_scene(blob)
    region = (5, 3, 52, 43)
    h, w = 40, 47
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")   # noqa: E731
    with ctx.progressive(region, 4) as prog:
        prog.advance(4)
        rgb0, depth0, ns0 = prog.read()
        ids0 = prog.gbuffer_device(ids=new((h, w, 2), torch.int32))["ids"]
        ctx.synchronize()
        l0 = (0.2126 * rgb0[..., 0] + 0.7152 * rgb0[..., 1] + 0.0722 * rgb0[..., 2]).astype(np.float32)
        mom0 = np.stack([l0, l0 * l0 + np.float32(0.01)], axis=-1)
        history = tuple(to_device(x) for x in (rgb0, depth0, 4 * ns0.astype(np.float32)))
        hmom = to_device(mom0)
        prog.restart()
        prog.advance(4)
        before = prog.read()
        frame = (new((h, w, 3)), new((h, w)), new((h, w), torch.int32))
        prog.read_device(*frame)
        ids1 = prog.gbuffer_device(ids=new((h, w, 2), torch.int32))["ids"]
        ctx.synchronize()
        side = torch.cuda.Stream()
        for flags in (dict(moments=True), dict(clamp=True, clamp_radius=2, moments=True, shorten=True), dict(clamp=True, clamp_radius=3, shorten=True)):
            plain = ctx.reproject_moments_device(frame, history, cam, cam, origin=(5, 3), ids=ids1, hist_ids=ids0, hist_moments=hmom, **flags)
            ctx.synchronize()
            want = tuple(None if x is None else x.cpu().numpy() for x in plain)
            assert_same(want, hip.reproject_moments_host(before, (rgb0, depth0, 4 * ns0.astype(np.float32)), cam, cam, origin=(5, 3), ids=ids1.cpu().numpy(),
                                                         hist_ids=ids0.cpu().numpy(), hist_moments=mom0, **flags), (flags.keys(), "host"))
            if flags.get("moments"):
                assert (want[3] >= 0).mean() > 0.5
            for stream in (None, side):
                got = prog.reproject_moments_device(history, cam, hist_ids=ids0, hist_moments=hmom, stream=stream.cuda_stream if stream else None, **flags)
                stream.synchronize() if stream else ctx.synchronize()
                assert_same(tuple(None if x is None else x.cpu().numpy() for x in got), want, (flags.keys(), stream is not None))
        after = prog.read()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, after))


# ---- hip.TemporalPreview on the renderer's own frames ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soft_blob():
    hs = host_scene(mu.PREVIEW_SCENE, mu.PREVIEW_SIZE)
    blob = hs.flatten()
    hs.close()
    return blob


def preview_frames(ctx, blob, count, make):
    """`count` frames of 4 spp of a still camera pushed through make() -> a hip.TemporalPreview; -> the planes after every push."""
    import torch
    from qaray_amd import hip
    w, h = mu.PREVIEW_SIZE
    region = (0, 0, w, h)
    ctx.upload_scene(blob)
    cam = hip.blob_camera(blob).copy()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    rgb, depth = torch.empty((h, w, 3), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev)
    ns, ids = torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tp = make(region)
    seen = []
    for k in range(count):
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=50 + k, stream=s.cuda_stream)
        ctx.gbuffer_device(region, 50 + k, ids=ids, stream=s.cuda_stream)
        acc, length = tp.push(cam, rgb, depth, ns, ids, stream=s.cuda_stream)
        s.synchronize()
        seen.append((acc.cpu().numpy(), length.cpu().numpy(), None if tp.variance is None else tp.variance.cpu().numpy()))
    return seen, tp


@pytest.mark.parametrize("clamp", (False, True))
def test_a_preview_without_moments_and_shorten_is_todays_preview(ctx, soft_blob, clamp):
    import torch
    from qaray_amd import hip
    w, h = mu.PREVIEW_SIZE
    region = (0, 0, w, h)
    ctx.upload_scene(soft_blob)
    cam = hip.blob_camera(soft_blob).copy()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    rgb, depth = torch.empty((h, w, 3), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev)
    ns, ids = torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tp = hip.TemporalPreview(ctx, region, clamp=clamp, moments=False, shorten=False)
    assert tp.moments_params is None
    acc = length = None
    for k in range(3):
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=50 + k, stream=s.cuda_stream)
        ctx.gbuffer_device(region, 50 + k, ids=ids, stream=s.cuda_stream)
        prev = None if acc is None else (acc.clone(), tp._depth.clone(), length.clone(), tp._ids.clone())
        acc, length = tp.push(cam, rgb, depth, ns, ids, stream=s.cuda_stream)
        s.synchronize()
        assert tp.variance is None
        if prev is not None:    # the push is the call it was before, on the same planes
            if clamp:
                want = ctx.reproject_motion_device((rgb, depth, ns), prev[:3], cam, cam, ids=ids, hist_ids=prev[3], clamp=True, stream=s.cuda_stream)
            else:
                want = ctx.reproject_device((rgb, depth, ns), prev[:3], cam, cam, ids=ids, hist_ids=prev[3], stream=s.cuda_stream)
            s.synchronize()
            assert torch.equal(want[0], acc) and torch.equal(want[1], length)
    assert float(length.mean()) > 11
    # and the moments leave the colour and the length as they are, plane for plane
    plain, _ = preview_frames(ctx, soft_blob, 3, lambda region: hip.TemporalPreview(ctx, region, clamp=clamp))
    with_moments, _ = preview_frames(ctx, soft_blob, 3, lambda region: hip.TemporalPreview(ctx, region, clamp=clamp, moments=True))
    for k, (a, b) in enumerate(zip(plain, with_moments)):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), k
    assert np.array_equal(bits(plain[2][0]), bits(acc.cpu().numpy()))


def test_a_previews_variance_plane(ctx, soft_blob):
    from qaray_amd import hip
    seen, tp = preview_frames(ctx, soft_blob, 5, lambda region: hip.TemporalPreview(ctx, region, moments=True))
    assert (seen[0][2] == -1).all() and (seen[2][2] == -1).all()        # the first push; three frames behind a pixel
    for acc, length, variance in seen[3:]:    # trusted: four frames' worth of samples behind the pixel (the scene has a lens, so sample 0 of
        assert np.array_equal(variance >= 0, length >= 16) and ((variance >= 0) | (variance == -1)).all()    # an edge pixel changes sides with the seed)
    assert (seen[3][2] >= 0).mean() > 0.8 and (seen[4][2] > 0).mean() > 0.3
    tp.reset()
    # after reset(): the next push is a first push again
    import torch
    w, h = mu.PREVIEW_SIZE
    dev = torch.device("cuda", 0)
    rgb, depth = torch.ones((h, w, 3), dtype=torch.float32, device=dev), torch.full((h, w), 5.0, dtype=torch.float32, device=dev)
    ns = torch.full((h, w), 4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    acc, length = tp.push(hip.blob_camera(soft_blob).copy(), rgb, depth, ns)
    assert (tp.variance.cpu().numpy() == -1).all() and (length.cpu().numpy() == 4).all()


def test_the_shortened_length_lets_go_of_the_history_a_light_edit_made_wrong(ctx, soft_blob):
    """Scenario (b) of DESIGN.md 4k: the light quartered before frame 5 of 8, luma RMSE of the last preview to the 256-spp frame of the
    dimmed scene, the same frames (seeds) through the clamp alone and through the clamp with the shortened length.  Measured on one
    MI355X: 0.0420 with the shortened length (defaults; mean length 20.5), 0.0471 with the clamp alone (31.3), 0.0420 for the last raw frame."""
    short, clamp = mu.preview_run(ctx, soft_blob, "light", clamp=True, shorten=True), mu.preview_run(ctx, soft_blob, "light", clamp=True)
    assert np.array_equal(bits(short["truth"]), bits(clamp["truth"])) and np.array_equal(bits(short["raw"]), bits(clamp["raw"]))
    e_short, e_clamp, e_raw = (mu.luma_rmse(x, short["truth"]) for x in (short["acc"], clamp["acc"], short["raw"]))
    print(f"light quartered before frame 5: luma RMSE to the 256-spp frame: clamp + shorten {e_short:.4f}, clamp alone {e_clamp:.4f}, raw 4-spp {e_raw:.4f}; "
          f"mean length {short['length'].mean():.1f} against {clamp['length'].mean():.1f}")
    assert e_short < e_clamp


def test_the_shortened_length_keeps_most_of_a_still_scenes_gain(ctx, soft_blob):
    """Scenario (c) of DESIGN.md 4k: a still scene; below the midpoint of the raw frame's and the unclamped preview's RMSE, computed in
    the same run.  Measured on one MI355X: 0.0546 (mean length 29.1), no clamp 0.0547 (31.3), raw 0.0593, midpoint 0.0570."""
    short, off = mu.preview_run(ctx, soft_blob, "still", clamp=True, shorten=True), mu.preview_run(ctx, soft_blob, "still", clamp=False)
    e_short, e_off, e_raw = (mu.luma_rmse(x, short["truth"]) for x in (short["acc"], off["acc"], short["raw"]))
    print(f"still scene: luma RMSE to the 256-spp frame: clamp + shorten {e_short:.4f}, no clamp {e_off:.4f}, raw 4-spp {e_raw:.4f}, "
          f"midpoint {0.5 * (e_raw + e_off):.4f}; mean length {short['length'].mean():.1f} against {off['length'].mean():.1f}")
    assert e_short < 0.5 * (e_raw + e_off)
