"""Reprojection with node motion and colour clamp on the device (qa_reproject_motion_device, qa_progressive_reproject_motion_device:
the kernel qa_reproject_k<1> of qa_reproject.hip): the device build of qa_reproject_motion_dev.h equals the host build
(qa_test_reproject_motion_host, pinned to a restatement of the specification by tests/test_reproject_motion_host.py) bit for bit, at
the sizes where the clamp's staged halo is wider than the frame, fills one tile and crosses tiles; on a progressive frame's slabs;
and through hip.TemporalPreview on the renderer's own frames, previews follow moved nodes and drop the history a light edit made
wrong."""
import os

import numpy as np
import pytest

import reproject_motion_util as mu
import reproject_util as ru
from conftest import ensure_assets
from reproject_motion_util import call_motion, motion_inputs
from reproject_util import bits

pytestmark = pytest.mark.gpu

# one thread; narrower than the halo; one full tile; the halo crosses tiles; three tiles by two, ragged
SIZES = ((1, 1), (3, 2), (16, 16), (17, 17), (33, 20))
ORIGINS = ((0, 0), (5, 3))
FLAGS = (dict(motion=True), dict(motion=False, clamp=True, clamp_radius=1), dict(motion=False, clamp=True, clamp_radius=3, clamp_gamma=0.5),
         dict(motion=True, clamp=True, clamp_radius=2))


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
    return call_motion(hip.reproject_motion_host, a, motion=motion, **kw)


def device(ctx, a, motion=True, stream=None, alias=False, table_on_device=False, **kw):
    """Context.reproject_motion_device on a dict of motion_inputs() -> (out, length) as numpy; every input is compared bitwise
    afterwards (the current colour too unless the output was written over it)."""
    import torch
    host_side = [*a["cur"], *a["hist"], a["ids"], a["hist_ids"]]
    t = [to_device(x) for x in host_side]
    table = a["motion"] if motion else None
    if table is not None and table_on_device:
        table = to_device(table.view(np.uint8))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out, length = ctx.reproject_motion_device(tuple(t[0:3]), tuple(t[3:6]), a["c0"], a["c1"], origin=a["origin"], ids=t[6], hist_ids=t[7], motion=table,
                                              out=t[0] if alias else None, stream=stream.cuda_stream if stream is not None else None, **kw)
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
    side = torch.cuda.Stream()
    for still in (False, True):
        a = motion_inputs(w, h, origin, seed=100 * w + h + origin[0], still=still)
        for table in (a["motion"], mu.all_moved_motion()):    # the sphere alone (it is outside the smallest frames); every node
            b = dict(a, motion=table)
            for flags in FLAGS:
                want = host(b, **flags)
                for stream in (None, side):
                    assert_same(device(ctx, b, stream=stream, table_on_device=stream is None, **flags), want, (still, flags, stream is not None))
                if not flags.get("clamp"):    # in place: without the clamp only
                    assert_same(device(ctx, b, alias=True, **flags), want, (still, flags, "in place"))


def test_flags_0_on_the_device_are_the_old_call(ctx):
    from qaray_amd import hip
    a = motion_inputs(seed=7)
    assert_same(device(ctx, a, motion=False), call_motion(hip.reproject_motion_host, a, motion=False), "flags 0")
    assert_same(device(ctx, a, motion=False), ru.call(hip.reproject_host, a), "the old form")


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_edges_equal_the_host_bit_for_bit(ctx, name, a):
    a = dict(a, motion=mu.all_moved_motion())
    for flags in (dict(motion=True, clamp=True, clamp_radius=2), dict(motion=True), dict(motion=False, clamp=True, clamp_radius=3)):
        out, length = device(ctx, a, **flags)
        assert_same((out, length), host(a, **flags), (name, flags))
        fin = np.isfinite(a["cur"][0]).all(-1)
        assert np.isfinite(length).all() and np.isfinite(out[fin]).all()


def test_ids_outside_the_table_never_address_it(ctx):
    a = motion_inputs(seed=23)
    a["motion"] = mu.all_moved_motion()
    count = len(a["motion"])
    word = np.array([-1, count, count + 7, np.iinfo(np.int32).min, 0, 1, 2, np.iinfo(np.int32).max], np.int32)
    a["ids"][..., 0] = word[np.random.default_rng(5).integers(0, len(word), a["ids"].shape[:2])]
    a["hist_ids"][...] = a["ids"]    # (so that pixels of every id keep taps)
    for flags in (dict(motion=True), dict(motion=True, clamp=True, clamp_radius=1)):
        got = device(ctx, a, **flags)
        assert_same(got, host(a, **flags), flags)
    # the table's records are used for the ids inside it alone: with the table cut to one record, ids 1 and 2 are unmoved too
    one = dict(a, motion=a["motion"][:1])
    assert_same(device(ctx, one), host(one), "one record")
    assert (bits(host(one)[0]) != bits(host(a)[0])).any()


def test_parameters_reach_the_kernel(ctx):
    from qaray_amd import hip
    a = motion_inputs(seed=21)
    for kw in (dict(clamp=True, clamp_radius=2, clamp_gamma=0.0), dict(clamp=True, clamp_gamma=2.5, depth_tolerance=0.5, max_history=2.5),
               dict(params=hip.ReprojectMotionParams.of(max_history=7, clamp=True, clamp_radius=3))):
        assert_same(device(ctx, a, **kw), host(a, **kw), kw)
    tight, loose = device(ctx, a, clamp=True, clamp_gamma=0.0)[0], device(ctx, a, clamp=True, clamp_gamma=3.0)[0]
    assert (bits(tight) != bits(loose)).mean() > 0.3


def test_refused_calls_on_the_device(ctx):
    import torch
    from qaray_amd import hip
    a = motion_inputs(seed=41)
    t = [to_device(x) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])]
    cur, hist = tuple(t[0:3]), tuple(t[3:6])
    table = to_device(a["motion"].view(np.uint8))
    for kw in (dict(motion=a["motion"]), dict(motion=a["motion"], ids=t[6]), dict(clamp=True, clamp_radius=4), dict(clamp=True, clamp_gamma=-1.0),
               dict(clamp=True, out=t[0])):
        with pytest.raises(hip.HipError) as e:
            ctx.reproject_motion_device(cur, hist, a["c0"], a["c1"], **kw)
        assert e.value.code == -1, kw
    big = torch.zeros((ru.H, ru.W, 16), dtype=torch.float32, device="cuda")    # 64 bytes per pixel: a table and a colour plane at once
    with pytest.raises(hip.HipError) as e:
        ctx.reproject_motion_device(cur, hist, a["c0"], a["c1"], ids=t[6], hist_ids=t[7], motion=big, out=big.view(-1)[:3 * ru.H * ru.W].view(ru.H, ru.W, 3))
    assert e.value.code == -1 and "motion table" in str(e.value)
    assert ctx.reproject_motion_device(cur, hist, a["c0"], a["c1"], ids=t[6], hist_ids=t[7], motion=table, out=t[0])[0] is t[0]   # in place: allowed
    ctx.synchronize()


def test_a_smaller_frame_after_a_larger_one_gives_the_same_bits():
    from qaray_amd import hip
    c = hip.Context(0)   # (its own context, as the old call's test)
    try:
        flags = dict(clamp=True, clamp_radius=3)
        small, large = motion_inputs(7, 5, (30, 28), seed=31), motion_inputs(seed=32)
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
        inst0 = hip.blob_table(ctx.download_scene(), "instances").copy()
        inst1 = inst0.copy()
        inst1[mu.NODE_S1]["pos"] += np.array([0.5, 0.0, 0.25], np.float32)
        ctx.edit_instances(mu.NODE_S1, inst1[mu.NODE_S1:mu.NODE_S1 + 1])
        table = hip.node_motion(inst0, inst1)
        assert table["moved"].tolist() == [0, 0, 1, 0, 0, 0, 0]
        history = tuple(to_device(x) for x in (rgb0, depth0, ns0.astype(np.float32)))
        with pytest.raises(hip.HipError):   # stale: the pixels are the old scene's
            prog.reproject_motion_device(history, cam, hist_ids=ids0, motion=table)
        prog.restart()
        prog.advance(4)
        before = prog.read()
        frame = (new((h, w, 3)), new((h, w)), new((h, w), torch.int32))
        prog.read_device(*frame)
        ids1 = prog.gbuffer_device(ids=new((h, w, 2), torch.int32))["ids"]
        ctx.synchronize()
        side = torch.cuda.Stream()
        for flags in (dict(motion=table), dict(motion=table, clamp=True, clamp_radius=2), dict(clamp=True, clamp_radius=3)):
            plain = ctx.reproject_motion_device(frame, history, cam, cam, origin=(5, 3), ids=ids1, hist_ids=ids0, **flags)
            ctx.synchronize()
            want = tuple(x.cpu().numpy() for x in plain)
            assert_same(want, hip.reproject_motion_host(before, (rgb0, depth0, ns0.astype(np.float32)), cam, cam, origin=(5, 3), ids=ids1.cpu().numpy(),
                                                        hist_ids=ids0.cpu().numpy(), **flags), (flags.keys(), "host"))
            if "motion" in flags:
                s1 = ids1.cpu().numpy()[..., 0] == mu.NODE_S1
                assert s1.sum() > 50 and (want[1] > 4)[s1].mean() > 0.5    # the moved sphere finds its history
            for stream in (None, side):
                out, length = prog.reproject_motion_device(history, cam, hist_ids=ids0, stream=stream.cuda_stream if stream else None, **flags)
                stream.synchronize() if stream else ctx.synchronize()
                assert_same((out.cpu().numpy(), length.cpu().numpy()), want, (flags.keys(), stream is not None))
        after = prog.read()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, after))


# ---- quality: the renderer's own previews through hip.TemporalPreview ------------------------------------------------------------

@pytest.fixture(scope="module")
def soft_blob():
    hs = host_scene(mu.PREVIEW_SCENE, mu.PREVIEW_SIZE)
    blob = hs.flatten()
    hs.close()
    return blob


def test_previews_follow_moved_nodes_without_a_reset(ctx, soft_blob):
    """Measured on one MI355X: s1 moves 0.15 and group turns one degree before each of seven frames.  Luma RMSE to the 256-spp frame
    of the final scene 0.0588 for the last raw 4-spp frame (what a reset after every edit shows), 0.0532 accumulated; 487 pixels show a
    node that moved, their mean length 31.1 of 32 samples (the others' 30.9; asserted > 2 * 4)."""
    r = mu.preview_run(ctx, soft_blob, "nodes")
    e_raw, e_acc = mu.luma_rmse(r["raw"], r["truth"]), mu.luma_rmse(r["acc"], r["truth"])
    moved = r["moved"]
    print(f"node moves: luma RMSE to the 256-spp frame: raw 4-spp {e_raw:.4f}, accumulated {e_acc:.4f}; pixels of moved nodes {moved.sum()}, their mean "
          f"length {r['length'][moved].mean():.1f}, the others' {r['length'][~moved].mean():.1f}")
    assert moved.sum() > 300
    assert e_acc < e_raw
    assert r["length"][moved].mean() > 2 * mu.PREVIEW_SPP


def test_the_clamp_drops_the_history_a_light_edit_made_wrong(ctx, soft_blob):
    """Measured on one MI355X: luma RMSE to the 256-spp frame of the dimmed scene 0.0471 with the clamp (defaults: radius 1, gamma 1),
    0.1231 without it (four of eight frames of history show the light at four times its strength), 0.0420 for the last raw frame."""
    on, off = mu.preview_run(ctx, soft_blob, "light", clamp=True), mu.preview_run(ctx, soft_blob, "light", clamp=False)
    assert np.array_equal(bits(on["truth"]), bits(off["truth"]))
    e_on, e_off, e_raw = mu.luma_rmse(on["acc"], on["truth"]), mu.luma_rmse(off["acc"], off["truth"]), mu.luma_rmse(on["raw"], on["truth"])
    print(f"light quartered before frame 5: luma RMSE to the 256-spp frame: clamp on {e_on:.4f}, clamp off {e_off:.4f}, raw 4-spp {e_raw:.4f}")
    assert e_on < e_off


def test_the_clamp_keeps_most_of_a_still_scenes_gain(ctx, soft_blob):
    """Measured on one MI355X: luma RMSE to the 256-spp frame 0.0593 for the last raw frame, 0.0547 accumulated without the clamp,
    0.0544 with it (asserted: below their midpoint, 0.0570).  DESIGN.md 4j has the table for radius 1, 2 x gamma 1, 2, 3."""
    on, off = mu.preview_run(ctx, soft_blob, "still", clamp=True), mu.preview_run(ctx, soft_blob, "still", clamp=False)
    e_on, e_off, e_raw = mu.luma_rmse(on["acc"], on["truth"]), mu.luma_rmse(off["acc"], off["truth"]), mu.luma_rmse(on["raw"], on["truth"])
    print(f"still scene: luma RMSE to the 256-spp frame: clamp on {e_on:.4f}, clamp off {e_off:.4f}, raw 4-spp {e_raw:.4f}, midpoint {0.5 * (e_raw + e_off):.4f}")
    assert np.array_equal(on["length"], off["length"])    # the clamp leaves the length as it is
    assert e_off < e_raw
    assert e_on < 0.5 * (e_raw + e_off)


def test_a_preview_without_clamp_and_instances_is_the_old_preview(ctx, soft_blob):
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
    tp = hip.TemporalPreview(ctx, region)
    acc = length = None
    for k in range(3):
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=50 + k, stream=s.cuda_stream)
        ctx.gbuffer_device(region, 50 + k, ids=ids, stream=s.cuda_stream)
        prev = None if acc is None else (acc.clone(), tp._depth.clone(), length.clone(), tp._ids.clone())
        acc, length = tp.push(cam, rgb, depth, ns, ids, stream=s.cuda_stream)
        s.synchronize()
        if prev is not None:    # the push is the old call on the same planes
            want = ctx.reproject_device((rgb, depth, ns), prev[:3], cam, cam, ids=ids, hist_ids=prev[3], stream=s.cuda_stream)
            s.synchronize()
            assert torch.equal(want[0], acc) and torch.equal(want[1], length)
    assert float(length.mean()) > 11
