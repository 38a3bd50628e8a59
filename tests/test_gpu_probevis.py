"""Probe visibility on the device (qa_lightprobe.hip: qa_probevis_sh*, qa_probevis_grid_shade_device; the opening comment of
qa_probevis_dev.h is the specification).  The anchor: probevis_sh_device gives probe_sh_device's sh, cube, hits and tmin bit for bit,
and its moments are the numpy pooling (tests/probevis_util.py) of the t that radiance_rays_device returns for the rays of
probe_directions_host - the composition of tests/test_gpu_probe.py's anchor, so no ray is traced that the plain call does not trace.
The rest: independence of batch, order and chunking, void probes, counters and refusals, the shading kernel against its host form,
and the two rooms of tests/golden/probevis, where a wall stands between the light and half of the probes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gbuffer_util import REGION, SEEDS, bits, scene_blob
from probe_util import MISS
from probevis_util import ROOMS_D, ROOMS_GRID, ROOMS_M, moments_ref, rooms_points
from radiance_util import QA_EINVAL, QA_ENOSCENE, anchor_blob
from ray_query_util import fresh
from test_gpu_probe import ANCHOR, IDS, LIT_BOX, dev, differing, fused, probe_points

pytestmark = pytest.mark.gpu

DMAX = 25.0   # (the anchor's scenes measure tens of units: some rays are clamped, some are not, the misses always)


def rays_t(c, P, S, m, spp, max_bounce, seed, jitter):
    """t (n, K) of the probes' rays as radiance_rays_device returns it for probe_directions_host's directions and streams"""
    from qaray_amd import hip
    n, K = len(P), 6 * m * m
    S = np.arange(n, dtype=np.uint32) if S is None else np.asarray(S, np.uint32)
    d, _, _ = hip.probe_directions_host(m, S, seed, jitter)
    sid = ((S.astype(np.uint64)[:, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    o = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, K, 3)), np.float32)
    _, t, _ = c.radiance_rays_device(dev(o.reshape(-1, 3)), dev(d.reshape(-1, 3)), spp, max_bounce, seed, stream_ids=dev(sid.reshape(-1)), miss_environment=True)
    c.synchronize()
    return t.cpu().numpy().reshape(n, K)


def pooled(t, P, m, d, dmax):
    """The moments the specification asks for: zeros for a void probe"""
    out = np.stack([moments_ref(t[q], m, d, dmax) for q in range(len(P))])
    out[~np.isfinite(P).all(axis=1)] = 0
    return out


def visfused(c, P, S, m, d, spp, max_bounce, seed, jitter, dmax=DMAX, cube=True, **kw):
    got = c.probevis_sh_device(dev(P), d, dmax, m, spp, max_bounce, seed, jitter, stream_ids=None if S is None else dev(np.asarray(S, np.uint32)),
                               cube=cube or None, **kw)
    c.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "hits" else v.cpu().numpy()) for k, v in got.items()}


@pytest.mark.parametrize("scene", list(ANCHOR))
def test_the_moments_pool_the_t_of_the_plain_calls_rays(scene):
    """Five probes (the camera position and the midpoints of four camera rays that hit); (m, d) = (1, 1), (4, 2), (6, 3), (6, 6); spp 1
    with centres and the probes' indices as stream ids, spp 3 with jitter and ids at both ends of 32 bits."""
    c = fresh(anchor_blob(scene))
    try:
        P = probe_points(c)
        for m, d in ((1, 1), (4, 2), (6, 3), (6, 6)):
            for spp, seed, S, jitter in ((1, SEEDS[0], None, False), (3, SEEDS[1], IDS, True)):
                plain = fused(c, P, S, m, spp, 5, seed, jitter)
                t = rays_t(c, P, S, m, spp, 5, seed, jitter)
                # the t behind the moments is the t behind tmin; dmax in the middle of it, so that rays fall on both sides
                assert np.array_equal(bits(t.min(axis=1)), bits(plain["tmin"])) and (t < MISS).any()
                dmax = np.float32(np.median(t[t < MISS]))
                got = visfused(c, P, S, m, d, spp, 5, seed, jitter, dmax=float(dmax))
                assert set(got) == set(plain) | {"moments"} and not differing(got, plain), (scene, m, d, spp, differing(got, plain))
                want = pooled(t, P, m, d, dmax)
                assert got["moments"].shape == (5, 6, d, d, 2) and np.array_equal(bits(got["moments"]), bits(want)), (scene, m, d, spp)
                assert (got["moments"][..., 0] <= dmax).all() and (got["moments"][..., 0] > 0).all()
    finally:
        c.close()


def test_moments_do_not_depend_on_chunks_batch_or_order():
    """chunk_rays = 1, 100 and 0 give equal bits for n = 5 at m = 4, d = 2; batches of 1, 2 and 5 give per-probe results equal to the
    largest batch's, a permutation with its stream ids the permuted results; the host form equals the device form; without sh
    (NULL in the C call) the other outputs keep their bits; d and dmax matter."""
    import torch
    from qaray_amd import hip
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        kw = dict(m=4, d=2, spp=2, max_bounce=3, seed=SEEDS[1], jitter=True)
        whole = visfused(c, P, IDS, **kw)
        assert (whole["moments"] > 0).all() and len(np.unique(whole["moments"].reshape(5, -1), axis=0)) == 5
        for chunk_rays in (1, 100, 0):
            assert not differing(visfused(c, P, IDS, chunk_rays=chunk_rays, **kw), whole), chunk_rays
            assert not differing(visfused(c, P, IDS, chunk_rays=chunk_rays, cube=False, **kw), whole), chunk_rays
        for n in (1, 2, 5):
            assert not differing(visfused(c, P[:n], IDS[:n], **kw), {k: v[:n] for k, v in whole.items()}), n
        perm = np.random.default_rng(5).permutation(5)
        assert not differing(visfused(c, P[perm], IDS[perm], chunk_rays=200, **kw), {k: v[perm] for k, v in whole.items()})
        host = c.probevis_sh(P, kw["d"], DMAX, kw["m"], kw["spp"], kw["max_bounce"], kw["seed"], kw["jitter"], stream_ids=IDS, cube=True)
        assert set(host) == set(whole) and not differing(host, whole)
        assert not differing(c.probevis_sh(P, kw["d"], DMAX, kw["m"], kw["spp"], kw["max_bounce"], kw["seed"], True, stream_ids=IDS, chunk_rays=100), whole)
        # sh = NULL: moments, hits and tmin alone, on the device and from the host
        L = hip.lib()
        par, vis = hip.ProbeParams.of(4, 2, 3, SEEDS[1], True, chunk_rays=100), hip.ProbeVisParams.of(2, DMAX)
        tp, ids = dev(P), dev(IDS)
        mo = torch.full((5, 6, 2, 2, 2), 7.0, device="cuda:0")
        hits = torch.full((5,), 7, dtype=torch.int32, device="cuda:0")
        tmin = torch.full((5,), 7.0, device="cuda:0")
        assert L.qa_probevis_sh_device(c._h, 5, tp.data_ptr(), ids.data_ptr(), C.byref(par), C.byref(vis), None, None, hits.data_ptr(), tmin.data_ptr(),
                                       mo.data_ptr(), None) == 0
        c.synchronize()
        assert np.array_equal(bits(mo.cpu().numpy()), bits(whole["moments"])) and np.array_equal(hits.cpu().numpy().view(np.uint32), whole["hits"])
        assert np.array_equal(bits(tmin.cpu().numpy()), bits(whole["tmin"]))
        hmo = np.full((5, 6, 2, 2, 2), 7, np.float32)
        assert L.qa_probevis_sh(c._h, 5, P.ctypes.data, IDS.ctypes.data, C.byref(par), C.byref(vis), None, None, None, None, hmo.ctypes.data) == 0
        assert np.array_equal(bits(hmo), bits(whole["moments"]))
        for change in (dict(d=4), dict(d=1), dict(dmax=3.0)):
            other = visfused(c, P, IDS, **{**kw, **change})
            assert other["moments"].shape != whole["moments"].shape or not np.array_equal(bits(other["moments"]), bits(whole["moments"])), change
            assert not differing({k: v for k, v in other.items() if k != "moments"}, whole), change
    finally:
        c.close()


def test_void_probes_have_zero_moments_and_disturb_nothing():
    """Nine void probes (NaN, +inf and -inf in each component) among ten good ones: their moments are +0, the others keep their bits,
    in chunks of one probe and in one chunk"""
    c = fresh(scene_blob(LIT_BOX))
    try:
        good = probe_points(c, 9)
        void = np.repeat(good[:1], 9, axis=0)
        for i, bad in enumerate((np.nan, np.inf, -np.inf)):
            for k in range(3):
                void[3 * i + k, k] = bad
        P = np.insert(good, np.arange(9), void, axis=0)
        isvoid = ~np.isfinite(P).all(axis=1)
        assert isvoid.sum() == 9 and len(P) == 19
        ids = np.zeros(len(P), np.uint32)
        ids[~isvoid] = 100 + np.arange(len(good))
        ids[isvoid] = 7
        kw = dict(m=6, d=3, spp=2, max_bounce=2, seed=SEEDS[0], jitter=True)
        alone = visfused(c, good, ids[~isvoid], **kw)
        assert (alone["moments"] > 0).all()
        for chunk_rays, cube in ((0, True), (1, False), (500, False)):
            got = visfused(c, P, ids, chunk_rays=chunk_rays, cube=cube, **kw)
            assert not bits(got["moments"][isvoid]).any() and not bits(got["sh"][isvoid]).any()
            assert not differing({k: v[~isvoid] for k, v in got.items()}, alone), (chunk_rays, cube)
    finally:
        c.close()


def test_counters_launches_and_refusals():
    """The counters and the launch count move as for the plain call on the same arguments; every refusal of the C ABI - the plain
    call's and the moments' own - leaves every output alone."""
    import torch
    from qaray_amd import hip
    L = hip.lib()
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        n, m, K, d = len(P), 4, 96, 2
        moved = []
        for call in (lambda **kw: c.probe_sh(P, m=m, **kw), lambda **kw: c.probevis_sh(P, d, DMAX, m=m, **kw)):
            row = []
            for kw in (dict(spp=3, max_bounce=0), dict(spp=2, chunk_rays=2 * K)):
                c.reset_counters()
                launches0 = c.kernel_time()[1]
                call(**kw)
                row.append((c.counters(), c.kernel_time()[1] - launches0))
            moved.append(row)
        assert moved[0] == moved[1], moved
        assert moved[1][0][0]["samples"] == n * K * 3 and moved[1][0][1] == 1 and moved[1][1][1] == 3   # (chunks of 2, 2 and 1 probes)

        tp = dev(P)
        sh = torch.full((n, 9, 3), 7.0, device="cuda:0")
        cube = torch.full((n, 6, m, m, 3), 7.0, device="cuda:0")
        hits = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
        tmin = torch.full((n,), 7.0, device="cuda:0")
        mo = torch.full((n, 6, d, d, 2), 7.0, device="cuda:0")
        pp_, psh, pcube, phits, ptmin, pmo = (x.data_ptr() for x in (tp, sh, cube, hits, tmin, mo))
        par, vis = hip.ProbeParams.of(m=m), hip.ProbeVisParams.of(d, DMAX)
        pp, pv = C.byref(par), C.byref(vis)
        device = lambda h, n, *a: L.qa_probevis_sh_device(h, n, *a, None)   # noqa: E731
        hsh, hmo = np.full((n, 9, 3), 7, np.float32), np.full((n, 6, d, d, 2), 7, np.float32)
        hp = P.ctypes.data
        hostcall = lambda n, pts, par, vis, mo: L.qa_probevis_sh(c._h, n, pts, None, par, vis, hsh.ctypes.data, None, None, None, mo)   # noqa: E731
        # n == 0 launches nothing and needs no array
        assert device(c._h, 0, None, None, None, None, None, None, None, None, None) == 0
        assert L.qa_probevis_sh(c._h, 0, None, None, None, None, None, None, None, None, None) == 0
        assert c.probevis_sh(np.zeros((0, 3)), 2, 1.0, m=4)["moments"].shape == (0, 6, 2, 2, 2)
        # what the plain call refuses, the same way
        for args in ((1 << 31, pp_, None, pp, pv, psh, pcube, phits, ptmin, pmo), (n, None, None, pp, pv, psh, pcube, phits, ptmin, pmo),
                     (n, pp_, None, None, pv, psh, pcube, phits, ptmin, pmo)):
            assert device(c._h, *args) == QA_EINVAL, args
        for field, bad in (("spp", 0), ("max_bounce", -1), ("m", 0), ("m", 129), ("flags", 1), ("flags", 1 << 31)):
            q = hip.ProbeParams.of(m=m)
            setattr(q, field, bad)
            assert device(c._h, n, pp_, None, C.byref(q), pv, psh, pcube, phits, ptmin, pmo) == QA_EINVAL, (field, bad)
            assert hostcall(n, hp, C.byref(q), pv, hmo.ctypes.data) == QA_EINVAL, (field, bad)
        assert device(None, n, pp_, None, pp, pv, psh, pcube, phits, ptmin, pmo) == QA_EINVAL
        bare = hip.Context(0)
        try:
            assert device(bare._h, n, pp_, None, pp, pv, psh, pcube, phits, ptmin, pmo) == QA_ENOSCENE
            assert L.qa_probevis_sh(bare._h, n, hp, None, pp, pv, hsh.ctypes.data, None, None, None, hmo.ctypes.data) == QA_ENOSCENE
        finally:
            bare.close()
        # the moments' own rules: d outside 1 .. m, m % d != 0, dmax of 0, negative, NaN and inf, a normal_bias that is not finite,
        # NULL visibility params, a NULL moments array
        for field, bad in (("d", 0), ("d", -1), ("d", m + 1), ("d", 3), ("d", 8), ("dmax", 0.0), ("dmax", -1.0), ("dmax", np.nan), ("dmax", np.inf),
                           ("normal_bias", np.nan), ("normal_bias", np.inf)):
            v = hip.ProbeVisParams.of(d, DMAX)
            setattr(v, field, bad)
            assert device(c._h, n, pp_, None, pp, C.byref(v), psh, pcube, phits, ptmin, pmo) == QA_EINVAL, (field, bad)
            assert hostcall(n, hp, pp, C.byref(v), hmo.ctypes.data) == QA_EINVAL, (field, bad)
        assert device(c._h, n, pp_, None, pp, C.byref(hip.ProbeVisParams.default()), psh, pcube, phits, ptmin, pmo) == QA_EINVAL   # (dmax 0 as it comes)
        assert device(c._h, n, pp_, None, pp, None, psh, pcube, phits, ptmin, pmo) == QA_EINVAL
        assert device(c._h, n, pp_, None, pp, pv, psh, pcube, phits, ptmin, None) == QA_EINVAL
        assert hostcall(n, hp, pp, None, hmo.ctypes.data) == QA_EINVAL and hostcall(n, hp, pp, pv, None) == QA_EINVAL
        # the shading call
        nr = dev(np.float32([[0, 0, 1]] * n))
        out = torch.full((n, 3), 7.0, device="cuda:0")
        pn, po = nr.data_ptr(), out.data_ptr()
        one, cn = np.ones(3, np.float32), np.int32([n, 1, 1])
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        grid = lambda n_, sh_, mo_, d_, o_, s_, c_, p_, nr_, v_, out_: L.qa_probevis_grid_shade_device(c._h, n_, sh_, mo_, d_, ptr(o_), ptr(s_), ptr(c_), p_, nr_, v_, out_, None)   # noqa: E731
        ok = (n, psh, pmo, d, one, one, cn, pp_, pn, pv, po)
        for at, bad in ((0, 1 << 31), (1, None), (2, None), (3, 0), (3, 129), (4, None), (5, None), (5, np.float32([1, 0, 1])), (5, np.float32([1, np.nan, 1])),
                        (6, None), (6, np.int32([n, 0, 1])), (7, None), (8, None), (9, None), (10, None)):
            args = list(ok)
            args[at] = bad
            assert grid(*args) == QA_EINVAL, (at, bad)
        v = hip.ProbeVisParams.of(d, DMAX, np.nan)
        assert grid(*ok[:9], C.byref(v), po) == QA_EINVAL
        assert grid(0, None, None, d, one, one, cn, None, None, pv, None) == 0
        c.synchronize()
        torch.cuda.synchronize()
        # a refusal writes nothing
        assert (sh == 7.0).all() and (cube == 7.0).all() and (hits == 7).all() and (tmin == 7.0).all() and (mo == 7.0).all() and (out == 7.0).all()
        assert (hsh == 7).all() and (hmo == 7).all()
        # Python: raised before the library is reached
        with pytest.raises(ValueError):
            c.probevis_sh_device(tp, 3, DMAX, m=4)                       # d does not divide m
        with pytest.raises(ValueError):
            c.probevis_sh_device(tp, 2, None, m=4)                       # no dmax
        with pytest.raises(ValueError):
            c.probevis_sh_device(tp, 2, DMAX, m=4, moments=torch.empty((n, 6, 2, 2, 3), device="cuda:0"))
        with pytest.raises(TypeError):
            c.probevis_sh_device(tp, 2, DMAX, m=4, moments=torch.empty((n, 6, 2, 2, 2), dtype=torch.float64, device="cuda:0"))
        with pytest.raises(ValueError):
            c.probevis_sh(P, 5, DMAX, m=4)
        with pytest.raises(hip.HipError) as e:
            c.probevis_sh_device(tp, 2, 0.0, m=4)                        # dmax 0 reaches the library, which refuses it
        assert e.value.code == QA_EINVAL
        plain = hip.ProbeGrid(c, (0, 0, 0), (1, 1, 1), (2, 1, 1)).bake(m=2)
        with pytest.raises(ValueError):
            plain.shade_device(tp, nr, visibility=True)                   # baked without moments
        assert plain.moments is None
    finally:
        c.close()


@pytest.fixture(scope="module")
def baked():
    """A 2 x 1 x 3 grid inside the lit box, baked at m = 2 with d = 1 and d = 2, and without moments -> (context, {d: grid}, plain grid)"""
    from qaray_amd import hip
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        lo, hi = P[1:].min(axis=0), P[1:].max(axis=0)
        spacing = np.maximum((hi - lo) / np.float32([1, 1, 2]), 0.25)
        grids = {d: hip.ProbeGrid(c, lo, spacing, (2, 1, 3)).bake(visibility=True, d=d, m=2, spp=4, seed=SEEDS[0]) for d in (1, 2)}
        plain = hip.ProbeGrid(c, lo, spacing, (2, 1, 3)).bake(m=2, spp=4, seed=SEEDS[0])
        c.synchronize()
        sp = grids[1].spacing
        want = np.float32(1.5) * np.sqrt(np.float32(np.float32(sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]))
        for d, g in grids.items():
            assert g.moments.shape == (6, 6, d, d, 2) and g.dmax == want and (g.moments > 0).all() and (g.moments[..., 0] <= g.dmax).all()
            assert np.array_equal(bits(g.sh.cpu().numpy()), bits(plain.sh.cpu().numpy())) and (g.sh != 0).any()
        yield c, grids, plain
    finally:
        c.close()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_visibility_shading_is_the_host_form(n, baked):
    """ProbeGrid.shade_device(visibility=True) and qa_probevis_grid_shade_device equal probevis_grid_shade_host bit for bit: points
    inside the grid, outside it on every side, on the probes, and points and normals that are not finite; normal_bias 0 and 0.1.
    Without the flag a grid baked with moments shades with the bits of one baked without."""
    import torch
    from qaray_amd import hip
    c, grids, plain = baked
    grid = grids[1]
    rng = np.random.default_rng(200 + n)
    span = grid.spacing * (grid.counts - 1)
    p = rng.uniform(grid.origin - 0.5 * span - 1, grid.origin + 1.5 * span + 1, (n, 3)).astype(np.float32)
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    on = grid.points()
    p[: min(n, 6)] = on[: min(n, 6)]
    if n > 10:
        p[6], p[7], nr[8], nr[9] = (np.nan, 0, 0), (0, -np.inf, 0), (0, np.nan, 0), (np.inf, 0, 0)
        p[10] = (1e30, -1e30, 1e30)
    tp, tn = dev(p), dev(nr)
    for d, g in grids.items():
        sh, mo = g.sh.cpu().numpy(), g.moments.cpu().numpy()
        for bias in (0.0, 0.1):
            want = hip.probevis_grid_shade_host(sh, mo, g.origin, g.spacing, g.counts, p, nr, bias)
            got = g.shade_device(tp, tn, visibility=True, normal_bias=bias)
            out = torch.full((n, 3), 7.0, device="cuda:0")
            par = hip.ProbeVisParams.of(d, float(g.dmax), bias)
            assert hip.lib().qa_probevis_grid_shade_device(c._h, n, g.sh.data_ptr(), g.moments.data_ptr(), d, g.origin.ctypes.data, g.spacing.ctypes.data,
                                                           g.counts.ctypes.data, tp.data_ptr(), tn.data_ptr(), C.byref(par), out.data_ptr(), None) == 0
            c.synchronize()
            got, out = got.cpu().numpy(), out.cpu().numpy()
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(out), bits(want)), (n, d, bias)
            assert (got > 0).any() or n == 1
            if n > 10:
                assert not got[6:10].any()
        old = g.shade_device(tp, tn)
        ref = plain.shade_device(tp, tn)
        c.synchronize()
        assert np.array_equal(bits(old.cpu().numpy()), bits(ref.cpu().numpy()))
        assert np.array_equal(bits(old.cpu().numpy()), bits(hip.probe_grid_shade_host(sh, g.origin, g.spacing, g.counts, p, nr)))


def test_the_wall_between_two_rooms_stops_the_light(capsys):
    """tests/golden/probevis/two_rooms.xml: room A with an emitting ball, room B with nothing, a wall of 0.1 between them, no other
    light.  The grid of the CPU test (4 x 2 x 2, two columns of probes in each room) baked at m = 16, d = 8, 4 spp.  Over the 300
    points in B beside the wall the summed visibility result is below the summed trilinear result; only sums are compared: between
    lit probes of different brightness the reweighting may raise a single point.  The ratio of the sums is printed."""
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    fixture = os.path.join(GOLDEN, "probevis")
    c = fresh(load_scene_blob(os.path.join(fixture, "two_rooms.xml"), size=(32, 24), asset_root=fixture))
    try:
        o, s, cn = ROOMS_GRID
        grid = hip.ProbeGrid(c, o, s, cn).bake(visibility=True, d=ROOMS_D, m=ROOMS_M, spp=4)
        c.synchronize()
        K = 6 * ROOMS_M * ROOMS_M
        sh, hits, tmin = grid.sh.cpu().numpy(), grid.hits.cpu().numpy(), grid.tmin.cpu().numpy()
        in_a = grid.points()[:, 0] < 2.05
        # the preconditions
        assert in_a.sum() == 8 and (hits == K).all(), "the rooms are closed"
        assert (tmin > 0.3).all(), "no probe sits against a wall"
        assert not bits(sh[~in_a]).any(), "no light in B"
        assert (sh[in_a, 0, :] > 0).all(), "light at every probe of A"
        assert grid.dmax == np.float32(1.5) * np.sqrt(np.float32(3))
        p, nr = rooms_points()
        vis = grid.shade_device(dev(p), dev(nr), visibility=True)
        tri = grid.shade_device(dev(p), dev(nr))
        c.synchronize()
        vis, tri = vis.cpu().numpy().astype(np.float64), tri.cpu().numpy().astype(np.float64)
        with capsys.disabled():
            print(f"\ntwo rooms on the device: visibility {vis.sum():.6g}, trilinear {tri.sum():.6g}, ratio of the sums {vis.sum() / tri.sum():.4f}")
        assert tri.sum() > 0 and vis.sum() < tri.sum()
    finally:
        c.close()
