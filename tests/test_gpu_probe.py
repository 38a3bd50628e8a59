"""Light probes (qa_lightprobe.hip: qa_probe_sh*, qa_probe_shade_device, qa_probe_grid_shade_device; the opening comment of
qa_lightprobe_dev.h is the specification).  The anchor: probe_sh_device is, bit for bit, the composition written out here - the
directions of the host hook, radiance_rays_device on those rays with the streams (S * K + k) mod 2^32 and miss_environment, and the
numpy projection of tests/probe_util.py - which ties the call to qa_radiance_rays, and through its own anchor to every frame test
there is.  The rest checks what the specification says of probes: independence of batch, order and chunking, void probes, state and
refusals, and the two shading kernels against their host forms.

Radiance and probe calls only: no frame of an area-light scene is rendered here."""
import ctypes as C

import numpy as np
import pytest

from gbuffer_util import REGION, SEEDS, bits, scene_blob
from probe_util import MISS, project_ref
from radiance_util import QA_EINVAL, QA_ENOSCENE, QA_EUNSUPPORTED, SOFTSHADOW, anchor_blob, variant
from ray_query_util import BOX, fresh

pytestmark = pytest.mark.gpu

# scene -> (RES, LIGHTS, TEX, AREA) where tests/test_gpu_irradiance.py's table knows it: the LDS-resident and the global-memory
# scenes, with and without lights and textures; custom_textures.xml on top (whatever instance it runs)
ANCHOR = {
    BOX: (1, 0, 0, 0),
    "example_project11_box.xml": (0, 1, 0, 0),       # (meshes in global memory)
    "example_project7_checkboard.xml": (0, 1, 1, 0),
    "example_project3_sphere.xml": (1, 1, 0, 0),
    "custom_textures.xml": None,
}
LIT_BOX = "example_project3_box.xml"
IDS = np.uint32([0, 1, 77, 0xFFFFFFFF, 123456789])


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def probe_points(c, extra=4):
    """The camera position and the midpoints o + 0.5 t d of `extra` camera rays that hit, spread over the region -> float32 (1 + extra, 3)"""
    o, d = c.camera_rays(REGION, SEEDS[0])
    cast = c.cast_rays(o, d)
    hit = np.flatnonzero(cast["t"] < MISS)
    assert len(hit) >= extra
    pick = hit[np.linspace(0, len(hit) - 1, extra).astype(int)]
    mid = (o[pick] + (np.float32(0.5) * cast["t"][pick])[:, None] * d[pick]).astype(np.float32)
    return np.concatenate([o[:1], mid]).astype(np.float32)


def composed(c, P, S, m, spp, max_bounce, seed, jitter, photon_maps=False):
    """The composition the fused call must equal -> dict sh (n, 9, 3), cube (n, 6, m, m, 3), hits (n,), tmin (n,)"""
    from qaray_amd import hip
    n, K = len(P), 6 * m * m
    S = np.arange(n, dtype=np.uint32) if S is None else np.asarray(S, np.uint32)
    d, w, _ = hip.probe_directions_host(m, S, seed, jitter)
    sid = ((S.astype(np.uint64)[:, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    o = np.ascontiguousarray(np.broadcast_to(P[:, None, :], (n, K, 3)), np.float32)
    rgb, t, ns = c.radiance_rays_device(dev(o.reshape(-1, 3)), dev(d.reshape(-1, 3)), spp, max_bounce, seed, stream_ids=dev(sid.reshape(-1)),
                                        miss_environment=True, photon_maps=photon_maps)
    c.synchronize()
    rgb, t = rgb.cpu().numpy().reshape(n, K, 3), t.cpu().numpy().reshape(n, K)
    assert (ns.cpu().numpy() == spp).all()
    out = {"sh": np.zeros((n, 9, 3), np.float32), "cube": rgb.reshape(n, 6, m, m, 3), "hits": np.zeros(n, np.uint32), "tmin": np.zeros(n, np.float32)}
    for q in range(n):
        out["sh"][q], out["hits"][q], out["tmin"][q] = project_ref(d[q], w[q], rgb[q], t[q])
    return out


def fused(c, P, S, m, spp, max_bounce, seed, jitter, cube=True, **kw):
    got = c.probe_sh_device(dev(P), m, spp, max_bounce, seed, jitter, stream_ids=None if S is None else dev(np.asarray(S, np.uint32)), cube=cube or None, **kw)
    c.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "hits" else v.cpu().numpy()) for k, v in got.items()}


def differing(a, b):
    return [k for k in a if k in b and not (a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])))]


@pytest.mark.parametrize("scene", list(ANCHOR))
def test_a_probe_is_the_radiance_of_its_rays_projected(scene):
    """The anchor, bit for bit in sh, cube, hits and tmin: five probes (the camera position and the midpoints of four camera rays
    that hit), m = 1, 3, 4, 5 (6, 54, 96, 150 rays: below, across and above a wave), spp 1 and 3, max_bounce 0 and 5, centres and
    jitter; the probes' own indices as stream ids at spp 1, explicit ids at both ends of 32 bits at spp 3."""
    c = fresh(anchor_blob(scene))
    try:
        if ANCHOR[scene] is not None:
            assert variant(c.kernel_name()) == ANCHOR[scene], scene
        P = probe_points(c)
        lit = seen = False
        for m in (1, 3, 4, 5):
            for spp, seed, S in ((1, SEEDS[0], None), (3, SEEDS[1], IDS)):
                for max_bounce in (0, 5):
                    for jitter in (False, True):
                        want = composed(c, P, S, m, spp, max_bounce, seed, jitter)
                        got = fused(c, P, S, m, spp, max_bounce, seed, jitter)
                        assert not differing(got, want), (scene, m, spp, max_bounce, jitter, differing(got, want))
                        lit = lit or bool((got["sh"] != 0).any())
                        seen = seen or bool((got["hits"] > 0).any() and (got["tmin"] < MISS).any())
        assert lit and seen, "some light arrives and something is hit"
    finally:
        c.close()


def test_the_anchor_covers_both_residencies_lights_and_textures():
    known = [v for v in ANCHOR.values() if v is not None]
    assert len(ANCHOR) >= 4 and all(v[3] == 0 for v in known)
    for axis in range(3):
        assert {v[axis] for v in known} == {0, 1}


def test_a_probes_answer_does_not_depend_on_chunks_batch_or_order():
    """chunk_rays = 1, 100 and 0 (and 200: two probes per chunk and a last chunk of one) give equal bits for n = 5 at m = 4; batches
    of 1, 2 and 5 give per-probe results equal to the largest batch's, and a permutation with its stream ids the permuted results;
    the host form equals the device form; each argument matters."""
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        kw = dict(m=4, spp=2, max_bounce=3, seed=SEEDS[1], jitter=True)
        whole = fused(c, P, IDS, **kw)
        assert (whole["sh"] != 0).any() and len(np.unique(whole["sh"].reshape(5, -1), axis=0)) == 5
        for chunk_rays in (1, 100, 200, 0):
            assert not differing(fused(c, P, IDS, chunk_rays=chunk_rays, **kw), whole), chunk_rays
        for n in (1, 2, 5):
            part = fused(c, P[:n], IDS[:n], **kw)
            assert not differing(part, {k: v[:n] for k, v in whole.items()}), n
        perm = np.random.default_rng(5).permutation(5)
        shuffled = fused(c, P[perm], IDS[perm], chunk_rays=200, **kw)
        assert not differing(shuffled, {k: v[perm] for k, v in whole.items()})
        # without a cube the rays pass through the scratch: the same sh, hits and tmin
        assert not differing(fused(c, P, IDS, cube=False, chunk_rays=100, **kw), whole)
        host = c.probe_sh(P, stream_ids=IDS, cube=True, **kw)
        assert not differing(host, whole)
        assert not differing(c.probe_sh(P, stream_ids=IDS, chunk_rays=100, **kw), whole)
        # without stream ids a probe's stream is its index
        assert not differing(fused(c, P, None, **kw), fused(c, P, np.arange(5), **kw))
        for change in (dict(seed=SEEDS[0]), dict(spp=3), dict(max_bounce=0), dict(jitter=False), dict(m=3)):
            other = fused(c, P, IDS, **{**kw, **change})
            assert other["sh"].shape != whole["sh"].shape or not np.array_equal(bits(other["sh"]), bits(whole["sh"])), change
        assert not np.array_equal(bits(fused(c, P, IDS[::-1].copy(), **kw)["sh"]), bits(whole["sh"]))
    finally:
        c.close()


def test_void_probes_are_zero_and_disturb_nothing():
    """NaN, +inf and -inf in each component of the point, spread among good probes: sh and cube +0, hits 0, tmin the miss value; the
    good probes keep their bits, with and without a cube, in chunks of one probe and in one chunk."""
    c = fresh(scene_blob(LIT_BOX))
    try:
        good = probe_points(c, 9)
        void = np.repeat(good[:1], 9, axis=0)
        for i, bad in enumerate((np.nan, np.inf, -np.inf)):
            for k in range(3):
                void[3 * i + k, k] = bad
        at = np.arange(9)
        P = np.insert(good, at, void, axis=0)
        isvoid = ~np.isfinite(P).all(axis=1)
        assert isvoid.sum() == 9 and len(P) == 19
        ids = np.zeros(len(P), np.uint32)
        ids[~isvoid] = 100 + np.arange(len(good))
        ids[isvoid] = 7
        kw = dict(m=3, spp=2, max_bounce=2, seed=SEEDS[0], jitter=True)
        alone = fused(c, good, ids[~isvoid], **kw)
        assert (alone["sh"] != 0).any()
        for chunk_rays, cube in ((0, True), (1, True), (0, False), (120, False)):
            got = fused(c, P, ids, chunk_rays=chunk_rays, cube=cube, **kw)
            assert not bits(got["sh"][isvoid]).any() and not got["hits"][isvoid].any() and (got["tmin"][isvoid] == MISS).all()
            if cube:
                assert not bits(got["cube"][isvoid]).any()
            assert not differing({k: v[~isvoid] for k, v in got.items()}, alone), (chunk_rays, cube)
        assert not differing(fused(c, P, ids, **kw), composed(c, P, ids, **kw)), "and the composition says the same of them"
    finally:
        c.close()


def test_state_counters_and_refusals():
    """A frame has the same bits before and after a call; the counters move by n * K * spp samples and the kernel time by one launch
    per chunk; every refusal of the C ABI leaves the outputs alone; Python's argument errors are raised before the library is
    entered."""
    import torch
    from qaray_amd import hip
    L = hip.lib()
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        n, m, K = len(P), 3, 54
        frame0 = c.render_region(REGION, 2, seed=SEEDS[0])
        name = c.kernel_name()
        c.reset_counters()
        launches0 = c.kernel_time()[1]
        c.probe_sh(P, m=m, spp=3, max_bounce=0)
        cnt = c.counters()
        assert cnt["samples"] == n * K * 3 and 0 < cnt["casts_normal"] <= n * K * 3 and c.kernel_time()[1] == launches0 + 1 and c.kernel_name() == name
        c.reset_counters()
        c.probe_sh(P, m=m, spp=2, chunk_rays=2 * K)
        assert c.counters()["samples"] == n * K * 2 and c.kernel_time()[1] == launches0 + 1 + 3   # (chunks of 2, 2 and 1 probes)
        frame1 = c.render_region(REGION, 2, seed=SEEDS[0])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame0, frame1))

        tp = dev(P)
        sh = torch.full((n, 9, 3), 7.0, device="cuda:0")
        cube = torch.full((n, 6, m, m, 3), 7.0, device="cuda:0")
        hits = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
        tmin = torch.full((n,), 7.0, device="cuda:0")
        pp_, psh, pcube, phits, ptmin = (x.data_ptr() for x in (tp, sh, cube, hits, tmin))
        par = hip.ProbeParams.of(m=m)
        pp = C.byref(par)
        device = lambda h, n, *a: L.qa_probe_sh_device(h, n, *a, None)   # noqa: E731
        hsh = np.full((n, 9, 3), 7, np.float32)
        hp = P.ctypes.data
        # n == 0 launches nothing and needs no array
        assert device(c._h, 0, None, None, None, None, None, None, None) == 0
        assert L.qa_probe_sh(c._h, 0, None, None, None, None, None, None, None) == 0
        assert c.probe_sh(np.zeros((0, 3)))["sh"].shape == (0, 9, 3)
        refused = [
            (1 << 31, pp_, None, pp, psh, pcube, phits, ptmin),    # n beyond 2^31 - 1 (nothing is sized by it)
            (1 << 40, pp_, None, pp, psh, pcube, phits, ptmin),
            (n, None, None, pp, psh, pcube, phits, ptmin),         # a null point array
            (n, pp_, None, pp, None, pcube, phits, ptmin),         # a null sh
            (n, pp_, None, None, psh, pcube, phits, ptmin),        # null params
        ]
        for args in refused:
            assert device(c._h, *args) == QA_EINVAL, args
        # radiance's rules for spp and max_bounce; m outside 1 .. 128; every flag bit but QA_PROBE_JITTER and QA_RADIANCE_PHOTON_MAPS,
        # QA_RADIANCE_PER_SAMPLE and QA_RADIANCE_MISS_ENVIRONMENT (which is always set) among them
        for field, bad in (("spp", 0), ("spp", -3), ("max_bounce", -1), ("m", 0), ("m", -1), ("m", 129), ("flags", 1), ("flags", 2), ("flags", 4),
                           ("flags", 32), ("flags", 1 << 31), ("flags", 16 | 1)):
            q = hip.ProbeParams.of(m=m)
            setattr(q, field, bad)
            assert device(c._h, n, pp_, None, C.byref(q), psh, pcube, phits, ptmin) == QA_EINVAL, (field, bad)
            assert L.qa_probe_sh(c._h, n, hp, None, C.byref(q), hsh.ctypes.data, None, None, None) == QA_EINVAL, (field, bad)
        # a chunk is a batch of the radiance query: its limit on the rays applies to a chunk, whatever the batch holds
        big = hip.ProbeParams.of(m=128, chunk_rays=1 << 40)
        assert device(c._h, (1 << 31) - 1, pp_, None, C.byref(big), psh, pcube, phits, ptmin) == QA_EINVAL
        big = hip.ProbeParams.of(m=128, chunk_rays=(1 << 31) + 98304)
        assert device(c._h, (1 << 31) - 1, pp_, None, C.byref(big), psh, pcube, phits, ptmin) == QA_EINVAL
        assert L.qa_probe_sh(c._h, 1 << 31, hp, None, pp, hsh.ctypes.data, None, None, None) == QA_EINVAL
        assert L.qa_probe_sh(c._h, n, None, None, pp, hsh.ctypes.data, None, None, None) == QA_EINVAL
        assert L.qa_probe_sh(c._h, n, hp, None, pp, None, None, None, None) == QA_EINVAL
        assert device(None, n, pp_, None, pp, psh, pcube, phits, ptmin) == QA_EINVAL
        # flag without maps: the radiance query's code
        q = hip.ProbeParams.of(m=m, photon_maps=True)
        assert device(c._h, n, pp_, None, C.byref(q), psh, pcube, phits, ptmin) == QA_ENOSCENE
        bare = hip.Context(0)
        try:
            assert device(bare._h, n, pp_, None, pp, psh, pcube, phits, ptmin) == QA_ENOSCENE
            assert L.qa_probe_sh(bare._h, n, hp, None, pp, hsh.ctypes.data, None, None, None) == QA_ENOSCENE
        finally:
            bare.close()
        # the shading calls
        nr = dev(np.float32([[0, 0, 1]] * n))
        idx = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        out = torch.full((n, 3), 7.0, device="cuda:0")
        pn, pi, po = nr.data_ptr(), idx.data_ptr(), out.data_ptr()
        shade = lambda *a: L.qa_probe_shade_device(c._h, *a, None)   # noqa: E731
        for args in ((1 << 31, psh, n, pn, None, po), (n, None, n, pn, None, po), (n, psh, n, None, None, po), (n, psh, n, pn, None, None),
                     (n, psh, 0, pn, pi, po), (n, psh, 1 << 31, pn, pi, po), (n, psh, n - 1, pn, None, po)):
            assert shade(*args) == QA_EINVAL, args
        one, cn = np.ones(3, np.float32), np.int32([n, 1, 1])
        grid = lambda *a: L.qa_probe_grid_shade_device(c._h, *a, None)   # noqa: E731
        for o_, s_, c_ in ((None, one, cn), (one, None, cn), (one, one, None), (one, np.float32([1, 0, 1]), cn), (one, np.float32([1, -1, 1]), cn),
                           (one, np.float32([1, np.nan, 1]), cn), (np.float32([np.inf, 0, 0]), one, cn), (one, one, np.int32([n, 0, 1])),
                           (one, one, np.int32([1 << 16, 1 << 16, 1]))):
            ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
            assert grid(n, psh, ptr(o_), ptr(s_), ptr(c_), pp_, pn, po) == QA_EINVAL, (o_, s_, c_)
        for args in ((n, None, pp_, pn, po), (n, psh, None, pn, po), (n, psh, pp_, None, po), (n, psh, pp_, pn, None), (1 << 31, psh, pp_, pn, po)):
            assert grid(args[0], args[1], one.ctypes.data, one.ctypes.data, cn.ctypes.data, *args[2:]) == QA_EINVAL, args
        assert shade(0, None, 0, None, None, None) == 0 and grid(0, None, one.ctypes.data, one.ctypes.data, cn.ctypes.data, None, None, None) == 0
        c.synchronize()
        torch.cuda.synchronize()
        # a refusal writes nothing
        assert (sh == 7.0).all() and (cube == 7.0).all() and (hits == 7).all() and (tmin == 7.0).all() and (hsh == 7).all() and (out == 7.0).all()
        # optional outputs: sh alone
        assert device(c._h, n, pp_, None, pp, psh, None, None, None) == 0
        c.synchronize()
        want = c.probe_sh(P, m=m)
        assert np.array_equal(bits(sh.cpu().numpy()), bits(want["sh"])) and (cube == 7.0).all() and (hits == 7).all() and (tmin == 7.0).all()
        # on a stream of the caller's, into tensors of the caller's
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            sp = dev(P)
            got = c.probe_sh_device(sp, m=m, sh=sh, cube=cube, hits=hits, tmin=tmin, stream=s.cuda_stream)
        s.synchronize()
        assert got["sh"] is sh and got["cube"] is cube and got["hits"] is hits and got["tmin"] is tmin
        assert np.array_equal(bits(sh.cpu().numpy()), bits(want["sh"])) and np.array_equal(hits.cpu().numpy().view(np.uint32), want["hits"])
        assert np.array_equal(bits(tmin.cpu().numpy()), bits(want["tmin"]))

        # Python: raised before the library is reached
        with pytest.raises(TypeError):
            c.probe_sh_device(P)                                            # numpy where a tensor is expected
        with pytest.raises(TypeError):
            c.probe_sh_device(tp.double())                                  # dtype
        with pytest.raises(TypeError):
            c.probe_sh_device(tp, hits=torch.empty(n, device="cuda:0"))
        with pytest.raises(TypeError):
            c.probe_sh_device(tp, stream_ids=torch.zeros(n, device="cuda:0"))
        with pytest.raises(ValueError):
            c.probe_sh_device(tp.cpu())                                     # device
        with pytest.raises(ValueError):
            c.probe_sh_device(tp, m=0)
        with pytest.raises(ValueError):
            c.probe_sh_device(tp, m=m, cube=torch.empty((n, 6, m, m + 1, 3), device="cuda:0"))   # shape
        with pytest.raises(ValueError):
            c.probe_sh_device(torch.empty((n, 6), device="cuda:0")[:, :3])  # contiguity
        with pytest.raises(ValueError):
            c.probe_sh(P, stream_ids=np.arange(n + 1))
        with pytest.raises(ValueError):
            c.probe_shade_device(sh[:2], nr)                                # fewer probes than points and no index
        with pytest.raises(TypeError):
            c.probe_shade_device(sh, nr, index=idx.long())
        with pytest.raises(ValueError):
            hip.ProbeGrid(c, (0, 0, 0), (1, 1, 1), (2, 1, 3)).shade_device(tp, nr)   # not baked
    finally:
        c.close()


def test_long_area_light_paths_are_refused():
    """Area lights with max_bounce > 7 are refused as the radiance query refuses them, and nothing is written; max_bounce 7 runs."""
    import torch
    from qaray_amd import hip
    c = fresh(anchor_blob(SOFTSHADOW))
    try:
        assert variant(c.kernel_name())[3] == 1
        P = probe_points(c)
        sh = torch.full((len(P), 9, 3), 7.0, device="cuda:0")
        with pytest.raises(hip.HipError) as e:
            c.probe_sh_device(dev(P), m=2, max_bounce=8, sh=sh)
        assert e.value.code == QA_EUNSUPPORTED
        c.synchronize()
        assert (sh == 7.0).all()
        assert (c.probe_sh(P, m=2, max_bounce=7)["sh"] != 0).any()
    finally:
        c.close()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_shading_is_the_host_form(n, baked):
    """probe_shade_device, with and without an index (clamped at both ends), equals probe_shade_host bit for bit"""
    from qaray_amd import hip
    c, grid, sh = baked
    rng = np.random.default_rng(n)
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    nr[0] = (0, 0, 1)
    if n > 3:
        nr[1], nr[2], nr[3] = (np.nan, 0, 0), (0, np.inf, 0), (0, 0, 0)
    idx = rng.integers(-2, len(sh) + 2, n).astype(np.int32)
    got = c.probe_shade_device(grid.sh, dev(nr), index=dev(idx))
    c.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(hip.probe_shade_host(sh, nr, idx)))
    many = np.ascontiguousarray(np.resize(sh, (n, 9, 3)))
    got = c.probe_shade_device(dev(many), dev(nr))
    c.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(hip.probe_shade_host(many, nr))) and (got > 0).any()


@pytest.fixture(scope="module")
def baked():
    """A 2 x 1 x 3 grid inside the lit box, baked at m = 2 -> (context, grid, its coefficients on the host)"""
    from qaray_amd import hip
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        lo, hi = P[1:].min(axis=0), P[1:].max(axis=0)
        grid = hip.ProbeGrid(c, lo, np.maximum((hi - lo) / np.float32([1, 1, 2]), 0.25), (2, 1, 3)).bake(m=2, spp=4, seed=SEEDS[0])
        c.synchronize()
        sh = grid.sh.cpu().numpy()
        assert sh.shape == (6, 9, 3) and (sh != 0).any()
        want = c.probe_sh(grid.points(), m=2, spp=4, seed=SEEDS[0])
        assert np.array_equal(bits(sh), bits(want["sh"])) and np.array_equal(grid.hits.cpu().numpy().view(np.uint32), want["hits"])
        assert np.array_equal(bits(grid.tmin.cpu().numpy()), bits(want["tmin"]))
        yield c, grid, sh
    finally:
        c.close()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_grid_shading_is_the_host_form(n, baked):
    """ProbeGrid.shade_device equals probe_grid_shade_host bit for bit: points inside the grid, outside it on every side, on the
    probes, and points and normals that are not finite"""
    from qaray_amd import hip
    c, grid, sh = baked
    rng = np.random.default_rng(100 + n)
    span = grid.spacing * (grid.counts - 1)
    p = rng.uniform(grid.origin - 0.5 * span - 1, grid.origin + 1.5 * span + 1, (n, 3)).astype(np.float32)
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    on = grid.points()
    p[: min(n, 6)] = on[: min(n, 6)]
    if n > 10:
        p[6], p[7], nr[8], nr[9] = (np.nan, 0, 0), (0, -np.inf, 0), (0, np.nan, 0), (np.inf, 0, 0)
        p[10] = (1e30, -1e30, 1e30)
    got = grid.shade_device(dev(p), dev(nr))
    c.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(hip.probe_grid_shade_host(sh, grid.origin, grid.spacing, grid.counts, p, nr)))
    assert (got > 0).any() or n == 1
    if n > 10:
        assert not got[6:10].any()


def test_probes_gather_from_photon_maps_when_asked():
    """custom_photon.xml with its maps built: photon_maps=True equals the composition with photon_maps=True on the radiance call, bit
    for bit; without the flag the call is refused while the maps are built (QA_EUNSUPPORTED), and with it once they are cleared
    (QA_ENOSCENE); both refusals write nothing."""
    import torch
    from qaray_amd import hip
    c = fresh(scene_blob("custom_photon.xml"))
    try:
        P = probe_points(c)
        plain = fused(c, P, IDS, 3, 2, 5, SEEDS[0], False)
        c.build_photon_maps((3000, 20, 0.2), (400, 20, 1.0))
        for m, spp, jitter in ((3, 2, False), (4, 1, True)):
            want = composed(c, P, IDS, m, spp, 5, SEEDS[0], jitter, photon_maps=True)
            got = fused(c, P, IDS, m, spp, 5, SEEDS[0], jitter, photon_maps=True, chunk_rays=2 * 6 * m * m)
            assert not differing(got, want), (m, spp, jitter, differing(got, want))
            if m == 3:
                assert not np.array_equal(bits(got["sh"]), bits(plain["sh"])), "the maps change what a probe sees"
        sh = torch.full((len(P), 9, 3), 7.0, device="cuda:0")
        with pytest.raises(hip.HipError) as e:
            c.probe_sh_device(dev(P), m=3, sh=sh)
        assert e.value.code == QA_EUNSUPPORTED
        c.clear_photon_maps()
        with pytest.raises(hip.HipError) as e:
            c.probe_sh_device(dev(P), m=3, sh=sh, photon_maps=True)
        assert e.value.code == QA_ENOSCENE
        c.synchronize()
        assert (sh == 7.0).all()
        assert not differing(fused(c, P, IDS, 3, 2, 5, SEEDS[0], False), plain)
    finally:
        c.close()
