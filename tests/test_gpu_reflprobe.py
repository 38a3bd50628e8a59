"""Reflection probes on the device (qa_reflprobe.hip: qa_reflprobe_prefilter_device, qa_reflprobe_shade_device,
qa_reflprobe_grid_shade_device; the opening comment of qa_reflprobe_dev.h is the specification).  The prefilter against the float32
numpy restatement of tests/reflprobe_util.py, bit for bit, on cubes built with torch and on the cubes probe_sh_device traces; the two
lookups against their host forms; ProbeGrid.bake(reflections=True) against the composition by hand; every refusal; and a lamp seen
from a probe of tests/golden/probevis/two_rooms.xml."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gbuffer_util import SEEDS, bits, scene_blob
from probe_util import directions_ref
from radiance_util import QA_EINVAL, anchor_blob
from ray_query_util import BOX, fresh
from reflprobe_util import layout_ref, prefilter_ref
from test_gpu_probe import LIT_BOX, dev, probe_points

pytestmark = pytest.mark.gpu

# Stream order (tests/test_reflprobe_stream_closure.py): no entry of this family orders anything, so no case runs two streams
CASES = {}
EXEMPT = {
    "qa_reflprobe_prefilter_device": "reads d_cube and writes d_chain, both the caller's: no buffer of the context's is touched, nothing is ordered or recorded",
    "qa_reflprobe_shade_device": "reads the caller's chain, directions and levels and writes the caller's rgb: as qa_probe_shade_device, nothing to order",
    "qa_reflprobe_grid_shade_device": "reads the caller's chain, points, directions and levels and writes the caller's rgb: as qa_probe_grid_shade_device",
}


@pytest.fixture(scope="module")
def bare():
    """A context without a scene: none of the three calls needs one"""
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def torch_cube(n, m, seed, special=True):
    """A cube built on the device: uniform in [0, 4), and with NaN, inf, -0 and a denormal among probe 0's texels"""
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    cube = torch.rand((n, 6, m, m, 3), generator=g, device="cuda:0") * 4
    if special:
        flat = cube[0].view(-1)
        vals = torch.tensor([float("nan"), float("inf"), -0.0, 1e-42, 0.0], device="cuda:0")
        flat[torch.arange(len(vals), device="cuda:0") * 7 % flat.numel()] = vals
    return cube


def prefiltered(c, cube, L):
    chain = c.reflprobe_prefilter_device(cube, L)
    c.synchronize()
    return chain.cpu().numpy()


@pytest.mark.parametrize("m,levels", [(2, (1, 2)), (4, (1, 2, 3)), (8, (1, 2, 3, 4)), (16, (5,)), (32, (3,))])
def test_the_prefilter_is_the_restatement(bare, m, levels):
    """m = 2, 4, 8 with every L and (16, 5): one staged piece, several probes per workgroup below m = 16.  (32, 3): 6144 source
    records in four pieces of 1536 and 1920 filtered texels in four runs of 512.  Three probes, the first with texels that are not
    finite."""
    for L in levels:
        cube = torch_cube(3, m, 100 * m + L)
        got = prefiltered(bare, cube, L)
        want = prefilter_ref(cube.cpu().numpy(), L)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (m, L, np.flatnonzero((bits(got) != bits(want)).any(axis=(0, 2)))[:8])
        assert np.isfinite(got[1:]).all() and (got[1:] > 0).all() and not np.isfinite(got[0]).all()


@pytest.mark.parametrize("m", [4, 8])
def test_a_probes_chain_does_not_depend_on_the_batch(bare, m):
    """130 probes - eight (m = 4) or four (m = 8) share a workgroup, the last workgroup is partly filled - against the restatement,
    and batches of 1, 2 and 5 against the 130's first probes; into a chain that is given"""
    import torch
    cube = torch_cube(130, m, m)
    whole = prefiltered(bare, cube, None)
    assert np.array_equal(bits(whole), bits(prefilter_ref(cube.cpu().numpy())))
    for n in (1, 2, 5):
        assert np.array_equal(bits(prefiltered(bare, cube[:n].contiguous(), None)), bits(whole[:n])), n
    given = torch.full((5, whole.shape[1], 3), 7.0, device="cuda:0")
    assert bare.reflprobe_prefilter_device(cube[125:].contiguous(), chain=given) is given
    bare.synchronize()
    assert np.array_equal(bits(given.cpu().numpy()), bits(whole[125:]))


@pytest.mark.parametrize("scene", [BOX, "custom_textures.xml"])
def test_the_chain_of_a_traced_cube(scene):
    """probe_sh_device(cube=True) -> reflprobe_prefilter_device on one stream: level 0 is the cube bit for bit, the rest the
    restatement of the downloaded cube; a void probe among the five good ones stays zero"""
    c = fresh(anchor_blob(scene))
    try:
        P = np.insert(probe_points(c), 2, [np.nan, 0, 0], axis=0).astype(np.float32)
        for m, spp, seed in ((4, 1, SEEDS[0]), (8, 3, SEEDS[1])):
            out = c.probe_sh_device(dev(P), m, spp, 5, seed, cube=True)
            chain = c.reflprobe_prefilter_device(out["cube"])
            c.synchronize()
            cube, chain = out["cube"].cpu().numpy(), chain.cpu().numpy()
            K = 6 * m * m
            assert np.array_equal(bits(chain[:, :K]), bits(cube.reshape(len(P), K, 3)))
            assert np.array_equal(bits(chain), bits(prefilter_ref(cube)))
            assert not bits(chain[2]).any() and (chain[[0, 1, 3, 4, 5], K:] > 0).any()
    finally:
        c.close()


@pytest.fixture(scope="module")
def baked():
    """A 2 x 1 x 3 grid inside the lit box baked at m = 4: plain, with reflections (all levels, and one level), and with reflections
    and visibility -> (context, dict of grids)"""
    from qaray_amd import hip
    c = fresh(scene_blob(LIT_BOX))
    try:
        P = probe_points(c)
        lo, hi = P[1:].min(axis=0), P[1:].max(axis=0)
        spacing = np.maximum((hi - lo) / np.float32([1, 1, 2]), 0.25)
        kw = dict(m=4, spp=4, seed=SEEDS[0])
        new = lambda: hip.ProbeGrid(c, lo, spacing, (2, 1, 3))   # noqa: E731
        grids = {"plain": new().bake(**kw), "refl": new().bake(reflections=True, **kw), "one": new().bake(reflections=True, levels=1, **kw),
                 "vis": new().bake(visibility=True, d=2, **kw), "both": new().bake(visibility=True, d=2, reflections=True, **kw)}
        c.synchronize()
        yield c, grids
    finally:
        c.close()


def test_bake_with_reflections_is_the_composition_by_hand(baked):
    """The chain is reflprobe_prefilter_device of the cube the same bake hands out, with and without visibility; sh, hits, tmin and
    the moments keep the plain bake's bits; without the flag nothing is kept"""
    import torch
    c, grids = baked
    pts = torch.from_numpy(grids["plain"].points()).to("cuda:0")
    out = c.probe_sh_device(pts, m=4, spp=4, seed=SEEDS[0], cube=True)
    by_hand = {L: c.reflprobe_prefilter_device(out["cube"], L) for L in (None, 1)}
    c.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    for name, L, levels in (("refl", None, 3), ("both", None, 3), ("one", 1, 1)):
        g = grids[name]
        assert (g.m, g.levels) == (4, levels) and g.chain.shape == (6, layout_ref(4, levels)[4], 3)
        assert np.array_equal(bits(host(g.chain)), bits(host(by_hand[L]))) and (host(g.chain) > 0).any(), name
        assert np.array_equal(bits(host(g.chain)), bits(prefilter_ref(host(out["cube"]), levels)))
    for name, plain in (("refl", "plain"), ("one", "plain"), ("both", "vis")):
        for field in ("sh", "hits", "tmin", "moments"):
            a, b = host(getattr(grids[name], field)), host(getattr(grids[plain], field))
            assert (a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, field)
    assert grids["both"].moments is not None and grids["plain"].chain is None and grids["vis"].chain is None and grids["vis"].m is None
    with pytest.raises(ValueError):
        grids["plain"].reflect_device(pts, pts, pts[:, 0].contiguous())
    from qaray_amd import hip
    with pytest.raises(ValueError):
        hip.ProbeGrid(c, (0, 0, 0), (1, 1, 1), (1, 1, 1)).bake(reflections=True, m=6)   # (refused before anything is traced)


def lookups(rng, grid, n):
    """Points in and around the grid and on its probes, random directions with axes, ties and void ones among them, levels at,
    between and outside the chain's"""
    span = grid.spacing * (grid.counts - 1)
    p = rng.uniform(grid.origin - 0.5 * span - 1, grid.origin + 1.5 * span + 1, (n, 3)).astype(np.float32)
    R = rng.standard_normal((n, 3)).astype(np.float32)
    lam = rng.uniform(-1, 4, n).astype(np.float32)
    on = grid.points()
    p[: min(n, 6)] = on[: min(n, 6)]
    if n > 20:
        R[:6] = np.float32([[1, 0, 0], [0, -1, 0], [1, 1, 0], [-1, 1, 1], [0, -2, 2], [1e-40, 0, 0]])
        p[6], p[7], R[8], R[9], R[10], lam[11] = (np.nan, 0, 0), (0, -np.inf, 0), (0, np.nan, 0), (np.inf, 0, 0), (0, 0, 0), np.nan
        p[12] = (1e30, -1e30, 1e30)
        lam[13:19] = (0, 1, 2, np.inf, -np.inf, 1.5)
    return p, R, lam


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_the_lookups_are_their_host_forms(n, baked):
    """Context.reflprobe_shade_device (with and without an index) and ProbeGrid.reflect_device equal reflprobe_shade_host and
    reflprobe_grid_shade_host bit for bit, at L = 1 and L = lg + 1 = 3"""
    from qaray_amd import hip
    c, grids = baked
    rng = np.random.default_rng(300 + n)
    for name in ("one", "refl"):
        g = grids[name]
        chain = g.chain.cpu().numpy()
        p, R, lam = lookups(rng, g, n)
        index = rng.integers(-2, 9, n).astype(np.int32)
        tp, tR, tl = dev(p), dev(R), dev(lam)
        got = c.reflprobe_shade_device(g.chain, 4, tR, tl, g.levels, index=dev(index))
        grid = g.reflect_device(tp, tR, tl)
        c.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(hip.reflprobe_shade_host(chain, 4, R, lam, g.levels, index))), (n, name)
        want = hip.reflprobe_grid_shade_host(chain, 4, g.origin, g.spacing, g.counts, p, R, lam, g.levels)
        assert np.array_equal(bits(grid.cpu().numpy()), bits(want)), (n, name)
        assert (want > 0).any() or n == 1
        if n > 20:
            assert not want[6:12].any()
        if n <= 6:   # (lookup i takes probe i)
            plain = c.reflprobe_shade_device(g.chain, 4, tR, tl, g.levels)
            c.synchronize()
            assert np.array_equal(bits(plain.cpu().numpy()), bits(hip.reflprobe_shade_host(chain, 4, R, lam, g.levels)))


def test_refusals_write_nothing(bare):
    import torch
    from qaray_amd import hip
    L = hip.lib()
    c = bare
    n, m, lv, T = 3, 4, 3, 126
    cube = torch.zeros((n, 6, m, m, 3), device="cuda:0")
    chain = torch.full((n, T, 3), 7.0, device="cuda:0")
    d = torch.ones((n, 3), device="cuda:0")
    lam = torch.zeros((n,), device="cuda:0")
    idx = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
    rgb = torch.full((n, 3), 7.0, device="cuda:0")
    pc, ph, pd, pl, pi, pr = (t.data_ptr() for t in (cube, chain, d, lam, idx, rgb))
    torch.cuda.synchronize()
    # the prefilter
    for args in ((1 << 31, pc, m, lv, ph), (n, None, m, lv, ph), (n, pc, m, lv, None), (n, pc, 0, 1, ph), (n, pc, 3, 1, ph), (n, pc, 6, 2, ph), (n, pc, 256, 1, ph),
                 (n, pc, m, 0, ph), (n, pc, m, 4, ph), (n, pc, m, -1, ph)):
        assert L.qa_reflprobe_prefilter_device(c._h, *args, None) == QA_EINVAL, args
    assert L.qa_reflprobe_prefilter_device(None, n, pc, m, lv, ph, None) == QA_EINVAL
    assert L.qa_reflprobe_prefilter_device(c._h, 0, None, 0, 0, None, None) == 0
    # the lookup
    ok = (n, ph, n, m, lv, pd, pl, pi, pr)
    for at, bad in ((0, 1 << 31), (1, None), (2, 0), (2, 1 << 31), (3, 5), (3, 0), (4, 0), (4, 4), (5, None), (6, None), (8, None)):
        args = list(ok)
        args[at] = bad
        assert L.qa_reflprobe_shade_device(c._h, *args, None) == QA_EINVAL, (at, bad)
    assert L.qa_reflprobe_shade_device(c._h, n, ph, n - 1, m, lv, pd, pl, None, pr, None) == QA_EINVAL   # fewer probes than lookups, no index
    assert L.qa_reflprobe_shade_device(None, *ok, None) == QA_EINVAL
    assert L.qa_reflprobe_shade_device(c._h, 0, None, 0, 0, 0, None, None, None, None, None) == 0
    # the grid lookup
    one, cn = np.ones(3, np.float32), np.int32([n, 1, 1])
    ptr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a   # noqa: E731
    grid = lambda *a: L.qa_reflprobe_grid_shade_device(c._h, *(ptr(x) for x in a), None)   # noqa: E731
    ok = (n, ph, m, lv, one, one, cn, pd, pd, pl, pr)
    for at, bad in ((0, 1 << 31), (1, None), (2, 12), (3, 0), (3, 4), (4, None), (4, np.float32([0, np.inf, 0])), (5, None), (5, np.float32([1, 0, 1])),
                    (5, np.float32([1, np.nan, 1])), (6, None), (6, np.int32([n, 0, 1])), (6, np.int32([1 << 16, 1 << 16, 1])), (7, None), (8, None), (9, None), (10, None)):
        args = list(ok)
        args[at] = bad
        assert grid(*args) == QA_EINVAL, (at, bad)
    assert grid(0, None, m, lv, one, one, cn, None, None, None, None) == 0
    c.synchronize()
    torch.cuda.synchronize()
    assert (chain == 7.0).all() and (rgb == 7.0).all()
    # Python: raised before the library is reached
    with pytest.raises(ValueError):
        c.reflprobe_prefilter_device(torch.zeros((1, 6, 6, 6, 3), device="cuda:0"))
    with pytest.raises(ValueError):
        c.reflprobe_prefilter_device(cube, 4)
    with pytest.raises(ValueError):
        c.reflprobe_prefilter_device(cube, chain=chain[:, :100].contiguous())
    with pytest.raises(TypeError):
        c.reflprobe_prefilter_device(cube.double())
    with pytest.raises(ValueError):
        c.reflprobe_shade_device(chain, 4, d, lam, 2)            # the chain of three levels is not one of two
    with pytest.raises(ValueError):
        c.reflprobe_shade_device(chain[:2].contiguous(), 4, d, lam)   # fewer probes than lookups
    with pytest.raises(TypeError):
        c.reflprobe_shade_device(chain, 4, d, lam.double())


def test_a_lamp_is_sharp_at_the_mirror_level_and_blurred_at_the_last():
    """tests/golden/probevis/two_rooms.xml, the probe at (0.5, 0.5, 0.5) of the lit room, the emitting ball of radius 0.15 at
    (1, 1, 1.7): the cube's brightest texel lies towards the ball (the precondition); the level-0 lookup towards the ball is greater
    than the one in the opposite direction, and at the 1 x 1 level the two differ by less than at level 0"""
    from qaray_amd.host import load_scene_blob
    fixture = os.path.join(GOLDEN, "probevis")
    c = fresh(load_scene_blob(os.path.join(fixture, "two_rooms.xml"), size=(32, 24), asset_root=fixture))
    try:
        P = np.float32([[0.5, 0.5, 0.5]])
        to = np.float32([1, 1, 1.7]) - P[0]
        to /= np.linalg.norm(to)
        out = c.probe_sh_device(dev(P), m=16, spp=16, cube=True)
        chain = c.reflprobe_prefilter_device(out["cube"])
        R = dev(np.float32([to, -to, to, -to]))
        rgb = c.reflprobe_shade_device(chain, 16, R, dev(np.float32([0, 0, 4, 4])), index=dev(np.zeros(4, np.int32)))
        c.synchronize()
        cube = out["cube"].cpu().numpy().reshape(-1, 3)
        d, _, _ = directions_ref(16)
        brightest = d[np.argmax(cube.sum(axis=1))]
        assert float(brightest @ to) > 0.97, (brightest, to)     # within 14 degrees: the ball spans 12, a texel 6
        rgb = rgb.cpu().numpy().sum(axis=1)
        assert rgb[0] > rgb[1] >= 0, rgb
        assert abs(rgb[2] - rgb[3]) < rgb[0] - rgb[1], rgb
    finally:
        c.close()
