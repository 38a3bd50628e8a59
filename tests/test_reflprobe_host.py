"""Reflection probes on the CPU (qaray_amd/csrc/hip/qa_reflprobe_dev.h; its opening comment is the specification): the host build of the
layout, the prefilter, the lookup and the grid lookup against the float32 restatement of tests/reflprobe_util.py, bit for bit; three
analytic anchors - a constant cube, a half-lit sky, and the 1 x 1 level against the diffuse shading of the projected harmonics; and
tests/cpp/reflprobe_check.cpp, the same functions stand-alone under AddressSanitizer + UBSan.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from probe_util import F32, bits, directions_ref
from reflprobe_util import grid_lookup_ref, layout_ref, lookup_ref, prefilter_ref
from qaray_amd import hip


def random_cube(rng, n, m):
    return rng.uniform(0, 4, (n, 6, m, m, 3)).astype(F32)


def special_cube(rng, n, m):
    """NaN, inf, -0 and denormal texels among random ones, and negative ones: nothing is clamped"""
    cube = rng.uniform(-1, 3, (n, 6, m, m, 3)).astype(F32)
    flat = cube.reshape(n, -1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42, -1e-45, 3e38, 0.0], F32)
    for q in range(n):
        at = rng.permutation(flat.shape[1])[: len(special)]
        flat[q, at] = special
    return cube


@pytest.mark.parametrize("m", [1, 2, 4, 8, 16])
def test_the_layout_is_the_comments(m):
    lg = m.bit_length() - 1
    for L in range(1, lg + 2):
        got = hip.reflprobe_layout(m, L)
        _, offset, res, squarings, T = layout_ref(m, L)
        assert got["levels"] == L and got["texels"] == T
        assert got["offset"].tolist() == offset and got["res"].tolist() == res and got["squarings"].tolist() == squarings
    assert hip.reflprobe_layout(m)["levels"] == lg + 1
    if m == 16:
        assert hip.reflprobe_layout(16)["squarings"].tolist() == [0, 5, 3, 1, 0] and hip.reflprobe_layout(16)["texels"] == 6 * (256 + 64 + 16 + 4 + 1)
    for bad in (0, lg + 2):
        with pytest.raises(ValueError):
            hip.reflprobe_layout(m, bad)
        assert hip.lib().qa_reflprobe_layout(m, bad, None, None, None, None) == -1
    for bad_m in (0, 3, 6, 12, 256, -4):
        with pytest.raises(ValueError):
            hip.reflprobe_layout(bad_m)
        assert hip.lib().qa_reflprobe_layout(bad_m, 1, None, None, None, None) == -1


@pytest.mark.parametrize("m", [1, 2, 4, 8])
def test_the_prefilter_is_the_restatement(m):
    """Every L at m = 1, 2, 4, 8; random cubes and cubes with NaN, inf, -0 and denormal texels; batches of 1, 2 and 5; a zero cube"""
    rng = np.random.default_rng(40 + m)
    lg = m.bit_length() - 1
    for L in range(1, lg + 2):
        for n, make in ((1, random_cube), (2, special_cube), (5, random_cube), (5, special_cube)):
            cube = make(rng, n, m)
            got = hip.reflprobe_prefilter_host(cube, L)
            want = prefilter_ref(cube, L)
            assert got.shape == want.shape == (n, layout_ref(m, L)[4], 3)
            assert np.array_equal(bits(got), bits(want)), (m, L, n, make.__name__)
            # level 0 is the cube, bit for bit
            assert np.array_equal(bits(got[:, : 6 * m * m]), bits(cube.reshape(n, -1, 3)))
        zero = hip.reflprobe_prefilter_host(np.zeros((2, 6, m, m, 3), F32), L)
        assert not bits(zero).any()


def test_the_prefilter_is_the_restatement_at_16():
    rng = np.random.default_rng(16)
    cube = special_cube(rng, 2, 16)
    cube[1] = random_cube(rng, 1, 16)[0]
    got, want = hip.reflprobe_prefilter_host(cube, 5), prefilter_ref(cube, 5)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(got[1]).all() and not np.isfinite(got[0]).all()


def test_a_nan_texel_reaches_the_outputs_whose_lobe_covers_it():
    """One NaN texel at the centre of +x, m = 8: at level 3 (exponent 1) the hemisphere around it is NaN and -x is not; at level 1
    (exponent 8) it is covered by fewer texels than at level 2"""
    cube = np.ones((1, 6, 8, 8, 3), F32)
    cube[0, 0, 4, 4, 1] = np.nan
    chain = hip.reflprobe_prefilter_host(cube)
    L, offset, res, _, T = layout_ref(8)
    top = chain[0, offset[3]:]
    assert np.isnan(top[0, 1]) and not np.isnan(top[1]).any() and not np.isnan(top[:, [0, 2]]).any()
    share = [np.isnan(chain[0, offset[l]:offset[l] + 6 * res[l] ** 2, 1]).mean() for l in (1, 2, 3)]
    assert 0 < share[0] <= share[1] <= share[2] < 1


def lookup_directions(rng, n=64):
    """Random ones; the axes, the edge and corner diagonals (the tie rule); just inside every face edge; not finite; zero; huge; tiny"""
    R = rng.standard_normal((n, 3)).astype(F32)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    fixed += [(sx, sy, 0) for sx in (1, -1) for sy in (1, -1)] + [(0, sy, sz) for sy in (1, -1) for sz in (1, -1)] + [(sx, 0, sz) for sx in (1, -1) for sz in (1, -1)]
    fixed += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    inside = np.nextafter(F32(1), F32(0))
    for a in range(3):
        for s in (1, -1):
            for e, t in ((1, inside), (1, -inside), (2, inside), (2, -inside)):
                v = [0.25, 0.25, 0.25]
                v[a], v[(a + e) % 3] = s, t
                fixed.append(tuple(v))
    fixed += [(np.nan, 0, 1), (0, np.inf, 0), (1, 1, -np.inf), (0, 0, 0), (-0.0, 0.0, -0.0), (3e38, -3e38, 1e38), (1e-45, 0, 0), (1e-40, -1e-40, 1e-41), (2, 0.5, -0.5)]
    return np.concatenate([np.array(fixed, F32), R])


def lookup_levels(rng, n, L):
    """At, between and outside the levels, and not finite"""
    lam = rng.uniform(-1, L, n).astype(F32)
    special = [0, L - 1, L - 0.5, L, L + 3, -0.0, -2, 0.5, 1, 1.25, np.inf, -np.inf, np.nan, 1e30]
    lam[: len(special)] = np.array(special, F32)
    return rng.permutation(lam)


@pytest.mark.parametrize("m", [1, 2, 4])
def test_the_lookup_is_the_restatement(m):
    """Chains whose coarsest level has r = 1, 2 and 4 texels per face edge (and every L above it)"""
    rng = np.random.default_rng(70 + m)
    lg = m.bit_length() - 1
    for big in (m, 4 * m):
        if big > 16:
            continue
        L = (big.bit_length() - 1) - lg + 1   # the last level has m texels per face edge
        chain = rng.uniform(-1, 3, (7, layout_ref(big, L)[4], 3)).astype(F32)
        R = lookup_directions(rng)
        lam = lookup_levels(rng, len(R), L)
        index = rng.integers(-3, 10, len(R)).astype(np.int32)
        index[:4] = (-2 ** 31, 2 ** 31 - 1, 0, 6)
        got = hip.reflprobe_shade_host(chain, big, R, lam, L, index)
        want = lookup_ref(chain, big, R, lam, L, index)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert not len(bad), (big, L, bad[:8], R[bad[:3]], lam[bad[:3]], got[bad[:3]], want[bad[:3]])
        void = ~np.isfinite(R).all(axis=1) | (R == 0).all(axis=1) | np.isnan(lam)
        assert void.sum() >= 6 and not got[void].any() and (got[~void] != 0).any()
        # without an index lookup i takes probe i
        few = hip.reflprobe_shade_host(chain, big, R[:7], lam[:7], L)
        assert np.array_equal(bits(few), bits(lookup_ref(chain, big, R[:7], lam[:7], L)))


def test_a_texel_centre_at_a_level_answers_that_texel():
    """The direction of every texel centre of level l at lambda = l: g lands on the texel up to rounding, so the answer is the
    texel within the blend's error; at m = 1 and a whole level it is the texel exactly"""
    rng = np.random.default_rng(3)
    chain = rng.uniform(0, 1, (1, layout_ref(8)[4], 3)).astype(F32)
    L, offset, res, _, _ = layout_ref(8)
    for l in range(L):
        d, _, _ = directions_ref(res[l])
        got = hip.reflprobe_shade_host(chain, 8, d, np.full(len(d), l, F32), index=np.zeros(len(d), np.int32))
        want = chain[0, offset[l]:offset[l] + len(d)]
        assert np.abs(got - want).max() < 1e-5, l
    assert np.array_equal(bits(got), bits(want))   # (the 1 x 1 level: both taps are the one texel, f = 0)


def grid_points(rng, origin, spacing, counts, n=96):
    origin, spacing = np.asarray(origin, F32), np.asarray(spacing, F32)
    span = spacing * (np.asarray(counts) - 1)
    p = rng.uniform(origin - 0.5 * span - 1, origin + 1.5 * span + 1, (n, 3)).astype(F32)
    for side in range(6):                                            # far outside on every side
        p[side] = origin + 0.5 * span
        p[side, side // 2] = (1e30, -1e30)[side % 2]
    p[6], p[7], p[8] = (np.nan, 0, 0), (0, -np.inf, 0), (3e38, -3e38, 3e38)
    return p


@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 1, 3), (4, 2, 2)])
def test_the_grid_lookup_is_the_restatement(counts):
    rng = np.random.default_rng(sum(counts))
    probes = int(np.prod(counts))
    for m, L in ((4, 3), (4, 1), (2, 2)):
        chain = rng.uniform(-1, 3, (probes, layout_ref(m, L)[4], 3)).astype(F32)
        for origin, spacing in (((0.5, -1.0, 0.25), (1.0, 0.5, 2.0)), ((0.3, 0.1, -0.7), (0.9, 1.1, 0.35))):
            p = grid_points(rng, origin, spacing, counts)
            R = lookup_directions(rng, 0)
            R = np.concatenate([rng.standard_normal((len(p) - len(R), 3)).astype(F32), R]) if len(R) < len(p) else R[: len(p)]
            lam = lookup_levels(rng, len(p), L)
            got = hip.reflprobe_grid_shade_host(chain, m, origin, spacing, counts, p, R, lam, L)
            want = grid_lookup_ref(chain, m, origin, spacing, counts, p, R, lam, L)
            bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
            assert not len(bad), (counts, m, L, bad[:8], got[bad[:3]], want[bad[:3]])
            assert not got[6:8].any() and (got != 0).any()
    # a point on a probe takes that probe's answer exactly (a dyadic grid, so that the point is the probe)
    origin, spacing = (0.5, -1.0, 0.25), (1.0, 0.5, 2.0)
    on = hip.ProbeGrid(None, origin, spacing, counts).points()
    R = rng.standard_normal((len(on), 3)).astype(F32)
    lam = rng.uniform(0, 1, len(on)).astype(F32)
    got = hip.reflprobe_grid_shade_host(chain, 2, origin, spacing, counts, on, R, lam, 2)
    assert np.array_equal(bits(got), bits(hip.reflprobe_shade_host(chain, 2, R, lam, 2))) and (got != 0).any()


def test_a_constant_cube_stays_constant():
    """Anchor 1: out = sum(q c) / sum(q) of a constant c.  The float32 prototype of the specification gave a relative deviation of
    1.7e-6 at most at m = 16; 1e-5 is asserted."""
    cube = np.empty((1, 6, 16, 16, 3), F32)
    cube[...] = np.float32([0.7, 1.3, 2.9])
    chain = hip.reflprobe_prefilter_host(cube)
    rel = np.abs(chain[0] / np.float32([0.7, 1.3, 2.9]) - 1)
    assert rel.max() <= 1e-5, rel.max()
    assert not rel[:1536].any()


def sky(m=16):
    """1 above z = 0 and 0 below, by the texel centres' directions"""
    d, _, _ = directions_ref(m)
    return np.repeat((d[:, 2] > 0).astype(F32)[:, None], 3, axis=1).reshape(1, 6, m, m, 3)


def test_the_half_lit_sky_at_the_1x1_level():
    """Anchor 2: the 1 x 1 level is the cosine-weighted mean: exactly 1 on +z, exactly 0 on -z, 0.5 on the four sides (the prototype
    gave 0.4999999 .. 0.5000001; 1e-5 is asserted)"""
    chain = hip.reflprobe_prefilter_host(sky())
    top = chain[0, layout_ref(16)[1][4]:]
    assert top.shape == (6, 3)
    assert (top[4] == 1).all() and (top[5] == 0).all()
    assert np.abs(top[:4] - 0.5).max() <= 1e-5, top[:4]


def test_the_1x1_level_agrees_with_the_diffuse_shading():
    """Anchor 3: on that sky the 1 x 1 level along +z, -z and +x against probe_shade_host of the projected harmonics, within 2e-3 (the
    bound tests/test_probe_host.py puts on the SH side) + 1e-5"""
    cube = sky()
    d, w, _ = hip.probe_directions_host(16)
    sh, _, _ = hip.probe_project_host(d[0], w[0], cube.reshape(-1, 3), np.ones(1536, F32))
    R = np.float32([[0, 0, 1], [0, 0, -1], [1, 0, 0]])
    diffuse = hip.probe_shade_host(np.broadcast_to(sh, (3, 9, 3)), R)
    chain = hip.reflprobe_prefilter_host(cube)
    glossy = hip.reflprobe_shade_host(chain, 16, R, np.full(3, 4, F32), index=np.zeros(3, np.int32))
    assert np.abs(glossy - diffuse).max() <= 2e-3 + 1e-5, (glossy, diffuse)
    assert np.abs(glossy[:, 0] - np.float32([1, 0, 0.5])).max() <= 1e-5


def test_the_level_of_a_glossiness():
    """Documented, not asserted against anything but its formula and its clamp"""
    assert hip.reflprobe_level([128, 32, 8, 4, 1e9, 0, np.nan], 16).tolist() == [1, 2, 3, 3.5, 0, 4, 0]
    assert hip.reflprobe_level(2.0, 16, 2) == 1 and hip.reflprobe_level(2.0, 16).dtype == np.float32


def test_hooks_refuse_bad_arguments():
    L = hip.lib()
    cube, chain = np.zeros((1, 6, 4, 4, 3), F32), np.full((1, 126, 3), 7, F32)
    pc, ph = cube.ctypes.data, chain.ctypes.data
    for n, c, m, lv, out in ((1, None, 4, 3, ph), (1, pc, 4, 3, None), (1, pc, 3, 1, ph), (1, pc, 0, 1, ph), (1, pc, 256, 1, ph), (1, pc, 4, 0, ph), (1, pc, 4, 4, ph),
                             (1 << 31, pc, 4, 3, ph)):
        assert L.qa_test_reflprobe_prefilter_host(n, c, m, lv, out) == -1, (n, m, lv)
    assert L.qa_test_reflprobe_prefilter_host(0, None, 0, 0, None) == 0
    d, lam, rgb = np.zeros((2, 3), F32), np.zeros(2, F32), np.full((2, 3), 7, F32)
    pd, pl, pr = d.ctypes.data, lam.ctypes.data, rgb.ctypes.data
    for args in ((2, None, 2, 4, 3, pd, pl, None, pr), (2, ph, 2, 4, 3, None, pl, None, pr), (2, ph, 2, 4, 3, pd, None, None, pr), (2, ph, 2, 4, 3, pd, pl, None, None),
                 (2, ph, 0, 4, 3, pd, pl, None, pr), (2, ph, 1, 4, 3, pd, pl, None, pr), (2, ph, 2, 5, 1, pd, pl, None, pr), (2, ph, 2, 4, 4, pd, pl, None, pr),
                 (2, ph, 1 << 31, 4, 3, pd, pl, None, pr)):
        assert L.qa_test_reflprobe_shade_host(*args) == -1, args
    one, cn = np.ones(3, F32), np.int32([1, 1, 1])
    ok = [2, ph, 4, 3, one.ctypes.data, one.ctypes.data, cn.ctypes.data, pd, pd, pl, pr]
    for at, bad in ((1, None), (2, 5), (3, 0), (4, None), (5, np.float32([1, 0, 1]).ctypes.data), (6, np.int32([1, 0, 1]).ctypes.data), (7, None), (8, None), (9, None), (10, None)):
        args = list(ok)
        args[at] = bad
        assert L.qa_test_reflprobe_grid_shade_host(*args) == -1, at
    assert (chain == 7).all() and (rgb == 7).all()
    with pytest.raises(ValueError):
        hip.reflprobe_prefilter_host(np.zeros((1, 6, 4, 3, 3)))
    with pytest.raises(ValueError):
        hip.reflprobe_shade_host(chain[:, :100], 4, d, lam)
    with pytest.raises(ValueError):
        hip.reflprobe_grid_shade_host(chain, 4, (0, 0, 0), (1, 1, 1), (2, 1, 1), d, d, lam)
    g = hip.ProbeGrid(None, (0, 0, 0), (1, 1, 1), (2, 1, 1))
    assert g.chain is None and g.m is None and g.levels is None


def test_header_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/reflprobe_check.cpp: the header's host half on heap buffers of exactly their size, stand-alone under ASan / UBSan
    (nothing is loaded into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "reflprobe_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "reflprobe_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "reflprobe_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
