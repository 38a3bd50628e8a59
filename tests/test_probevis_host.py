"""Probe visibility on the CPU (qaray_amd/csrc/hip/qa_probevis_dev.h; its opening comment is the specification): the host build of the
moments and of the visibility shading against the float32 restatement of tests/probevis_util.py, bit for bit; what the specification
promises of a point on a probe and of uniform coefficients; the light a wall stops, on the analytic two rooms; and
tests/cpp/probevis_check.cpp, the same functions stand-alone under AddressSanitizer + UBSan.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from probe_util import BAND, F32, MISS, Y_CONST, bits
from probevis_util import (ROOMS_D, ROOMS_DMAX, ROOMS_GRID, ROOMS_M, ROOM_A, ROOM_B, moments_ref, rooms_moments, rooms_points, rooms_sh,
                           vis_grid_shade_ref, vis_weights_f64)
from qaray_amd import hip

U = 2.0 ** -24   # the unit roundoff of fp32


def some_t(rng, K, dmax):
    """Hit parameters around dmax, with the values the clamp has to get right among them"""
    t = rng.uniform(0.0, 2.0 * dmax, K).astype(F32)
    t[rng.random(K) < 0.2] = MISS
    special = [0.0, -0.0, dmax, np.nextafter(F32(dmax), F32(0)), np.nextafter(F32(dmax), F32(9)), 3.0 * dmax, 1e30, 1e-30, np.inf, np.nan]
    at = rng.permutation(K)[: len(special)]
    t[at] = np.array(special[: len(at)], F32)
    return t


@pytest.mark.parametrize("m,d", [(1, 1), (2, 1), (2, 2), (4, 2), (6, 3), (6, 6), (16, 8)])
def test_moments_are_the_restatement(m, d):
    rng = np.random.default_rng(10 * m + d)
    for dmax in (F32(1.5), F32(0.37), F32(40.0)):
        t = some_t(rng, 6 * m * m, dmax)
        got = hip.probevis_moments_host(t, m, d, dmax)
        want = moments_ref(t, m, d, dmax)
        assert got.shape == (6, d, d, 2) and np.array_equal(bits(got), bits(want)), (m, d, dmax)
        assert (got[..., 0] >= 0).all() and (got[..., 0] <= dmax).all() and (got[..., 1] <= dmax * dmax * (1 + 4 * U)).all()
    # all misses: every cell sees dmax
    got = hip.probevis_moments_host(np.full(6 * m * m, MISS), m, d, 2.0)
    assert (got[..., 0] == 2.0).all() and (got[..., 1] == 4.0).all()


def test_moment_cells_pool_the_texels_of_the_cube_map_order():
    """m = 4, d = 2: t = the texel's record index; cell (f, B, C) holds the mean of texels (f, 2B .. 2B + 1, 2C .. 2C + 1)"""
    t = np.arange(96, dtype=F32)
    got = hip.probevis_moments_host(t, 4, 2, 1000.0)
    cube = t.reshape(6, 4, 4)
    for f in range(6):
        for B in range(2):
            for C in range(2):
                block = cube[f, 2 * B:2 * B + 2, 2 * C:2 * C + 2].astype(np.float64)
                assert got[f, B, C, 0] == block.mean() and got[f, B, C, 1] == (block ** 2).mean()


def a_grid(rng, counts, m, d, dmax, void=()):
    """Random coefficients and moments (pooled from random t by the restatement) of a grid; the probes in `void` hold moments 0"""
    probes = int(np.prod(counts))
    sh = rng.uniform(-1, 2, (probes, 9, 3)).astype(F32)
    mo = np.stack([moments_ref(some_t(rng, 6 * m * m, dmax)[: 6 * m * m], m, d, dmax) for _ in range(probes)])
    mo = np.nan_to_num(mo, nan=0.5, posinf=0.5).astype(F32)
    for q in void:
        mo[q] = 0
    return sh, mo


def probe_positions(origin, spacing, counts):
    return hip.ProbeGrid(None, origin, spacing, counts).points()


def shading_points(rng, origin, spacing, counts, n=160):
    """Inside, outside on every side, on probes, on cell faces, along the axes and the diagonals from a probe, and not finite"""
    origin, spacing = np.asarray(origin, F32), np.asarray(spacing, F32)
    span = spacing * (np.asarray(counts) - 1)
    p = rng.uniform(origin - 0.5 * span - 1, origin + 1.5 * span + 1, (n, 3)).astype(F32)
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)
    on = probe_positions(origin, spacing, counts)
    k = min(len(on), 16)
    p[:k] = on[:k]                                                  # rr == 0 at normal_bias 0
    p[16:22] = on[0] + np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * F32(0.25)   # along an axis
    p[22:30] = on[-1] + np.float32([[1, 1, 0], [1, -1, 0], [-1, 1, 0], [0, 1, 1], [0, -1, 1], [1, 0, 1], [1, 1, 1], [-1, -1, -1]]) * F32(0.125)  # ties
    for i in range(30, 40):                                          # on the face between two cells: a probe's coordinate on one axis
        p[i, i % 3] = on[i % len(on)][i % 3]
    for side in range(6):                                            # far outside on every side
        p[40 + side] = origin + 0.5 * span
        p[40 + side, side // 2] = (1e30, -1e30)[side % 2]
    p[46] = (3e38, -3e38, 3e38)
    p[47], p[48], nr[49], nr[50], nr[51] = (np.nan, 0, 0), (0, -np.inf, 0), (0, np.nan, 0), (np.inf, 0, 0), (0, 0, 0)
    nr[52] = (3e38, 3e38, 0)                                         # (a normal that overflows the biased point: the fallback)
    return p, nr


@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 1, 3), (4, 2, 2)])
@pytest.mark.parametrize("m,d", [(6, 1), (6, 2), (6, 3)])
def test_visibility_shading_is_the_restatement(counts, m, d):
    rng = np.random.default_rng(100 * sum(counts) + d)
    probes = int(np.prod(counts))
    for origin, spacing in (((0.5, -1.0, 0.25), (1.0, 0.5, 2.0)), ((0.3, 0.1, -0.7), (0.9, 1.1, 0.35))):
        dmax = F32(1.5) * np.sqrt((np.float32(spacing) ** 2).sum(dtype=F32))
        void = sorted(set(rng.integers(0, probes, probes // 3).tolist()))
        sh, mo = a_grid(rng, counts, m, d, dmax, void)
        p, nr = shading_points(rng, origin, spacing, counts)
        for bias in (0.0, 0.1):
            got = hip.probevis_grid_shade_host(sh, mo, origin, spacing, counts, p, nr, bias)
            want = vis_grid_shade_ref(sh, mo, origin, spacing, counts, p, nr, bias)
            bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
            assert not len(bad), (counts, d, bias, bad[:8], got[bad[:3]], want[bad[:3]])
            assert np.isfinite(got).all() and (got >= 0).all() and not got[47:51].any() and (got > 0).any()
        # the overflowing normal falls back to the trilinear shading
        assert np.array_equal(bits(hip.probevis_grid_shade_host(sh, mo, origin, spacing, counts, p[52:53], nr[52:53], 1.0)),
                              bits(hip.probe_grid_shade_host(sh, origin, spacing, counts, p[52:53], nr[52:53])))


@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 1, 3), (4, 2, 2)])
def test_a_point_on_a_probe_takes_that_probes_shading(counts):
    """A dyadic grid, so that the point is the probe exactly: tri = 1 for one corner, x / x == 1, the other terms are 0 * finite"""
    rng = np.random.default_rng(sum(counts))
    origin, spacing = (0.5, -1.0, 0.25), (1.0, 0.5, 2.0)
    sh, mo = a_grid(rng, counts, 4, 2, 2.0, void=(0,))
    on = probe_positions(origin, spacing, counts)
    nr = rng.standard_normal((len(on), 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)
    got = hip.probevis_grid_shade_host(sh, mo, origin, spacing, counts, on, nr)
    assert np.array_equal(bits(got), bits(hip.probe_shade_host(sh, nr))) and (got > 0).any()


def shade_f64(sh, nr):
    """probeShade of one coefficient set (9, 3) at float32 normals (n, 3), in float64 with the fp32 constants -> (rgb (n, 3), T (n, 3)
    the sum of the nine terms' magnitudes)"""
    x, y, z = (nr[:, e].astype(np.float64) for e in range(3))
    c0, c1, c2, c3, c4 = (float(c) for c in Y_CONST)
    Y = np.stack([np.full(len(nr), c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z, c4 * (x * x - y * y)], axis=1)
    A = np.array([float(BAND[0])] + [float(BAND[1])] * 3 + [float(BAND[2])] * 5)
    terms = A[None, :, None] * sh.astype(np.float64)[None] * Y[:, :, None]
    return np.maximum(terms.sum(axis=1), 0), np.abs(terms).sum(axis=1)


def test_uniform_coefficients_shade_as_one_probe():
    """Every probe holds the same 27 coefficients: whatever the weights, they sum to 1 and the result is that set's shading.

    The bound, to first order in u = 2^-24, relative to T = sum_c |A_c sh_c Y_c(N)| (all w_j >= 0: nothing cancels in the weights):
      W is a sum of eight w_j: eight additions, so sum_j w_j / W = 1 within 8 u;
      a coefficient is sum_j fl(fl(w_j / W) * sh): per term one rounded quotient and one rounded product (2 u), and eight additions of
      terms of one sign (8 u) - 18 u for the coefficient;
      probeShade's nine terms: two products each (2 u; A_c is a constant of the specification), Y_c(N) from at most four roundings
      with |Y_6|'s 3 z^2 - 1 taken against its own bound (8 u), and nine additions (9 u) - 19 u.
    37 u T; 40 u T leaves the second-order terms room.  The reference is the float64 evaluation of the specification - with uniform
    coefficients sum_j (w_j / W) sh = sh there, which vis_weights_f64 confirms - not the code under test."""
    rng = np.random.default_rng(7)
    counts, origin, spacing = (4, 2, 2), (0.3, 0.1, -0.7), (0.9, 1.1, 0.35)
    _, mo = a_grid(rng, counts, 6, 3, 2.0, void=(3, 9))
    one = rng.uniform(-1, 2, (9, 3)).astype(F32)
    sh = np.broadcast_to(one, (16, 9, 3)).copy()
    p, nr = shading_points(rng, origin, spacing, counts, 400)
    ok = np.isfinite(p).all(axis=1) & np.isfinite(nr).all(axis=1) & (np.abs(nr) < 2).all(axis=1)
    p, nr = p[ok], nr[ok]
    k, _ = vis_weights_f64(mo, origin, spacing, counts, p, nr, 0.1)
    assert np.abs(k.sum(axis=1) - 1).max() < 1e-14 and (k >= 0).all()
    want, T = shade_f64(one, nr)
    bound = 40 * U * T
    got = hip.probevis_grid_shade_host(sh, mo, origin, spacing, counts, p, nr, 0.1)
    single = hip.probe_shade_host(np.broadcast_to(one, (len(nr), 9, 3)), nr)
    assert (np.abs(got - want) <= bound).all(), np.max(np.abs(got - want) / np.maximum(T, 1e-30)) / U
    assert (np.abs(single - want) <= bound).all() and (np.abs(got - single) <= 2 * bound).all()
    assert (got > 0).any()


def rooms(side):
    """The analytic two rooms: moments by the hook from each probe's exit distances, band 0 lit in the room across the wall from
    the points -> (visibility, trilinear) shading of the 300 points (n, 3)"""
    d, _, _ = hip.probe_directions_host(ROOMS_M)
    mo = rooms_moments(d[0], lambda t: hip.probevis_moments_host(t, ROOMS_M, ROOMS_D, ROOMS_DMAX))
    sh = rooms_sh(ROOM_A if side == "B" else ROOM_B)
    p, nr = rooms_points(side=side)
    o, s, cn = ROOMS_GRID
    return hip.probevis_grid_shade_host(sh, mo, o, s, cn, p, nr), hip.probe_grid_shade_host(sh, o, s, cn, p, nr)


def leak_ratio(side, capsys):
    vis, tri = rooms(side)
    assert (tri[:, 0] > 0).all() and (vis == vis[:, :1]).all() and (tri == tri[:, :1]).all()
    ratio = vis[:, 0].astype(np.float64) / tri[:, 0]
    with capsys.disabled():
        print(f"\nleak ratio visibility / trilinear, points in {side}: min {ratio.min():.4f} median {np.median(ratio):.4f} max {ratio.max():.4f}, "
              f"{int((ratio >= 1).sum())} of {len(ratio)} at or above 1, ratio of the sums {vis[:, 0].sum(dtype=np.float64) / tri[:, 0].sum(dtype=np.float64):.4f}")
    return vis[:, 0], tri[:, 0], ratio


def test_a_wall_stops_the_light(capsys):
    """300 seeded points in the dark room B beside the wall, x in (2.1, 2.5), random unit normals, nothing selected: at every point
    the visibility result is strictly below the trilinear one.  The shaded value is band 0 alone, so the ratio is the lit probes'
    share of the weight.  Measured by this test (float32 hooks): min 0.0101, median 0.0592, max 0.2595; the float64 prototype of
    the specification gave 0.015 / 0.056 / 0.61 on points of its own."""
    vis, tri, ratio = leak_ratio("B", capsys)
    assert (vis < tri).all(), (ratio.max(), int((vis >= tri).sum()))


def test_the_mirrored_rooms_keep_the_dark_probes_share_down(capsys):
    """The mirror: 300 points in A with x in (1.5, 2.0), B lit - the ratio is the share of the probes across the wall.  Measured by
    this test: min 0.0155, median 0.0574, max 1.1659, 1 of 300 at or above 1 (the prototype: 0.015 / 0.063 / 0.69 on points of its
    own).  A point that lies against the wall is as far from a probe of its own room as that probe's rays travel in the cell, so
    the Chebyshev bound cuts that probe as well and the share of the others can rise: what normal_bias is for.  Hence, as on the
    device, the sums are compared here and the per-point figures are printed."""
    vis, tri, ratio = leak_ratio("A", capsys)
    assert vis.sum(dtype=np.float64) < tri.sum(dtype=np.float64) and np.median(ratio) < 1


def test_hooks_refuse_bad_arguments():
    L = hip.lib()
    t, out = np.zeros(96, F32), np.zeros(6 * 4 * 2, F32)
    for m, d, dmax in ((0, 1, 1.0), (129, 1, 1.0), (4, 0, 1.0), (4, 3, 1.0), (4, 8, 1.0), (4, 2, 0.0), (4, 2, -1.0), (4, 2, np.nan), (4, 2, np.inf)):
        assert L.qa_test_probevis_moments_host(m, d, dmax, t.ctypes.data, out.ctypes.data) == -1, (m, d, dmax)
    assert L.qa_test_probevis_moments_host(4, 2, 1.0, None, out.ctypes.data) == -1 and L.qa_test_probevis_moments_host(4, 2, 1.0, t.ctypes.data, None) == -1
    with pytest.raises(ValueError):
        hip.probevis_moments_host(t, 4, 3, 1.0)
    with pytest.raises(ValueError):
        hip.probevis_moments_host(t[:-1], 4, 2, 1.0)
    sh, mo = np.zeros((2, 9, 3), F32), np.zeros((2, 6, 2, 2, 2), F32)
    p = np.zeros((1, 3), F32)
    with pytest.raises(ValueError):
        hip.probevis_grid_shade_host(sh, mo[:1], (0, 0, 0), (1, 1, 1), (2, 1, 1), p, p)
    with pytest.raises(ValueError):
        hip.probevis_grid_shade_host(sh, mo[:, :, :, :1], (0, 0, 0), (1, 1, 1), (2, 1, 1), p, p)
    with pytest.raises(hip.HipError):
        hip.probevis_grid_shade_host(sh, mo, (0, 0, 0), (1, 1, 1), (2, 1, 1), p, p, normal_bias=np.inf)
    with pytest.raises(hip.HipError):
        hip.probevis_grid_shade_host(sh, mo, (0, 0, 0), (1, 0, 1), (2, 1, 1), p, p)
    par = hip.ProbeVisParams.default()
    assert (par.d, par.dmax, par.normal_bias) == (8, 0.0, 0.0)
    g = hip.ProbeGrid(None, (0, 0, 0), (1, 1, 1), (2, 1, 1))
    assert g.moments is None and g.dmax is None


def test_header_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/probevis_check.cpp: the header's host half on heap buffers of exactly their size, stand-alone under ASan / UBSan
    (nothing is loaded into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "probevis_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "probevis_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "probevis_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
