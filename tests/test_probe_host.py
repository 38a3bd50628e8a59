"""Light probes on the CPU: the host build of qaray_amd/csrc/hip/qa_lightprobe_dev.h (hip.probe_directions_host, probe_project_host,
probe_shade_host, probe_grid_shade_host: the source the kernels of qa_lightprobe.hip are compiled from) against the float32 numpy
restatement of the header's opening comment in tests/probe_util.py, bit for bit; the analytic anchors of the cube-map direction set in
float64; tests/cpp/probe_check.cpp runs the same functions stand-alone under AddressSanitizer + UBSan on buffers of exactly the sizes
it is given."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from probe_util import F32, MISS, basis_ref, bits, directions_ref, grid_shade_ref, project_ref, shade_ref
from qaray_amd import hip

SEEDS = (0x51A7A7, 0, 0xFFFFFFFF)
STREAMS = (0, 1, 0xFFFFFFFF)
RESOLUTIONS = (1, 2, 3, 5, 16)


@pytest.mark.parametrize("jitter", (False, True), ids=("centres", "jitter"))
@pytest.mark.parametrize("m", RESOLUTIONS)
def test_directions_weights_and_streams_are_the_restatement(m, jitter):
    K = 6 * m * m
    for seed in SEEDS:
        d, w, rs = hip.probe_directions_host(m, STREAMS, seed, jitter)
        assert d.shape == (3, K, 3) and w.shape == (3, K) and rs.shape == (3, K)
        for q, S in enumerate(STREAMS):
            rd, rw, rstream = directions_ref(m, seed, S, jitter)
            assert np.array_equal(bits(d[q]), bits(rd)), (m, seed, S)
            assert np.array_equal(bits(w[q]), bits(rw)), (m, seed, S)
            assert np.array_equal(rs[q], rstream), (m, seed, S)
    # what the comment says of the set: unit directions (to the 4e-7 of a fp32 normalisation, as tests/cpp/ao_check.cpp), positive
    # weights, the texel centres without jitter
    length = np.linalg.norm(d.astype(np.float64), axis=2)
    assert np.abs(length - 1).max() < 4e-7 and (w > 0).all()
    if not jitter:
        assert np.array_equal(bits(d[0]), bits(d[2])), "the centres do not depend on the stream"
    else:
        assert not np.array_equal(bits(d[0]), bits(d[1])), "the jitter does"


def test_faces_follow_the_cube_map_order():
    """m = 1: six rays along +x, -x, +y, -y, +z, -z, each of weight 4 (a face's plane measure; normalised by W in the projection)"""
    d, w, rs = hip.probe_directions_host(1, (5,))
    assert np.array_equal(d[0], F32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]))
    assert (w == 4).all() and np.array_equal(rs[0], 30 + np.arange(6, dtype=np.uint32))


def rays_of(m, rng, special):
    K = 6 * m * m
    d, w, _ = hip.probe_directions_host(m, (7,), SEEDS[0], True)
    rgb = rng.uniform(0, 4, (K, 3)).astype(F32)
    t = np.where(rng.random(K) < 0.4, MISS, rng.uniform(0.01, 50, K)).astype(F32)
    if special:
        at = rng.choice(K * 3, min(4, K), replace=False)
        rgb.reshape(-1)[at] = np.resize(F32([np.nan, np.inf, -0.0, -np.inf]), len(at))
    return d[0], w[0], rgb, t


@pytest.mark.parametrize("special", (False, True), ids=("finite", "nan-inf-negzero"))
@pytest.mark.parametrize("m", (1, 3, 4, 5))   # K = 6, 54, 96, 150: below, across and well above 64 lanes
def test_projection_is_the_waves_order(m, special):
    rng = np.random.default_rng(100 * m + special)
    for _ in range(4):
        d, w, rgb, t = rays_of(m, rng, special)
        sh, hits, tmin = hip.probe_project_host(d, w, rgb, t)
        rsh, rhits, rtmin = project_ref(d, w, rgb, t)
        assert np.array_equal(bits(sh), bits(rsh)), m
        assert hits == rhits == int((t < MISS).sum()) and bits(tmin) == bits(rtmin) and tmin == t.min()
    # no hit at all: hits 0, tmin the miss value; a -0 radiance keeps +0 coefficients
    sh, hits, tmin = hip.probe_project_host(d, w, np.full_like(rgb, -0.0), np.full_like(t, MISS))
    assert hits == 0 and tmin == MISS and np.array_equal(bits(sh), bits(project_ref(d, w, np.full_like(rgb, -0.0), np.full_like(t, MISS))[0]))


def test_a_constant_environment_projects_onto_band_0():
    d, w, _ = hip.probe_directions_host(16)
    K = d.shape[1]
    sh, hits, tmin = hip.probe_project_host(d[0], w[0], np.broadcast_to(F32([0.75, 0.0625, 2.0]), (K, 3)), np.full(K, MISS, F32))
    assert hits == 0 and tmin == MISS
    want = np.float64([0.75, 0.0625, 2.0]) * 0.282095 * 4 * np.pi
    # band 0 up to the rounding of 24 additions per lane and six folds; the other bands by the Gram bound below: 0.005 * L * sqrt(4 pi)
    assert np.abs(sh[0] - want).max() < 1e-5 * want.max() and np.abs(sh[1:]).max() < 0.005 * 2.0 * np.sqrt(4 * np.pi)


def normals_with_void(rng, n):
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)
    nr[: min(6, n)] = F32([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0, -0.8], [0, 0, 0], [-0.0, 0.8, 0.6]])[: min(6, n)]
    return nr


def test_shade_is_the_restatement():
    rng = np.random.default_rng(4)
    for n in (1, 63, 64, 65, 130):
        sh = rng.uniform(-1, 2, (n, 9, 3)).astype(F32)
        nr = normals_with_void(rng, n)
        assert np.array_equal(bits(hip.probe_shade_host(sh, nr)), bits(shade_ref(sh, nr))), n
        idx = rng.integers(-3, n + 3, n).astype(np.int32)   # (outside [0, probes) on both sides: clamped)
        assert np.array_equal(bits(hip.probe_shade_host(sh, nr, idx)), bits(shade_ref(sh, nr, idx))), n
    # normals that are not finite shade to 0; coefficients that are not finite shade to what the sum gives, NaN to 0
    bad = F32([[np.nan, 0, 1], [0, np.inf, 0], [0, 0, -np.inf]])
    assert not hip.probe_shade_host(sh[:3], bad).any()
    sh[0, 0, 0], sh[1, 2, 1] = np.nan, np.inf
    got = hip.probe_shade_host(sh[:2], nr[:2])
    assert np.array_equal(bits(got), bits(shade_ref(sh[:2], nr[:2]))) and got[0, 0] == 0


GRIDS = (
    ((-1.0, 2.0, 0.5), (0.5, 0.25, 2.0), (3, 4, 2)),
    ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 3)),      # a count of 1 on an axis
    ((5.0, -3.0, 1.0), (0.1, 7.0, 0.3), (1, 1, 1)),      # a single probe
    ((-2.0, -2.0, -2.0), (1.0, 1.0, 1.0), (1, 5, 1)),
)


@pytest.mark.parametrize("origin,spacing,counts", GRIDS)
def test_grid_shade_is_the_restatement(origin, spacing, counts):
    rng = np.random.default_rng(sum(counts))
    o, sp, cn = np.float32(origin), np.float32(spacing), np.int32(counts)
    probes = int(np.prod(cn))
    sh = rng.uniform(-1, 2, (probes, 9, 3)).astype(F32)
    hi = o + sp * (cn - 1)
    inside = rng.uniform(o - sp, hi + sp, (200, 3)).astype(F32)            # inside, and outside on every side by up to a cell
    far = np.float32([[-1e6, 0, 0], [1e6, 0, 0], [0, -1e6, 0], [0, 1e6, 0], [0, 0, -1e6], [0, 0, 1e6], [1e30, -1e30, 1e30]])
    grid = hip.ProbeGrid(None, o, sp, cn).points()                         # exactly on the probes
    void = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])
    p = np.concatenate([inside, far, grid, void, inside[:3]])
    nr = normals_with_void(rng, len(p))
    nr[-3:] = void                                                          # (and normals that are not finite)
    got = hip.probe_grid_shade_host(sh, o, sp, cn, p, nr)
    assert np.array_equal(bits(got), bits(grid_shade_ref(sh, o, sp, cn, p, nr)))
    assert not got[-6:].any() and (got > 0).any()
    # a point on a probe takes that probe's coefficients exactly: the plain shade of that probe
    at = slice(len(inside) + len(far), len(inside) + len(far) + probes)
    assert np.array_equal(bits(got[at]), bits(hip.probe_shade_host(sh, nr[at])))


def test_grid_points_are_in_the_order_of_the_probe_index():
    g = hip.ProbeGrid(None, (1, 2, 3), (0.5, 1, 2), (2, 1, 3))
    assert g.probes == 6
    assert np.array_equal(g.points(), F32([[1, 2, 3], [1.5, 2, 3], [1, 2, 5], [1.5, 2, 5], [1, 2, 7], [1.5, 2, 7]]))


# ---- the analytic anchors, in float64 from the host hooks' directions and weights at m = 16 with centres
def anchor_set():
    d, w, _ = hip.probe_directions_host(16)
    return d[0].astype(np.float64), w[0].astype(np.float64)


def basis64(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full(len(d), 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3 * z * z - 1), 1.092548 * x * z, 0.546274 * (x * x - y * y)], axis=1)


def shade64(sh, n):
    A = np.array([1.0] + [2.0 / 3.0] * 3 + [0.25] * 5)
    return float((A * sh * basis64(np.float64([n]))[0]).sum())


def project64(radiance):
    d, w = anchor_set()
    return (w * radiance) @ basis64(d) * (4 * np.pi / w.sum())


def test_the_gram_matrix_of_the_direction_set_is_the_identity_within_0_005():
    d, w = anchor_set()
    Y = basis64(d)
    gram = (Y * w[:, None]).T @ Y * (4 * np.pi / w.sum())
    dev = np.abs(gram - np.eye(9)).max()
    print("gram deviation", dev)
    assert dev < 0.005


def test_a_constant_sky_shades_to_one_within_1e_5():
    d, _ = anchor_set()
    sh = project64(np.ones(len(d)))
    for n in ((0, 0, 1), (0, 0, -1), (1, 0, 0), (0.6, 0, -0.8)):
        print("constant sky", n, shade64(sh, n))
        assert abs(shade64(sh, n) - 1) < 1e-5


def test_an_upper_hemisphere_sky_shades_to_1_0_and_a_half_within_2e_3():
    d, _ = anchor_set()
    sh = project64((d[:, 2] > 0).astype(np.float64))
    for n, want in (((0, 0, 1), 1.0), ((0, 0, -1), 0.0), ((1, 0, 0), 0.5)):
        print("hemisphere sky", n, shade64(sh, n))
        assert abs(shade64(sh, n) - want) < 2e-3


def test_the_restated_basis_is_the_float64_one():
    d, _ = anchor_set()
    assert np.abs(basis_ref(d.astype(F32)) - basis64(d)).max() < 1e-6


def test_hooks_refuse_bad_arguments():
    with pytest.raises(ValueError):
        hip.probe_directions_host(0)
    with pytest.raises(ValueError):
        hip.probe_directions_host(129)
    with pytest.raises(ValueError):
        hip.probe_project_host(np.zeros((6, 3)), np.zeros(5), np.zeros((6, 3)), np.zeros(6))
    with pytest.raises(ValueError):
        hip.probe_shade_host(np.zeros((2, 9, 3)), np.zeros((2, 3)), np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        hip.probe_grid_shade_host(np.zeros((2, 9, 3)), (0, 0, 0), (1, 1, 1), (2, 2, 1), np.zeros((1, 3)), np.zeros((1, 3)))
    with pytest.raises(ValueError):
        hip.ProbeGrid(None, (0, 0, 0), (1, 0, 1), (2, 2, 1))
    L = hip.lib()
    z = np.zeros(64, F32)
    p = z.ctypes.data
    assert L.qa_test_probe_directions_host(0, 1, 0, p, 1, p, None, None) == -1       # QA_EINVAL
    assert L.qa_test_probe_directions_host(129, 1, 0, p, 1, p, None, None) == -1
    assert L.qa_test_probe_directions_host(1, 1, 1, p, 1, p, None, None) == -1       # a flag that is not QA_PROBE_JITTER
    assert L.qa_test_probe_directions_host(1, 1, 0, None, 1, p, None, None) == -1
    assert L.qa_test_probe_directions_host(1, 1, 0, p, 1, None, None, None) == -1
    assert L.qa_test_probe_directions_host(1, 1, 0, None, 0, None, None, None) == 0
    assert L.qa_test_probe_project_host(1, p, p, p, p, None, None, None) == -1
    assert L.qa_test_probe_project_host(1, p, None, p, p, p, None, None) == -1
    assert L.qa_test_probe_shade_host(1, p, 0, p, None, p) == -1
    assert L.qa_test_probe_shade_host(2, p, 1, p, None, p) == -1                     # fewer probes than points and no index
    one, bad, cn, c0 = np.ones(3, F32), F32([1, 0, 1]), np.int32([1, 1, 1]), np.int32([1, 0, 1])
    assert L.qa_test_probe_grid_shade_host(1, p, p, bad.ctypes.data, cn.ctypes.data, p, p, p) == -1
    assert L.qa_test_probe_grid_shade_host(1, p, p, one.ctypes.data, c0.ctypes.data, p, p, p) == -1
    assert L.qa_test_probe_grid_shade_host(1, p, p, one.ctypes.data, cn.ctypes.data, None, p, p) == -1
    par = hip.ProbeParams.default()
    assert (par.m, par.spp, par.max_bounce, par.seed, par.flags, par.chunk_rays) == (16, 1, 5, hip.DEFAULT_SEED, 0, 0)
    assert hip.QA_PROBE_JITTER == 16 and not hip.QA_PROBE_JITTER & (hip.QA_RADIANCE_PER_SAMPLE | hip.QA_RADIANCE_MISS_ENVIRONMENT | hip.QA_RADIANCE_PHOTON_MAPS)


def test_header_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/probe_check.cpp: the header's host half on heap buffers of exactly their size, stand-alone under ASan / UBSan (nothing
    is loaded into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "probe_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "probe_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "probe_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
