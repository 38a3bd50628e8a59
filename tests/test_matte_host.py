"""The matte planes on the CPU: the host build of qaray_amd/csrc/hip/qa_matte_dev.h (hip.matte_accumulate_host,
hip.matte_rgba_host: the source the kernels of qa_matte.hip are compiled from) against the float32 numpy restatements of the header's
opening comment in tests/matte_util.py, bit for bit and byte for byte; tests/cpp/matte_check.cpp runs the same functions stand-alone
under AddressSanitizer + UBSan on buffers of exactly the sizes it is given."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from matte_util import F32, accumulate_ref, bits, linear_byte, rgba_edge_frames, rgba_ref
from qaray_amd import hip

PATTERNS = ("all", "none", "alternating", "first_only", "last_only")


def hit_pattern(name, n):
    hit = np.zeros(n, bool)
    if name == "all":
        hit[:] = True
    elif name == "alternating":
        hit[::2] = True
    elif name == "first_only":
        hit[0] = True
    elif name == "last_only":
        hit[-1] = True
    return hit


def sample_values(n, seed):
    """Colours in [0, 1) with the texedge scenes' 1e21 and exact zeros among them, unit-ish normals of both signs"""
    rng = np.random.default_rng(seed)
    values = rng.uniform(0, 1, (n, 3)).astype(F32)
    values[rng.integers(0, n, max(1, n // 7)), rng.integers(0, 3, max(1, n // 7))] = F32(1e21)
    values[rng.integers(0, n, max(1, n // 5))] = 0
    values[0] = (F32(1e21), 0, F32(0.25))   # (so that every n, n = 1 included, holds both)
    normals = rng.normal(size=(n, 3)).astype(F32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True).astype(F32)
    return values, normals


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", [1, 2, 5, 64, 2048])
def test_accumulate_is_the_restated_running_mean(n, pattern):
    values, normals = sample_values(n, 100 * n + len(pattern))
    hit = hit_pattern(pattern, n)
    got = hip.matte_accumulate_host(values, normals, hit)
    want = accumulate_ref(values, normals, hit)
    for k in hip.MATTE_PLANES:
        assert np.array_equal(bits(np.asarray(got[k], F32)), bits(np.asarray(want[k], F32))), (k, got[k], want[k])
    hits = int(hit.sum())
    assert got["coverage"] == F32(hits) / F32(n)
    if hits == 0:
        assert not bits(got["normal"]).any() and np.array_equal(bits(got["backdrop"]), bits(got["albedo"]))
    if hits == n:
        assert not bits(got["backdrop"]).any()
    assert (values == F32(1e21)).any() and (values == 0).any()


def test_one_sample_is_the_value_itself_and_none_is_zero():
    values, normals = sample_values(1, 3)
    hit = hip.matte_accumulate_host(values, normals, [True])
    assert np.array_equal(bits(hit["albedo"]), bits(values[0])) and np.array_equal(bits(hit["normal"]), bits(normals[0]))
    assert hit["coverage"] == 1 and not bits(hit["backdrop"]).any()
    miss = hip.matte_accumulate_host(values, normals, [False])
    assert np.array_equal(bits(miss["backdrop"]), bits(values[0])) and miss["coverage"] == 0 and not bits(miss["normal"]).any()
    empty = hip.matte_accumulate_host(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, bool))
    assert all(not bits(np.asarray(empty[k], F32)).any() for k in hip.MATTE_PLANES)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("frame", ["1x1", "17x13", "33x35"])
def test_rgba_is_the_restated_straight_alpha(frame, srgb):
    rgb, backdrop, coverage, ns = rgba_edge_frames()[frame]
    got = hip.matte_rgba_host(rgb, backdrop, coverage, ns, srgb)
    want = rgba_ref(rgb, backdrop, coverage, ns, srgb)
    assert got.shape == coverage.shape + (4,) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (got[ns == 0] == 0).all()
    live = ns != 0
    # alpha: coverage through the linear byte whatever srgb is; a NaN coverage is byte 0 and its colour 0
    assert np.array_equal(got[..., 3][live], linear_byte(coverage)[live])
    nan_a = live & np.isnan(coverage)
    assert (got[nan_a] == 0).all()
    assert (got[live & (coverage == 0)] == 0).all()
    # rgb an ulp below the backdrop: a negative foreground, byte 0
    below = live & (coverage > 0) & (rgb < backdrop).all(axis=-1)
    if frame != "1x1":
        for mask in (nan_a, below, live & (coverage == 1), live & (coverage == F32(1) / F32(5)), ~live, np.isinf(rgb).any(axis=-1) & live,
                     np.isnan(rgb).any(axis=-1) & live):
            assert mask.sum() >= 3
    assert below.any() and (got[below][:, :3] == 0).all()
    # a NaN component ends as byte 0
    nan_c = np.isnan(rgb) & live[..., None] & (coverage > 0)[..., None]
    assert (got[..., :3][nan_c] == 0).all()


@pytest.mark.parametrize("srgb", [True, False])
def test_opaque_pixels_over_no_backdrop_carry_the_display_bytes(srgb):
    rgb, backdrop, coverage, ns = rgba_edge_frames()["33x35"]
    opaque = (coverage == 1) & (backdrop == 0).all(axis=-1) & (ns != 0)
    assert opaque.sum() >= 50
    got = hip.matte_rgba_host(rgb, backdrop, coverage, ns, srgb)
    disp = hip.display_host(rgb, np.ones(ns.shape, F32), ns, 5, srgb).color.reshape(rgb.shape)
    assert np.array_equal(got[..., :3][opaque], disp[opaque])
    assert (got[..., 3][opaque] == 255).all()


def test_arguments_are_checked_before_the_library_is_called():
    with pytest.raises(ValueError):
        hip.matte_accumulate_host(np.zeros((3, 3), F32), np.zeros((2, 3), F32), np.zeros(3, bool))
    with pytest.raises(ValueError):
        hip.matte_rgba_host(np.zeros((2, 2, 3), F32), np.zeros((2, 2, 3), F32), np.zeros((2, 2), F32), np.zeros((2, 3), np.uint32))
    with pytest.raises(ValueError):
        hip.matte_rgba_host(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, np.uint32))
    L = hip.lib()
    z = np.zeros(12, F32)
    assert L.qa_test_matte_rgba_host(None, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, 1, z.ctypes.data) == -1      # QA_EINVAL
    assert L.qa_test_matte_rgba_host(z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0, 1, z.ctypes.data) == -1
    assert L.qa_test_matte_accumulate_host(None, z.ctypes.data, z.ctypes.data, 2, z.ctypes.data, None, None, None) == -1


def test_header_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/matte_check.cpp: the header's host half over edge frames in heap buffers of exactly their size, stand-alone under
    ASan / UBSan (nothing is loaded into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "matte_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "matte_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "matte_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
