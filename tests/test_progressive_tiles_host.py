"""The per-tile error map and the noisiest-first selection of progressive frames on the CPU: qa_test_tile_error_host and
qa_test_tile_select_host run qaray_amd/csrc/hip/qa_prog_error_dev.h, the source the device kernels are compiled from, built for the
host.  Both are held bit for bit to the numpy restatements of that header's opening comment (tests/progressive_tiles_util.py);
tests/test_gpu_progressive_tiles.py holds the device build to this one."""
import numpy as np
import pytest

from progressive_tiles_util import tile_error_np, tile_select_np
from qaray_amd import hip

FIN = np.uint32(0x80000000)


def f2u(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def slab(w, h, seed):
    """A synthetic state slab: n in 0 .. 40, a fifth of the pixels finished, variances of every kind."""
    r = np.random.default_rng(seed)
    st = r.integers(0, 2 ** 32, (h, w, 8), dtype=np.uint64).astype(np.uint32)   # words 0, 2 .. 4: noise nobody may read
    n = r.integers(0, 41, (h, w)).astype(np.uint32)
    var = (r.random((h, w, 3)) * 0.05).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, 1e-39, 3e38, np.inf, np.nan, -1e-3, -np.inf, 1.0], np.float32)
    pick = r.random((h, w, 3)) < 0.08
    var[pick] = special[r.integers(0, len(special), int(pick.sum()))]
    st[..., 1] = n
    st[..., 5:8] = var.view(np.uint32)
    fin = r.random((h, w)) < 0.2
    st[fin, 0] = 0
    st[fin, 1] = FIN    # (as the kernels leave a finished pixel; the count is gone)
    return st


def check(st):
    got, want = hip.tile_error_host(st), tile_error_np(st)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(u32(got), u32(want)), np.argwhere(u32(got) != u32(want))
    assert not np.isnan(got).any() and (got >= 0).all() and not np.signbit(got).any()
    return got


@pytest.mark.parametrize("w,h", [(40, 28), (9, 9)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tile_error_host_equals_the_restatement(w, h, seed):
    st = slab(w, h, seed)
    got = check(st)
    assert got.shape == ((h + 7) // 8, (w + 7) // 8)


@pytest.mark.parametrize("w,h", [(40, 28), (9, 9)])
def test_tile_error_host_special_tiles(w, h):
    r = np.random.default_rng(7)
    st = slab(w, h, 11)
    st[..., 1] = r.integers(2, 41, (h, w)).astype(np.uint32)
    st[..., 5:8] = (r.random((h, w, 3)) * 0.05).astype(np.float32).view(np.uint32)
    plain = check(st)
    assert np.isfinite(plain).all() and (plain > 0).all()
    # a tile that is entirely finished: exactly +0; the last tile (an edge tile in both directions) too
    for ys, xs in ((slice(0, 8), slice(0, 8)), (slice(8 * ((h - 1) // 8), h), slice(8 * ((w - 1) // 8), w))):
        a = st.copy()
        a[ys, xs, 1] = FIN
        e = check(a)
        t = (ys.start // 8, xs.start // 8)
        assert u32(e)[t] == 0
        e[t] = plain[t]
        assert np.array_equal(u32(e), u32(plain))
    # a tile with a single live pixel: its v / 64, whatever the finished pixels' words say
    a = st.copy()
    a[0:8, 0:8, 1] = FIN
    a[0:8, 0:8, 5:8] = f2u(np.nan)
    a[3, 5, 1] = 10
    a[3, 5, 5:8] = f2u([0.25, 2.5, 0.125])
    e = check(a)
    assert e[0, 0] == np.float32(2.5) / np.float32(10) * np.float32(0.015625)
    # one pixel without an estimate spoils its tile alone: n = 0, n = 1, a NaN, an inf, a negative variance on top
    for word, value in ((1, 0), (1, 1), (6, f2u(np.nan)), (5, f2u(np.inf)), (7, f2u(-1.0))):
        a = st.copy()
        if word != 7:
            a[h - 1, w - 1, word] = value
        else:
            a[h - 1, w - 1, 5:8] = value
        e = check(a)
        assert np.isposinf(e[-1, -1]) and np.isfinite(e.ravel()[:-1]).all()
    # zero, denormal and huge variances stay finite; a sum that overflows is +inf
    a = st.copy()
    a[0:8, 0:8, 5:8] = f2u(0.0)
    a[0, 0, 5] = f2u(1e-44)
    a[8:16, 0:8, 5:8] = f2u(3e38)
    a[8:16, 0:8, 1] = 2
    e = check(a)
    assert 0 <= e[0, 0] < 1e-44 and np.isposinf(e[1, 0])
    a[8:16, 0:8, 1] = FIN
    a[8, 1, 1] = 2
    assert check(a)[1, 0] == np.float32(3e38) / np.float32(2) * np.float32(0.015625)


def select(error, levels, target, max_tiles=0, min_error=0.0):
    got, want = hip.tile_select_host(error, levels, target, max_tiles, min_error), tile_select_np(error, levels, target, max_tiles, min_error)
    assert np.array_equal(got[0], want[0]), (np.flatnonzero(got[0] != want[0]), max_tiles)
    assert got[1] == want[1], (got[1], want[1])
    return got


def test_tile_select_host_equals_a_stable_descending_argsort_cut():
    r = np.random.default_rng(5)
    n = 700
    values = np.array([0.0, 1e-45, 1e-39, 1e-12, 3e-7, 3.0000002e-7, 0.001, 0.5, 1.0, 7.5, 3e38], np.float32)
    error = values[r.integers(0, len(values), n)]            # heavy ties
    error[r.integers(0, n, 9)] = np.inf                      # several +inf
    error[100:140] = (r.random(40) * 1e-3).astype(np.float32)
    levels = r.choice(np.array([0, 4, 8, 16], np.uint32), n)
    cand = int(((levels < 8) & (error > 0)).sum())
    assert 100 < cand < n
    for k in (0, 1, 2, 9, 10, cand - 1, cand, cand + 1, 10 ** 6):
        mask, info = select(error, levels, 8, k)
        assert mask.sum() == info["selected"] == (cand if k == 0 else min(k, cand)) and info["candidates"] == cand
        assert not mask[levels >= 8].any() and not mask[error == 0].any()
    # exactly at a tie group's edges: the first, the last and one past the last of every group of equal errors
    e = error[(levels < 8) & (error > 0)]
    sizes = [int((e == v).sum()) for v in sorted(set(e.tolist()), reverse=True)]
    edge = np.cumsum(sizes)
    for k in sorted({int(x) for c in edge for x in (c - 1, c, c + 1) if 1 <= x <= cand}):
        select(error, levels, 8, k)
    # min_error: above some, above all finite ones (+inf still goes), above every error
    assert select(error, levels, 8, 0, 0.5)[1]["candidates"] == int(((levels < 8) & (error > 0.5)).sum())
    assert select(error, levels, 8, 5, 3.0e38)[0].sum() == min(5, int(((levels < 8) & np.isinf(error)).sum()))
    finite = np.where(np.isinf(error), np.float32(1.0), error)
    mask, info = select(finite, levels, 8, 0, 3.0e38)
    assert not mask.any() and info == {"selected": 0, "candidates": 0, "cut_bits": 0, "max_finite_bits": 0}
    # every level at the target already
    mask, info = select(error, np.full(n, 8, np.uint32), 8, 3)
    assert not mask.any() and info["candidates"] == 0
    # a NaN error is no candidate; all tiles equal: the first by index
    e2 = np.full(130, 0.25, np.float32)
    e2[7] = np.nan
    mask, _ = select(e2, np.zeros(130, np.uint32), 1, 20)
    assert np.array_equal(np.flatnonzero(mask), [t for t in range(21) if t != 7])
    # a 2-D map keeps its shape
    mask, _ = select(error[:60].reshape(6, 10), levels[:60].reshape(6, 10), 8, 4)
    assert mask.shape == (6, 10)


def test_selection_header_under_asan_ubsan(tmp_path):
    """qa_prog_error_dev.h compiles with g++ alone: tests/cpp/tile_select_check.cpp runs its host half under ASan / UBSan on
    buffers of exactly the sizes it is given (selection against a stable sort, error maps with edge tiles)."""
    import os
    import subprocess
    from conftest import ROOT
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "tile_select_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "tile_select_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "tile_select_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]


def test_arguments_are_checked_before_the_library_is_called():
    with pytest.raises(ValueError):
        hip.tile_error_host(np.zeros((8, 8, 7), np.uint32))
    with pytest.raises(ValueError):
        hip.tile_error_host(np.zeros((8, 8, 8), np.float32))
    with pytest.raises(ValueError):
        hip.tile_select_host(np.zeros(4, np.float32), np.zeros(5, np.uint32), 1)
    with pytest.raises(ValueError):
        hip.tile_select_host(np.zeros(4, np.float32), np.zeros(4, np.uint32), 1, min_error=-1.0)
    with pytest.raises(ValueError):
        hip.tile_select_host(np.zeros(4, np.float32), np.zeros(4, np.uint32), 1, min_error=float("nan"))
    L = hip.lib()
    z = np.zeros(8, np.uint32)
    assert L.qa_test_tile_error_host(None, 1, 1, z.ctypes.data) == -1      # QA_EINVAL
    assert L.qa_test_tile_error_host(z.ctypes.data, 0, 1, z.ctypes.data) == -1
    assert L.qa_test_tile_select_host(None, z.ctypes.data, 1, 1, 0, 0.0, z.ctypes.data, None) == -1
