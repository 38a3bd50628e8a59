"""Ambient occlusion on the CPU: the host build of qaray_amd/csrc/hip/qa_ao_dev.h (hip.ao_directions_host, hip.ao_face_normal_host and
the two hooks of the generator's inner steps: the source the kernels of qa_ao.hip are compiled from) against the float32 numpy
restatement of the header's opening comment in tests/ao_util.py, bit for bit; the distribution of the directions against the exact
moments of a cosine-weighted direction; tests/cpp/ao_check.cpp runs the same functions stand-alone under AddressSanitizer + UBSan on
buffers of exactly the sizes it is given."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ao_util import F32, bits, direction_from_ref, directions_ref, face_normal_ref, key_of, ray_key, sphere_ref
from qaray_amd import hip

M = 65536
SEEDS = (0x51A7A7, 0, 0xFFFFFFFF)


def unit_normals():
    """The three axes, (0.6, 0, -0.8), (1, 1, 1) / sqrt 3 and 64 random unit normals -> float32 (69, 3)"""
    rng = np.random.default_rng(20261)
    r = rng.standard_normal((64, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    fixed = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0.6, 0, -0.8), tuple(np.ones(3) / np.sqrt(3.0))]
    return np.concatenate([np.float64(fixed), r]).astype(F32)


NORMALS = unit_normals()


def pairs(k):
    """65 536 (stream, c) pairs of normal k: random words, with counters next to 2^32 - 1 and streams next to both ends among them"""
    rng = np.random.default_rng(1000 + k)
    stream = rng.integers(0, 2 ** 32, M, dtype=np.uint64).astype(np.uint32)
    c = rng.integers(0, 2 ** 32, M, dtype=np.uint64).astype(np.uint32)
    c[:64] = np.uint32(0xFFFFFFFF) - np.arange(64, dtype=np.uint32)
    c[64:128] = np.arange(64, dtype=np.uint32)
    stream[128:160] = np.arange(32, dtype=np.uint32)
    stream[160:192] = np.uint32(0xFFFFFFFF) - np.arange(32, dtype=np.uint32)
    return stream, c


@pytest.fixture(scope="module")
def draws():
    """The hook's directions for every normal at the default seed, made once: normal k -> float32 (M, 3)"""
    return [hip.ao_directions_host(SEEDS[0], *pairs(k), NORMALS[k]) for k in range(len(NORMALS))]


def test_directions_bit_for_bit(draws):
    for k, n in enumerate(NORMALS):
        stream, c = pairs(k)
        assert np.array_equal(bits(draws[k]), bits(directions_ref(SEEDS[0], stream, c, n))), f"normal {k} {n}"
    for seed in SEEDS[1:]:
        for k in (0, 3, 4, 17):
            stream, c = pairs(k)
            assert np.array_equal(bits(hip.ao_directions_host(seed, stream, c, NORMALS[k])), bits(directions_ref(seed, stream, c, NORMALS[k]))), (seed, k)
    # a normal per record
    stream, c = pairs(5)
    n = NORMALS[np.arange(M) % len(NORMALS)]
    assert np.array_equal(bits(hip.ao_directions_host(7, stream, c, n)), bits(directions_ref(7, stream, c, n)))
    assert hip.ao_directions_host(7, [], [], np.zeros((0, 3), F32)).shape == (0, 3)


DOWN = F32([0, 0, -1])


@pytest.fixture(scope="module")
def search():
    """One pass of the restatement over the 2^24 counters of stream 0 -> (the counters whose eight attempts all fail, the counters
    whose sphere point lies within l2 <= 1e-6 of the point opposite the normal (0, 0, -1))"""
    total, chunk = 1 << 24, 1 << 20
    key = key_of(SEEDS[0], np.zeros(1, np.uint32))
    fallback, short = [], []
    for lo in range(0, total, chunk):
        c = np.arange(lo, lo + chunk, dtype=np.uint32)
        s, fb, _ = sphere_ref(ray_key(key, c))
        fallback.append(c[fb])
        v = (DOWN + s).astype(F32)
        l2 = ((v[:, 0] * v[:, 0]).astype(F32) + (v[:, 1] * v[:, 1]).astype(F32)).astype(F32) + (v[:, 2] * v[:, 2]).astype(F32)
        short.append(c[l2 <= F32(1e-6)])
    return np.concatenate(fallback), np.concatenate(short)


def test_sphere_points_and_the_fallback_branch(search):
    """The inner step against the restatement, and the counters of 2^24 of one stream whose eight attempts all fail (about 4.5e-6 of
    them: some 75 expected); their directions are n + (0, 0, 1), normalised."""
    seed, chunk = SEEDS[0], 1 << 18
    found = search[0]
    print(f"fallback: {len(found)} of 2^24 counters take it")
    # the hook over a run of counters in full, and over every counter found
    c = np.arange(chunk, dtype=np.uint32)
    s_ref, fb_ref, taken = sphere_ref(ray_key(key_of(seed, np.zeros(1, np.uint32)), c))
    s, fb = hip.ao_sphere_host(seed, np.zeros(chunk, np.uint32), c)
    assert np.array_equal(bits(s), bits(s_ref)) and np.array_equal(fb, fb_ref)
    assert 0.20 < np.mean(taken > 0) < 0.23   # (1 - pi / 4 of the draws need a second attempt)
    if len(found):
        s, fb = hip.ao_sphere_host(seed, np.zeros(len(found), np.uint32), found)
        assert fb.all() and np.array_equal(s, np.tile(F32([0, 0, 1]), (len(found), 1)))
        for n in NORMALS[:5]:
            d = hip.ao_directions_host(seed, np.zeros(len(found), np.uint32), found, n)
            assert np.array_equal(bits(d), bits(direction_from_ref(n, s)))
            assert np.array_equal(bits(d), bits(directions_ref(seed, np.zeros(len(found), np.uint32), found, n)))
    else:
        print("no counter of 2^24 takes the fallback: the branch is checked through the hook that takes s directly")
    # the branch through the hook that takes s directly, whatever the search found
    s = np.tile(F32([0, 0, 1]), (len(NORMALS), 1))
    assert np.array_equal(bits(hip.ao_direction_from_host(NORMALS, s)), bits(direction_from_ref(NORMALS, s)))


def test_short_sum_branch(search):
    """l2 <= 1e-6: the sphere point opposite the normal.  About 2.5e-7 of the draws of a normal reach it (and, about (0, 0, -1), the
    counters that take the fallback, whose point (0, 0, 1) is the opposite one), so a search of 2^24 counters may find none; the test
    says which, and checks the branch through the hook that takes s directly in either case."""
    seed, n, found = SEEDS[0], DOWN, search[1]
    print(f"l2 <= 1e-6: {len(found)} of 2^24 counters reach it about {n}")
    if len(found):
        d = hip.ao_directions_host(seed, np.zeros(len(found), np.uint32), found, n)
        assert np.array_equal(bits(d), bits(np.tile(n, (len(found), 1))))
    else:
        print("no counter of 2^24 reaches l2 <= 1e-6: the branch is checked through the hook that takes s directly")
    # s = -n exactly, s an ulp or a thousandth off it, and the threshold's two sides
    rows_n, rows_s = [], []
    for k, nn in enumerate(NORMALS):
        for off in (0.0, 1e-7, 4e-4, 9.9e-4, 1.01e-3, 2e-3):
            t = np.cross(nn.astype(np.float64), [0.3, -0.5, 0.8])
            t /= np.linalg.norm(t)
            rows_n.append(nn)
            rows_s.append((-nn.astype(np.float64) + off * t).astype(F32))
    rows_n, rows_s = F32(rows_n), F32(rows_s)
    got, ref = hip.ao_direction_from_host(rows_n, rows_s), direction_from_ref(rows_n, rows_s)
    assert np.array_equal(bits(got), bits(ref))
    exact = np.arange(0, len(rows_n), 6)
    assert np.array_equal(bits(got[exact]), bits(rows_n[exact]))          # d = n
    assert not np.array_equal(bits(got[exact + 5]), bits(rows_n[exact + 5]))


def test_face_normal_bit_for_bit():
    rng = np.random.default_rng(5)
    N = rng.standard_normal((4096, 3)).astype(F32)
    d = rng.standard_normal((4096, 3)).astype(F32)
    N[:3] = np.eye(3, dtype=F32)
    d[:3] = F32([[0, 1, 0], [0, 0, 1], [1, 0, 0]])      # perpendicular: the dot is 0, N stays
    N[3], d[3] = F32([0, 0, 0]), F32([1, 2, 3])        # a zero normal stays +0
    N[4], d[4] = F32([0, 0, 1]), F32([0, 0, 1])        # along the ray: turned
    N[5], d[5] = F32([0, 0, 1]), F32([0, 0, -1])
    got = hip.ao_face_normal_host(N, d)
    assert np.array_equal(bits(got), bits(face_normal_ref(N, d)))
    assert np.array_equal(bits(got[:4]), bits(N[:4])) and np.array_equal(got[4], F32([0, 0, -1])) and np.array_equal(got[5], N[5])
    dots = (got.astype(np.float64) * d).sum(axis=1)
    assert (dots <= 1e-6).all()


def test_distribution(draws):
    """Five standard errors of the exact moments of a cosine-weighted direction at M draws: E[d.n] = 2/3 (variance 1/18),
    E[(d.n)^2] = 1/2 (variance 1/12), each tangential component mean 0 (variance 1/4)."""
    assert M == 65536
    for k, n in enumerate(NORMALS):
        d = draws[k].astype(np.float64)
        nn = n.astype(np.float64)
        cos = d @ nn
        a = np.cross(nn, [1.0, 0, 0] if abs(nn[0]) < 0.9 else [0, 1.0, 0])
        a /= np.linalg.norm(a)
        b = np.cross(nn, a)
        print(f"normal {k}: mean d.n {cos.mean():.5f}, mean (d.n)^2 {(cos ** 2).mean():.5f}, tangential means {(d @ a).mean():+.5f} {(d @ b).mean():+.5f}, "
              f"min d.n {cos.min():.3e}, length error {np.abs(np.linalg.norm(d, axis=1) - 1).max():.2e}")
        assert abs(cos.mean() - 2.0 / 3.0) < 0.0046, k
        assert abs((cos ** 2).mean() - 0.5) < 0.0057, k
        assert abs((d @ a).mean()) < 0.0098 and abs((d @ b).mean()) < 0.0098, k
        assert (cos >= 0).all(), k
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 4e-7, k


def test_key_determinism(draws):
    """The direction of (seed, stream, c) does not depend on its place in the batch; other streams and other seeds give other sets."""
    k = 4
    stream, c = pairs(k)
    perm = np.random.default_rng(9).permutation(M)
    shuffled = hip.ao_directions_host(SEEDS[0], stream[perm], c[perm], NORMALS[k])
    assert np.array_equal(bits(shuffled), bits(draws[k][perm]))
    alone = hip.ao_directions_host(SEEDS[0], stream[77:78], c[77:78], NORMALS[k])
    assert np.array_equal(bits(alone[0]), bits(draws[k][77]))
    c = np.arange(4096, dtype=np.uint32)
    base = hip.ao_directions_host(SEEDS[0], np.full(4096, 5, np.uint32), c, NORMALS[k])
    other_stream = hip.ao_directions_host(SEEDS[0], np.full(4096, 6, np.uint32), c, NORMALS[k])
    other_seed = hip.ao_directions_host(SEEDS[0] + 1, np.full(4096, 5, np.uint32), c, NORMALS[k])
    assert (bits(base) != bits(other_stream)).any(axis=1).mean() > 0.99
    assert (bits(base) != bits(other_seed)).any(axis=1).mean() > 0.99
    assert len(np.unique(bits(base), axis=0)) == 4096   # and the counters of one stream differ among themselves


def test_hooks_refuse_bad_arguments():
    with pytest.raises(ValueError):
        hip.ao_directions_host(1, np.zeros(3, np.uint32), np.zeros(4, np.uint32), NORMALS[0])
    with pytest.raises(ValueError):
        hip.ao_directions_host(1, np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros((2, 3), F32))
    with pytest.raises(ValueError):
        hip.ao_face_normal_host(np.zeros((3, 3), F32), np.zeros((2, 3), F32))
    L = hip.lib()
    z = np.zeros(12, F32)
    assert L.qa_test_ao_directions_host(1, None, z.ctypes.data, z.ctypes.data, 1, z.ctypes.data) == -1      # QA_EINVAL
    assert L.qa_test_ao_directions_host(1, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, None) == -1
    assert L.qa_test_ao_face_normal_host(z.ctypes.data, None, 1, z.ctypes.data) == -1
    assert L.qa_test_ao_sphere_host(1, z.ctypes.data, z.ctypes.data, 1, None, None) == -1
    assert L.qa_test_ao_direction_from_host(z.ctypes.data, None, 1, z.ctypes.data) == -1
    assert L.qa_test_ao_directions_host(1, None, None, None, 0, None) == 0


def test_planes_and_constants():
    assert hip.AO_PLANES == ("open", "rays", "ao") and hip.QA_AO_MAX_RAYS == 256


def test_header_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/ao_check.cpp: the header's host half on heap buffers of exactly their size, stand-alone under ASan / UBSan (nothing
    is loaded into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "ao_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "ao_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ao_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
