"""qa_device_math.h compiled for the host (same source as the device code) against glibc.
sinf/cosf restate glibc's algorithm and must return its bits on [0, 2*pi] - the only range the
integrator uses (phi = 2*pi*r, r in [0,1]).  expf/powf restate glibc's table-driven algorithms
(including where its x86-64 FMA build fuses) and asinf its fp32 polynomial routine; all must return
its bits too: tests/cpp/math_exhaustive.c sweeps them against the host libm (the full sweeps - every
float for expf, every float in [-1, 1] for asinf - pass; the suite runs strided ones).  The sphere's
texture coordinates (qa_texture_dev.h sphereU / sphereV) must equal the oracle's expressions.
tests/test_gpu_device_math.py pins the device build of the same source to this host build."""
import ctypes as C
import os
import subprocess

import numpy as np

from qaray_amd import hip


def _host(fn, x, y=None):
    L = hip.lib()
    L.qa_test_math_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    out = np.zeros_like(x)
    rc = L.qa_test_math_host(fn, x.ctypes.data, y.ctypes.data if y is not None else None, x.size, out.ctypes.data)
    assert rc == 0
    return out


def _libm(name, x, y=None):
    libm = C.CDLL("libm.so.6")
    f = getattr(libm, name)
    f.restype = C.c_float
    f.argtypes = [C.c_float] * (2 if y is not None else 1)
    if y is None:
        return np.array([f(float(v)) for v in x], np.float32)
    return np.array([f(float(a), float(b)) for a, b in zip(x, y)], np.float32)


def test_sincos_bit_exact_on_integrator_range():
    rng = np.random.default_rng(5)
    # every float in a few exponent ranges is too slow from python; sample densely instead:
    x = np.concatenate([
        rng.random(120000, dtype=np.float32) * np.float32(6.2831855),
        np.linspace(0, 6.2831855, 60000, dtype=np.float32),
        np.float32(2 * np.pi) * (np.float32(1.0) - rng.random(20000, dtype=np.float32) ** 8),   # near 2*pi
        rng.random(20000, dtype=np.float32) ** 8 * np.float32(1e-2),                              # near 0
        np.array([0.0, 6.2831855, np.pi, np.pi / 2, np.pi / 4, 0.75, 0.7853982, 2.0 ** -12, 2.0 ** -13], np.float32)])
    assert np.array_equal(_host(0, x).view(np.uint32), _libm("sinf", x).view(np.uint32))
    assert np.array_equal(_host(1, x).view(np.uint32), _libm("cosf", x).view(np.uint32))


def test_powf_expf_bit_exact():
    rng = np.random.default_rng(6)
    x = rng.random(40000, dtype=np.float32)
    y = rng.choice(np.array([2, 5, 10, 20, 50, 100, 1, 0, 80, 0.5], np.float32), 40000)
    assert np.array_equal(_host(2, x, y).view(np.uint32), _libm("powf", x, y).view(np.uint32))
    xe = -rng.random(40000, dtype=np.float32) * np.float32(50)
    assert np.array_equal(_host(3, xe).view(np.uint32), _libm("expf", xe).view(np.uint32))
    # edge cases the shading code relies on
    e = _host(2, np.array([0, 0, 1, 0.5], np.float32), np.array([5, 0, 7, 0], np.float32))
    assert e.tolist() == [0.0, 1.0, 1.0, 1.0]


def _math_exhaustive(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "math_exhaustive")
    subprocess.run(["gcc", "-O2", "-fopenmp", os.path.join(root, "tests", "cpp", "math_exhaustive.c"), "-o", exe, "-ldl", "-lm"],
                   check=True)
    return exe


def test_powf_expf_strided_sweep(tmp_path):
    """expf over every 16th block of 65536 float bit patterns (incl. NaN / inf / overflow ranges), powf over
    positive bases below 2 x 17 exponents plus random pairs - hundreds of millions of comparisons."""
    exe = _math_exhaustive(tmp_path)
    for mode in ("0", "1"):
        r = subprocess.run([exe, hip.HIP_LIB_PATH, mode, "16"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert " 0 mismatches" in r.stdout


def test_asinf_strided_sweep(tmp_path):
    """asinf over every 16th block of 65536 float bit patterns in [-1, 1], either sign (1.3e8 comparisons; stride 1,
    every float, passes too).  A correctly rounded (float) asin((double) x) fails it: glibc's asinf is not correctly rounded."""
    exe = _math_exhaustive(tmp_path)
    r = subprocess.run([exe, hip.HIP_LIB_PATH, "2", "16"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout


def test_asinf_bit_exact_at_its_branch_points():
    """Both signs around every branch of the routine (2^-27, 0.5, 0.975, 1), +-0, out of range, and where a correctly
    rounded asin differs from glibc's (e.g. 0x1.d12e9ep-12, the smallest such input)."""
    rng = np.random.default_rng(7)
    edges = np.array([0.0, 2.0 ** -27, 0.5, 0.975, 1.0, float.fromhex("0x1.d12e9ep-12"), float.fromhex("0x1.fffcd4p-1")], np.float32)
    near = (edges.view(np.uint32)[:, None] + np.arange(-40, 41, dtype=np.int64)[None, :]).clip(0, 0x3f800000).astype(np.uint32)
    x = np.concatenate([near.ravel().view(np.float32), rng.random(100000, dtype=np.float32),
                        rng.random(20000, dtype=np.float32) ** 12])
    x = np.concatenate([x, -x])
    assert np.array_equal(_host(4, x).view(np.uint32), _libm("asinf", x).view(np.uint32))
    out = _host(4, np.array([1.0000001, -1.5, np.inf, np.nan], np.float32))
    assert np.isnan(out).all()


def _sphere_uv_oracle(px, py, pz, rcp_l):
    """oracle/qa_oracle.c sphere_texcoord: (float) (0.5f - atan2(p.x, p.y) * kRCP_2PI), (float) (0.5f + asin(p.z * rcp_l) * kRCP_PI)
    in C double with libm's atan2 / asin; kRCP_* are the float constants 1.f / (2.f * (float) M_PI), 1.f / (float) M_PI."""
    libm = C.CDLL("libm.so.6")
    libm.atan2.restype = libm.asin.restype = C.c_double
    libm.atan2.argtypes = [C.c_double, C.c_double]
    libm.asin.argtypes = [C.c_double]
    pi = np.float32(np.pi)
    k2, k1 = float(np.float32(1) / (np.float32(2) * pi)), float(np.float32(1) / pi)
    zr = (pz * rcp_l).astype(np.float32)
    u = np.array([0.5 - libm.atan2(float(a), float(b)) * k2 for a, b in zip(px, py)], np.float32)
    v = np.array([0.5 + libm.asin(float(z)) * k1 for z in zr], np.float32)
    return u, v


def sphere_points(n, seed):
    """Points on spheres (radius 1, and the unnormalised hit points of the differentials' offset rays), the poles, and the
    seam of atan2 = +-pi (p.x = +-0 or tiny, p.y < 0): -> px, py, pz, rcp_l (float32)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    radius = rng.choice([1.0, 1.0, 0.37, 2.5], n)
    p = (d * radius[:, None]).astype(np.float32)
    seam = np.zeros((64, 3), np.float32)
    seam[:, 0] = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 1e-45, -1e-45] * 8, np.float32)
    seam[:, 1] = -np.sqrt(1 - np.linspace(-0.99, 0.99, 64) ** 2).astype(np.float32)
    seam[:, 2] = np.linspace(-0.99, 0.99, 64).astype(np.float32)
    poles = np.array([[0, 0, 1], [0, 0, -1], [-0.0, 0, 1], [0, -0.0, -1], [1e-7, 1e-7, 1], [-1e-7, 1e-7, -1], [0, 1e-20, 1],
                      [0, 0, 0.99999994], [0, 0, -0.99999994]], np.float32)
    p = np.concatenate([p, seam, poles])
    length = np.sqrt((p.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)).astype(np.float32)
    rcp_l = (np.float32(1) / length).astype(np.float32)
    unit = np.concatenate([radius == 1.0, np.ones(len(seam) + len(poles), bool)])
    rcp_l[unit & (np.arange(len(p)) % 2 == 0)] = np.float32(1)   # sphereTexCoord(p, 1.f): the hit point on the unit sphere itself
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), rcp_l


def same_bits(a, b):
    """Bit-equal, except that any NaN equals any NaN (payloads are not compared)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_sphere_texcoord_helpers_equal_the_oracle_expressions():
    px, py, pz, rcp_l = sphere_points(60000, 8)
    u, v = _sphere_uv_oracle(px, py, pz, rcp_l)
    assert same_bits(_host(5, px, py), u)
    assert same_bits(_host(6, pz, rcp_l), v)
    assert np.isfinite(u).all()

