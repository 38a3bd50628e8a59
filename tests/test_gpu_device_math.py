"""The device build of qa_device_math.h and of the sphere's texture coordinates against the host build of the same source,
bit for bit, on the MI355X.  tests/test_device_math.py pins the host build to glibc (the oracle's libm), so together they
pin every transcendental the kernels call: powf, expf, asinf (qa_device_math.h), and the double atan2 / asin of
sphereU / sphereV (qa_texture_dev.h: OCML's on the device, glibc's on the host).  sinf / cosf: test_gpu_parity.py.
For a NaN input the output must be a NaN; the payload is not compared."""
import ctypes as C

import numpy as np
import pytest

from test_device_math import same_bits, sphere_points

pytestmark = pytest.mark.gpu


def _both(fn, x, y=None):
    from qaray_amd import hip
    L = hip.lib()
    for f in (L.qa_test_math_device, L.qa_test_math_host):
        f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, np.float32)
    d, h = np.zeros_like(x), np.zeros_like(x)
    assert L.qa_test_math_device(fn, x.ctypes.data, y.ctypes.data, x.size, d.ctypes.data) == 0, L.qa_last_error()
    assert L.qa_test_math_host(fn, x.ctypes.data, y.ctypes.data, x.size, h.ctypes.data) == 0
    return d, h


def _mismatches(d, h):
    return int(np.count_nonzero(~((d.view(np.uint32) == h.view(np.uint32)) | (np.isnan(d) & np.isnan(h)))))


def _f(*hexes):
    return np.array([float.fromhex(v) if isinstance(v, str) else v for v in hexes], np.float32)


DENORMALS = _f("0x1p-149", "-0x1p-149", "0x1.fffffcp-127", "-0x1.fffffcp-127", "0x1p-140", "-0x1p-130")
SPECIAL = np.concatenate([_f(0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, -np.nan), DENORMALS])
# expf: the overflow threshold 0x1.62e42ep6 and the underflow / subnormal-result bounds (original special cases at |x| >= 88)
EXP_EDGES = np.concatenate([SPECIAL, _f("0x1.62e42ep6", "0x1.62e430p6", "-0x1.9fe368p6", "-0x1.9fe36ap6", "-0x1.5d589ep6", "-0x1.5d58a0p6",
                                        88.0, -88.0, 2.0 ** -24, -2.0 ** -24, 100.0, -104.0, -150.0)])


def test_powf_device_equals_host():
    """tools/gpu_math.py's ranges (glossy exponents on (0,1), (0,8)^(-50,250), bases near 1) plus the edges of both arguments."""
    rng = np.random.default_rng(1)
    n = 1 << 20
    cases = [(rng.random(n, dtype=np.float32), rng.choice(np.array([2, 5, 10, 20, 50, 80, 100, 0.5, 1], np.float32), n)),
             (rng.random(n, dtype=np.float32) * 8, rng.random(n, dtype=np.float32) * 300 - 50),
             (np.float32(1) + (rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(1e-5), np.full(n, 80, np.float32))]
    bases = np.concatenate([SPECIAL, _f(0.5, 2.0, 2.0 ** -126, 2.0 ** 127, 3.4028235e38, 0.99999994, 1.0000001)])
    exps = np.concatenate([SPECIAL, _f(0.5, 2.0, 80.0, -50.0, 126.0, 150.0, 1e10, -1e10)])
    bx, ey = np.meshgrid(bases, exps)
    cases.append((bx.ravel(), ey.ravel()))
    # overflow / underflow of the result: y*log2(x) just around +128 and -150
    x = rng.random(1 << 16, dtype=np.float32) * 7 + np.float32(1.01)
    y = (np.float32(128) / np.log2(x)).astype(np.float32)
    cases.append((np.concatenate([x, x, x, x]), np.concatenate([y, np.nextafter(y, np.float32(0)), -y * np.float32(150 / 128), -y])))
    for x, y in cases:
        d, h = _both(2, x, y)
        assert _mismatches(d, h) == 0


def test_expf_device_equals_host():
    rng = np.random.default_rng(2)
    n = 1 << 20
    for x in (rng.random(n, dtype=np.float32) * 200 - 100, -rng.random(n, dtype=np.float32), EXP_EDGES,
              # every float bit pattern of a stride: all exponents, both signs, NaNs and infinities
              np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32)):
        d, h = _both(3, x)
        assert _mismatches(d, h) == 0


def test_asinf_device_equals_host():
    """A strided sweep of every float in [-1, 1] (each 61st bit pattern of either sign, and 1.0), the edges and the NaN inputs."""
    pos = np.arange(0, 0x3f800001, 61, dtype=np.uint32)
    pos = np.append(pos, np.uint32(0x3f800000))
    x = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)
    d, h = _both(4, x)
    assert _mismatches(d, h) == 0
    d, h = _both(4, np.concatenate([SPECIAL, _f(1.0000001, -1.5, 0.975, 0.97499996, 0.5, 0.49999997, 2.0 ** -27, "0x1.fffffep-28")]))
    assert _mismatches(d, h) == 0
    assert np.isnan(d[np.isnan(SPECIAL).nonzero()[0]]).all()


def test_sphere_texcoords_device_equal_host():
    """Dense random points on spheres (unit and offset-ray hit points), the poles, and the seam at atan2 = +-pi."""
    px, py, pz, rcp_l = sphere_points(1 << 20, 3)
    du, hu = _both(5, px, py)
    dv, hv = _both(6, pz, rcp_l)
    bad_u, bad_v = _mismatches(du, hu), _mismatches(dv, hv)
    assert (bad_u, bad_v) == (0, 0), f"u: {bad_u}, v: {bad_v} of {px.size} differ"
    assert same_bits(du, hu) and same_bits(dv, hv)
