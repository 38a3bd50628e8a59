"""What the denoiser's tests share: a float64 numpy restatement of the filter, written from the specification in the opening comment
of qaray_amd/csrc/hip/qa_denoise_dev.h (not from its code: whole-frame array operations, float64 throughout), and the frames the
host and the device tests run."""
import numpy as np

MISS = np.float32(1.0e30)
VOID, MISS_CLASS, HIT = 0, 1, 2
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
EPS_L = float(np.float32(1e-4))
SLOPE_FLOOR = float(np.float32(1e-3))


def classes(rgb, depth, ns):
    finite = np.isfinite(rgb).all(axis=2) & np.isfinite(depth)
    cls = np.where(depth == MISS, MISS_CLASS, HIT)
    return np.where((ns == 0) | ~finite, VOID, cls)


def luma(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _shift(a, dx, dy, fill=0):
    """a at p + (dx, dy) for every pixel p, and whether that pixel lies in the image."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ok = np.zeros((h, w), bool)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dx) < w and abs(dy) < h:
        out[yd, xd] = a[ys, xs]
        ok[yd, xd] = True
    return out, ok


def denoise_ref(rgb, depth, ns, iterations=5, sigma_color=4.0, sigma_depth=1.0):
    """-> float64 (h, w, 3); void pixels carry their input values."""
    rgb32 = np.asarray(rgb, np.float32)
    cls = classes(rgb32, np.asarray(depth, np.float32), np.asarray(ns))
    live = cls != VOID
    c = np.where(live[..., None], rgb32.astype(np.float64), 0.0)
    z = np.where(live, np.asarray(depth, np.float64), 0.0)
    if iterations == 0:
        return rgb32.astype(np.float64)
    # pass 0: the variance of the luma over the 3x3 window's members, the slope of the depth
    l = luma(c)
    members = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, ok = _shift(l, dx, dy)
            cq, _ = _shift(cls, dx, dy)
            members.append((lq, ok & live & (cq == cls)))
    n = sum(m.astype(np.float64) for _, m in members)
    mean = sum(np.where(m, lq, 0.0) for lq, m in members) / np.maximum(n, 1)
    var = sum(np.where(m, (lq - mean) ** 2, 0.0) for lq, m in members) / np.maximum(n, 1)
    var = np.where(n > 1, var, 0.0)
    hit = cls == HIT
    slope = np.zeros_like(z)
    for axis in (0, 1):
        d = []
        for side in (-1, 1):
            zq, ok = _shift(z, side if axis == 0 else 0, side if axis == 1 else 0)
            hq, _ = _shift(hit, side if axis == 0 else 0, side if axis == 1 else 0, False)
            d.append((np.abs(z - zq), ok & hq))
        (d0, m0), (d1, m1) = d
        slope = np.maximum(slope, np.where(m0 & m1, np.minimum(d0, d1), np.where(m0, d0, np.where(m1, d1, 0.0))))
    slope = np.where(hit, np.maximum(slope, SLOPE_FLOOR * np.abs(z)), 0.0)
    # the iterations
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(iterations):
            s = 1 << i
            lp = luma(c)
            den_l = sigma_color * np.sqrt(var) + EPS_L
            den_z = sigma_depth * slope * s
            sw = np.zeros_like(lp)
            sc = np.zeros_like(c)
            sv = np.zeros_like(lp)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        sw += 9.0 / 64
                        sv += (9.0 / 64) ** 2 * var
                        continue
                    cq, ok = _shift(c, s * dx, s * dy)
                    vq, _ = _shift(var, s * dx, s * dy)
                    zq, _ = _shift(z, s * dx, s * dy)
                    kq, _ = _shift(cls, s * dx, s * dy)
                    ok = ok & live & (kq == cls)
                    e = np.abs(lp - luma(cq)) / den_l
                    dz = np.abs(z - zq)
                    e = e + np.where(hit & (dz != 0), dz / (den_z * max(abs(dx), abs(dy))), 0.0)
                    w = np.where(ok, H5[dx + 2] * H5[dy + 2] * np.exp(-e), 0.0)
                    sw += w
                    sc += w[..., None] * (cq - c)
                    sv += w * w * vq
            c = np.where(live[..., None], c + sc / sw[..., None], 0.0)
            var = np.where(live, sv / (sw * sw), 0.0)
    return np.where(live[..., None], c, rgb32.astype(np.float64))


def random_frame(w, h, seed, void=True):
    """A frame of w x h pixels with hit, miss and void pixels mixed: colours in [0, 2), hit depths on a bumpy slanted plane, a
    quarter of the pixels missing the scene, and - when asked for - some pixels skipped (ns 0), NaN or infinite."""
    r = np.random.default_rng(seed)
    rgb = (r.random((h, w, 3)) * 2).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    depth = (3 + 0.2 * x + 0.1 * y + r.random((h, w))).astype(np.float32)
    depth[r.random((h, w)) < 0.25] = MISS
    ns = r.integers(1, 9, (h, w)).astype(np.uint32)
    if void:
        k = r.random((h, w))
        ns[k < 0.08] = 0
        rgb[(k >= 0.08) & (k < 0.12), 1] = np.nan
        rgb[(k >= 0.12) & (k < 0.16), 2] = np.inf
    return rgb, depth, ns


HOST_SIZES = ((1, 1), (9, 1), (1, 9), (7, 5), (33, 17))   # (w, h)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
