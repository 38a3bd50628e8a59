"""What the guided denoiser's tests share: a float64 numpy restatement of the GUIDED FORM section of the opening comment of
qaray_amd/csrc/hip/qa_denoise_dev.h (written from that text, not from its code: whole-frame array operations, float64
throughout), and the frames the host and the device tests run."""
import numpy as np

from denoise_util import EPS_L, H5, HIT, MISS, SLOPE_FLOOR, VOID, _shift, bits, classes, luma, random_frame  # noqa: F401

GUIDE_NORMAL, GUIDE_ALBEDO = 1, 2
RELIABLE_N = float(np.float32(0.02))
RELIABLE_A = float(np.float32(0.3))
SIGMA_A = float(np.float32(0.02))
MISS_CLASS = 1


def guide_bits(cls, normal, albedo):
    """-> (n, valid_n, a, valid_a, reliable) of the GUIDED FORM: float64 guides (0 where not valid) and boolean planes."""
    h, w = cls.shape
    live = cls != VOID
    if normal is None:
        n, vn = np.zeros((h, w, 3)), np.zeros((h, w), bool)
    else:
        n32 = np.asarray(normal, np.float32)
        fin = np.isfinite(n32).all(axis=2)
        vn = (cls == HIT) & fin & (np.where(fin[..., None], n32, 0) != 0).any(axis=2)
        n = np.where(vn[..., None], n32.astype(np.float64), 0.0)
    if albedo is None:
        a, va = np.zeros((h, w, 3)), np.zeros((h, w), bool)
    else:
        a32 = np.asarray(albedo, np.float32)
        va = live & np.isfinite(a32).all(axis=2)
        a = np.where(va[..., None], a32.astype(np.float64), 0.0)
    reliable = live.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            cq, ok = _shift(cls, dx, dy)
            member = ok & live & (cq != VOID)
            nq, _ = _shift(n, dx, dy)
            aq, _ = _shift(a, dx, dy)
            vnq, _ = _shift(vn, dx, dy, False)
            vaq, _ = _shift(va, dx, dy, False)
            bad = member & (cq != cls)
            bad |= member & vn & vnq & ~(1.0 - (n * nq).sum(axis=2) <= RELIABLE_N)
            bad |= member & va & vaq & ~(np.abs(a - aq).max(axis=2) <= RELIABLE_A)
            reliable &= ~bad
    return n, vn, a, va, reliable


def denoise_guided_ref(rgb, depth, ns, normal=None, albedo=None, iterations=5, sigma_color=4.0, sigma_depth=1.0, sigma_normal=0.1):
    """-> float64 (h, w, 3); void pixels carry their input values."""
    rgb32 = np.asarray(rgb, np.float32)
    cls = classes(rgb32, np.asarray(depth, np.float32), np.asarray(ns))
    live = cls != VOID
    if iterations == 0:
        return rgb32.astype(np.float64)
    c = np.where(live[..., None], rgb32.astype(np.float64), 0.0)
    z = np.where(live, np.asarray(depth, np.float64), 0.0)
    hit = cls == HIT
    nrm, vn, alb, va, reliable = guide_bits(cls, normal, albedo)
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
                    nq, _ = _shift(nrm, s * dx, s * dy)
                    vnq, _ = _shift(vn, s * dx, s * dy, False)
                    e = e + np.where(reliable & vn & vnq, np.maximum(0.0, 1.0 - (nrm * nq).sum(axis=2)) / sigma_normal, 0.0)
                    aq, _ = _shift(alb, s * dx, s * dy)
                    vaq, _ = _shift(va, s * dx, s * dy, False)
                    e = e + np.where(reliable & va & vaq, np.abs(alb - aq).max(axis=2) / SIGMA_A, 0.0)
                    w = np.where(ok, H5[dx + 2] * H5[dy + 2] * np.exp(-e), 0.0)
                    sw += w
                    sc += w[..., None] * (cq - c)
                    sv += w * w * vq
            c = np.where(live[..., None], c + sc / sw[..., None], 0.0)
            var = np.where(live, sv / (sw * sw), 0.0)
    return np.where(live[..., None], c, rgb32.astype(np.float64))


def guided_frame(w, h, seed):
    """A frame with guide planes and every special case.  Colours in [0, 2); hit depths on a bumpy slanted plane; the right quarter
    misses the scene (one border between the classes, not a sprinkle: most windows hold one class, so most pixels can be
    reliable); 3 % of the pixels void (ns 0, NaN or infinite colours).  Normals: (0, 0, 1) in every other column band of 5 pixels,
    elsewhere tilted a little (reliable) or a lot (not); some 0, some NaN, 0 on misses.  Albedos: blocks of 4x4 pixels whose steps
    are smaller and larger than the reliable bound, textured background on the misses; some components 0, NaN or infinite."""
    r = np.random.default_rng(seed)
    rgb = (r.random((h, w, 3)) * 2).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    depth = (3 + 0.2 * x + 0.1 * y + 0.05 * r.random((h, w))).astype(np.float32)
    depth[x >= w - w // 4] = MISS
    ns = r.integers(1, 9, (h, w)).astype(np.uint32)
    k = r.random((h, w))
    ns[k < 0.01] = 0
    rgb[(k >= 0.01) & (k < 0.02), 1] = np.nan
    rgb[(k >= 0.02) & (k < 0.03), 2] = np.inf
    n = np.float64([0, 0, 1]) + r.normal(size=(h, w, 3)) * np.where(r.random((h, w, 1)) < 0.7, 0.03, 1.0)
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    n[..., :] = np.where((x // 5 % 2 == 0)[..., None], np.float32([0, 0, 1]), n)
    k = r.random((h, w))
    n[k < 0.02] = 0
    n[(k >= 0.02) & (k < 0.04), 0] = np.nan
    n[depth == MISS] = 0
    blocks = (0.3 + 0.5 * r.random((h // 4 + 1, w // 4 + 1, 3))).astype(np.float32)
    al = blocks[y // 4, x // 4].copy()
    k = r.random((h, w))
    al[k < 0.01, 0] = 0
    al[(k >= 0.01) & (k < 0.02), 2] = np.nan
    al[(k >= 0.02) & (k < 0.03), 0] = np.inf
    return rgb, depth, ns, n, al


GUIDED_SIZES = ((1, 1), (9, 1), (1, 9), (7, 5), (33, 17), (40, 33))   # (w, h)
