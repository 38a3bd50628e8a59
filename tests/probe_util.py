"""What the light-probe tests share: a float32 numpy restatement of the specification (the opening comment of
qaray_amd/csrc/hip/qa_lightprobe_dev.h: the cube map's directions and weights, the jitter words, the ray streams, the nine basis
functions, the wave's projection, the shading and the grid's interpolation), written from that comment; the counter-based words are
tests/ao_util.py's, by import."""
import numpy as np

from ao_util import GOLDEN_RATIO, key_of, mix, ray_key, signed_unit

F32 = np.float32
U32 = np.uint32
MISS = F32(1.0e30)
LANES = 64
FOUR_PI = F32(12.566371)
Y_CONST = (F32(0.282095), F32(0.488603), F32(1.092548), F32(0.315392), F32(0.546274))
BAND = (F32(1), F32(2) / F32(3), F32(0.25))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def offsets_ref(m, seed, S, jitter):
    """-> (j0, j1) float32 (K,) of the probe with stream id S"""
    K = 6 * m * m
    if not jitter:
        return np.full(K, 0.5, F32), np.full(K, 0.5, F32)
    kr = ray_key(np.broadcast_to(key_of(seed, S), (K,)), np.arange(K, dtype=np.uint32))
    j = [((signed_unit(mix(kr ^ U32(((t + 1) * GOLDEN_RATIO) & 0xFFFFFFFF))) + F32(1)).astype(F32) * F32(0.5)).astype(F32) for t in (0, 1)]
    return j[0], j[1]


def directions_ref(m, seed=0, S=0, jitter=False):
    """One probe -> (d (K, 3), w (K,), ray_stream (K,) uint32)"""
    K = 6 * m * m
    k = np.arange(K)
    f, r = k // (m * m), k % (m * m)
    b, c = r // m, r % m
    j0, j1 = offsets_ref(m, seed, S, jitter)
    step = F32(2) / F32(m)
    u = ((c.astype(F32) + j0).astype(F32) * step).astype(F32) - F32(1)
    v = ((b.astype(F32) + j1).astype(F32) * step).astype(F32) - F32(1)
    l2 = ((u * u).astype(F32) + (v * v).astype(F32)).astype(F32) + F32(1)
    i = (F32(1) / np.sqrt(l2).astype(F32)).astype(F32)
    a = f // 2
    s = np.where(f % 2 == 0, F32(1), F32(-1)).astype(F32)
    d = np.zeros((K, 3), F32)
    d[k, a] = s * i
    d[k, (a + 1) % 3] = u * i
    d[k, (a + 2) % 3] = s * (v * i).astype(F32)
    w = (((F32(4) / F32(m * m)) * i).astype(F32) / l2).astype(F32)
    stream = ((int(S) * K + k) & 0xFFFFFFFF).astype(np.uint32)
    return d, w.astype(F32), stream


def basis_ref(d):
    """d (n, 3) -> Y (n, 9) float32"""
    d = np.asarray(d, F32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = Y_CONST
    with np.errstate(all="ignore"):
        Y = np.stack([
            np.full(len(d), c0, F32),
            c1 * y, c1 * z, c1 * x,
            c2 * (x * y).astype(F32), c2 * (y * z).astype(F32),
            c3 * ((F32(3) * (z * z).astype(F32)).astype(F32) - F32(1)).astype(F32),
            c2 * (x * z).astype(F32),
            c4 * ((x * x).astype(F32) - (y * y).astype(F32)).astype(F32),
        ], axis=1)
    return Y.astype(F32)


def project_ref(d, w, rgb, t):
    """The wave's projection of one probe's K rays -> (sh (9, 3) float32, hits int, tmin float32)"""
    d, rgb = np.asarray(d, F32).reshape(-1, 3), np.asarray(rgb, F32).reshape(-1, 3)
    w, t = np.asarray(w, F32).reshape(-1), np.asarray(t, F32).reshape(-1)
    K = len(w)
    Y = basis_ref(d)
    acc = np.zeros((LANES, 28), F32)
    hits = np.zeros(LANES, np.uint32)
    tmin = np.full(LANES, MISS, F32)
    with np.errstate(all="ignore"):
        for first in range(0, K, LANES):   # every lane's next ray, ascending
            k = np.arange(first, min(first + LANES, K))
            lane = k - first
            term = ((w[k, None] * rgb[k]).astype(F32)[:, None, :] * Y[k][:, :, None]).astype(F32)   # (rays, 9, 3)
            acc[lane, :27] = (acc[lane, :27] + term.reshape(len(k), 27)).astype(F32)
            acc[lane, 27] = (acc[lane, 27] + w[k]).astype(F32)
            hits[lane] += (t[k] < MISS).astype(np.uint32)
            tmin[lane] = np.where(t[k] < tmin[lane], t[k], tmin[lane])
        off = 32
        while off >= 1:
            other = np.arange(LANES) ^ off
            acc = (acc + acc[other]).astype(F32)
            hits = hits + hits[other]
            tmin = np.where(tmin[other] < tmin, tmin[other], tmin)
            off //= 2
        scale = FOUR_PI / acc[0, 27]
        sh = (acc[0, :27] * scale).astype(F32).reshape(9, 3)
    return sh, int(hits[0]), tmin[0]


def shade_ref(sh, normals, index=None):
    """sh (probes, 9, 3), normals (n, 3) -> rgb (n, 3) float32"""
    sh = np.asarray(sh, F32).reshape(-1, 9, 3)
    nr = np.asarray(normals, F32).reshape(-1, 3)
    n = len(nr)
    q = np.arange(n) if index is None else np.clip(np.asarray(index, np.int64), 0, len(sh) - 1)
    return shade_coefficients_ref(sh[q], nr)


def shade_coefficients_ref(co, nr):
    """co (n, 9, 3) the coefficients of every shading point, nr (n, 3) -> rgb (n, 3)"""
    Y = basis_ref(nr)
    A = np.array([BAND[0]] + [BAND[1]] * 3 + [BAND[2]] * 5, F32)
    s = np.zeros((len(nr), 3), F32)
    with np.errstate(all="ignore"):
        for c in range(9):
            s = (s + ((A[c] * co[:, c, :]).astype(F32) * Y[:, c, None]).astype(F32)).astype(F32)
        out = np.where(s > 0, s, F32(0)).astype(F32)
    out[~np.isfinite(nr).all(axis=1)] = 0
    return out


def lerp_ref(a, b, f):
    with np.errstate(all="ignore"):
        return (((F32(1) - f).astype(F32) * a).astype(F32) + (f * b).astype(F32)).astype(F32)


def grid_axis_ref(p, origin, spacing, n):
    """-> (i0, i1, f) of one axis; p float32 (count,) finite"""
    with np.errstate(all="ignore"):
        g = ((p - F32(origin)).astype(F32) / F32(spacing)).astype(F32)
    g = np.where(g < 0, F32(0), g).astype(F32)
    top = F32(n - 1)
    g = np.where(g > top, top, g).astype(F32)
    if n > 1:
        i0 = np.minimum(g.astype(np.int64), n - 2)
        i1 = i0 + 1
    else:
        i0 = np.zeros(len(g), np.int64)
        i1 = i0
    return i0, i1, (g - i0.astype(F32)).astype(F32)


def grid_shade_ref(sh, origin, spacing, counts, points, normals):
    sh = np.asarray(sh, F32).reshape(-1, 27)
    P, N = np.asarray(points, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    ok = np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1)
    out = np.zeros((len(P), 3), F32)
    if not ok.any():
        return out
    p, nr = P[ok], N[ok]
    nx, ny = int(counts[0]), int(counts[1])
    ax = [grid_axis_ref(p[:, e], origin[e], spacing[e], int(counts[e])) for e in range(3)]

    def at(z, y, x):
        iz, iy, ix = ax[2][z], ax[1][y], ax[0][x]
        return sh[(iz * ny + iy) * nx + ix]
    fx, fy, fz = (ax[e][2][:, None] for e in range(3))
    x00, x01 = lerp_ref(at(0, 0, 0), at(0, 0, 1), fx), lerp_ref(at(0, 1, 0), at(0, 1, 1), fx)
    x10, x11 = lerp_ref(at(1, 0, 0), at(1, 0, 1), fx), lerp_ref(at(1, 1, 0), at(1, 1, 1), fx)
    mixed = lerp_ref(lerp_ref(x00, x01, fy), lerp_ref(x10, x11, fy), fz)
    out[ok] = shade_coefficients_ref(mixed.reshape(-1, 9, 3), nr)
    return out
