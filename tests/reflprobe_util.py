"""What the reflection-probe tests share: a float32 numpy restatement of the specification (the opening comment of
qaray_amd/csrc/hip/qa_reflprobe_dev.h: the chain's layout, the prefilter's sequential sum per output texel, the face of a direction,
the bilinear lookup between two levels and the grid's blend), written from that comment.  The cube map's directions, the grid's axis
function and the lerp are tests/probe_util.py's restatements, by import, as the header uses qa_lightprobe_dev.h's."""
import numpy as np

from probe_util import F32, directions_ref, grid_axis_ref, lerp_ref


def layout_ref(m, levels=None):
    """-> (levels, offset [levels], res [levels], squarings [levels], T)"""
    lg = int(m).bit_length() - 1
    assert m == 1 << lg
    L = lg + 1 if levels is None else levels
    res = [m >> l for l in range(L)]
    offset = [6 * sum(r * r for r in res[:l]) for l in range(L)]
    squarings = [0] + [max(0, 2 * (lg - l) - 1) for l in range(1, L)]
    return L, offset, res, squarings, 6 * sum(r * r for r in res)


def prefilter_ref(cube, levels=None):
    """cube (n, 6, m, m, 3) -> chain (n, T, 3): the loop over the source records k is the specification's, the output texels of a
    level (and the probes) are the vectorised dimension"""
    cube = np.asarray(cube, F32)
    n, m = cube.shape[0], cube.shape[2]
    K = 6 * m * m
    src = cube.reshape(n, K, 3)
    L, offset, res, squarings, T = layout_ref(m, levels)
    chain = np.zeros((n, T, 3), F32)
    chain[:, :K] = src
    d, w, _ = directions_ref(m)
    with np.errstate(all="ignore"):
        for l in range(1, L):
            o, _, _ = directions_ref(res[l])
            count = len(o)
            acc = np.zeros((n, count, 3), F32)
            W = np.zeros(count, F32)
            for k in range(K):
                c = ((o[:, 0] * d[k, 0]).astype(F32) + (o[:, 1] * d[k, 1]).astype(F32)).astype(F32) + (o[:, 2] * d[k, 2]).astype(F32)
                c = np.where(c > 0, c, F32(0)).astype(F32)
                for _ in range(squarings[l]):
                    c = (c * c).astype(F32)
                on = c > 0
                q = (c * w[k]).astype(F32)
                term = (q[None, :, None] * src[:, k, None, :]).astype(F32)
                acc = np.where(on[None, :, None], (acc + term).astype(F32), acc)
                W = np.where(on, (W + q).astype(F32), W)
            chain[:, offset[l]:offset[l] + count] = (acc / W[None, :, None]).astype(F32)
    return chain


def face_ref(R):
    """R (n, 3) finite and not zero -> (face (n,), u (n,), v (n,))"""
    R = np.asarray(R, F32)
    mag = np.abs(R)
    a = np.zeros(len(R), np.int64)
    ma = mag[:, 0].copy()
    for e in (1, 2):
        up = mag[:, e] > ma
        a[up] = e
        ma[up] = mag[up, e]
    i = np.arange(len(R))
    va, vu, vw = R[i, a], R[i, (a + 1) % 3], R[i, (a + 2) % 3]
    neg = va < 0
    s = np.where(neg, F32(-1), F32(1)).astype(F32)
    with np.errstate(all="ignore"):
        u = (vu / ma).astype(F32)
        v = ((s * vw).astype(F32) / ma).astype(F32)
    return 2 * a + neg, u, v


def level_lookup_ref(chain, m, levels, l, face, u, v):
    """chain (n, T, 3): lookup i in chain[i] -> (n, 3)"""
    _, offset, res, _, _ = layout_ref(m, levels)
    r = res[l]
    with np.errstate(all="ignore"):
        gu = ((((u + F32(1)).astype(F32) * F32(0.5)).astype(F32) * F32(r)).astype(F32) - F32(0.5)).astype(F32)
        gv = ((((v + F32(1)).astype(F32) * F32(0.5)).astype(F32) * F32(r)).astype(F32) - F32(0.5)).astype(F32)
    c0, c1, fu = grid_axis_ref(gu, 0.0, 1.0, r)
    b0, b1, fv = grid_axis_ref(gv, 0.0, 1.0, r)
    i = np.arange(len(chain))
    base = offset[l] + face * r * r

    def tex(b, c):
        return chain[i, base + b * r + c]
    x0 = lerp_ref(tex(b0, c0), tex(b0, c1), fu[:, None])
    x1 = lerp_ref(tex(b1, c0), tex(b1, c1), fu[:, None])
    return lerp_ref(x0, x1, fv[:, None])


def void_ref(R, lam):
    R, lam = np.asarray(R, F32), np.asarray(lam, F32)
    return ~np.isfinite(R).all(axis=1) | (R == 0).all(axis=1) | np.isnan(lam)


def lookup_ref(chain, m, R, lam, levels=None, index=None):
    """chain (probes, T, 3), R (n, 3), lam (n,) -> rgb (n, 3) float32"""
    chain = np.asarray(chain, F32)
    R = np.asarray(R, F32).reshape(-1, 3)
    n = len(R)
    lam = np.broadcast_to(np.asarray(lam, F32), (n,))
    q = np.arange(n) if index is None else np.clip(np.asarray(index, np.int64), 0, len(chain) - 1)
    return lookup_each_ref(chain[q], m, R, lam, levels)


def lookup_each_ref(chains, m, R, lam, levels=None):
    """chains (n, T, 3), one per lookup"""
    L = layout_ref(m, levels)[0]
    out = np.zeros((len(R), 3), F32)
    ok = ~void_ref(R, lam)
    if not ok.any():
        return out
    ch, R, lam = chains[ok], R[ok], lam[ok]
    face, u, v = face_ref(R)
    l0, l1, fl = grid_axis_ref(lam, 0.0, 1.0, L)
    lo, hi = np.zeros((len(R), 3), F32), np.zeros((len(R), 3), F32)
    for l in range(L):
        for dst, which in ((lo, l0), (hi, l1)):
            at = which == l
            if at.any():
                dst[at] = level_lookup_ref(ch[at], m, levels, l, face[at], u[at], v[at])
    out[ok] = lerp_ref(lo, hi, fl[:, None])
    return out


def grid_lookup_ref(chain, m, origin, spacing, counts, points, R, lam, levels=None):
    chain = np.asarray(chain, F32)
    P, R = np.asarray(points, F32).reshape(-1, 3), np.asarray(R, F32).reshape(-1, 3)
    lam = np.broadcast_to(np.asarray(lam, F32), (len(P),))
    ok = np.isfinite(P).all(axis=1) & ~void_ref(R, lam)
    out = np.zeros((len(P), 3), F32)
    if not ok.any():
        return out
    p, r, lm = P[ok], R[ok], lam[ok]
    nx, ny = int(counts[0]), int(counts[1])
    ax = [grid_axis_ref(p[:, e], origin[e], spacing[e], int(counts[e])) for e in range(3)]

    def at(z, y, x):
        return lookup_each_ref(chain[(ax[2][z] * ny + ax[1][y]) * nx + ax[0][x]], m, r, lm, levels)
    fx, fy, fz = (ax[e][2][:, None] for e in range(3))
    x00, x01 = lerp_ref(at(0, 0, 0), at(0, 0, 1), fx), lerp_ref(at(0, 1, 0), at(0, 1, 1), fx)
    x10, x11 = lerp_ref(at(1, 0, 0), at(1, 0, 1), fx), lerp_ref(at(1, 1, 0), at(1, 1, 1), fx)
    out[ok] = lerp_ref(lerp_ref(x00, x01, fy), lerp_ref(x10, x11, fy), fz)
    return out
