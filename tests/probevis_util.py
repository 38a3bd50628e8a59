"""What the probe-visibility tests share: a float32 numpy restatement of the specification (the opening comment of
qaray_amd/csrc/hip/qa_probevis_dev.h: the distance moments of a probe's direction cells, the cell a vector points into, the weights
of a cell's eight probes and the shading from them), written from that comment; a float64 evaluation of the same for the bounds;
and the analytic two-room geometry of the leak tests.  The grid's axis function and the shading are tests/probe_util.py's, the
counter-based words behind the jitter tests/ao_util.py's, by import."""
import numpy as np

from ao_util import MISS, bits  # noqa: F401  (the rays' miss value, which the moments clamp; bits() for the tests)
from probe_util import F32, grid_axis_ref, grid_shade_ref, shade_coefficients_ref

FLOOR = F32(0.05)
WRAP = F32(0.2)


def moments_ref(t, m, d, dmax):
    """One probe's t (6 m^2,) -> (6, d, d, 2) float32: one accumulator pair per cell, its texels b ascending, then c ascending"""
    t = np.asarray(t, F32).reshape(6, m, m)
    r = m // d
    dmax = F32(dmax)
    s = np.zeros((6, d, d), F32)
    s2 = np.zeros((6, d, d), F32)
    with np.errstate(all="ignore"):
        for b in range(r):
            for c in range(r):
                tk = t[:, b::r, c::r]                      # texel (B * r + b, C * r + c) of every cell
                x = np.where(tk < dmax, tk, dmax).astype(F32)
                s = (s + x).astype(F32)
                s2 = (s2 + (x * x).astype(F32)).astype(F32)
        n = F32(r * r)
        return np.stack([(s / n).astype(F32), (s2 / n).astype(F32)], axis=-1)


def cell_ref(v, d):
    """v (n, 3) float32 -> the cell index (f * d + row) * d + column each points into"""
    v = np.asarray(v, F32).reshape(-1, 3)
    mag = np.abs(v)
    a = np.zeros(len(v), np.int64)
    ma = mag[:, 0].copy()
    for e in (1, 2):
        more = mag[:, e] > ma
        a[more] = e
        ma = np.where(more, mag[:, e], ma)
    i = np.arange(len(v))
    va, vu, vw = v[i, a], v[i, (a + 1) % 3], v[i, (a + 2) % 3]
    neg = va < 0
    s = np.where(neg, F32(-1), F32(1)).astype(F32)
    fd = F32(d)
    with np.errstate(all="ignore"):
        u = (vu / ma).astype(F32)
        w = ((s * vw).astype(F32) / ma).astype(F32)
        gu = (((u + F32(1)).astype(F32) * F32(0.5)).astype(F32) * fd).astype(F32)
        gw = (((w + F32(1)).astype(F32) * F32(0.5)).astype(F32) * fd).astype(F32)
        col = np.where(gu < fd, np.nan_to_num(gu, nan=0.0).astype(np.int64), d - 1)
        row = np.where(gw < fd, np.nan_to_num(gw, nan=0.0).astype(np.int64), d - 1)
    return ((2 * a + neg) * d + row) * d + col


def weights_ref(moments, origin, spacing, counts, p, nr, normal_bias):
    """Finite points p and normals nr (n, 3) -> (w (n, 8) float32, probe (n, 8) int64, W (n,) float32)"""
    mo = np.asarray(moments, F32)
    d = mo.shape[2]
    mo = mo.reshape(len(mo), 6 * d * d, 2)
    origin, spacing = np.asarray(origin, F32), np.asarray(spacing, F32)
    nx, ny = int(counts[0]), int(counts[1])
    ax = [grid_axis_ref(p[:, e], origin[e], spacing[e], int(counts[e])) for e in range(3)]
    n = len(p)
    w = np.zeros((n, 8), F32)
    probe = np.zeros((n, 8), np.int64)
    W = np.zeros(n, F32)
    with np.errstate(all="ignore"):
        biased = (p + (F32(normal_bias) * nr).astype(F32)).astype(F32)
        for j in range(8):
            idx, we, v = [], [], np.zeros((n, 3), F32)
            for e in range(3):
                far = (j >> e) & 1
                i0, i1, f = ax[e]
                idx.append(i1 if far else i0)
                we.append(f if far else (F32(1) - f).astype(F32))
                Q = (origin[e] + (idx[e].astype(F32) * spacing[e]).astype(F32)).astype(F32)
                v[:, e] = (biased[:, e] - Q).astype(F32)
            probe[:, j] = (idx[2] * ny + idx[1]) * nx + idx[0]
            tri = ((we[0] * we[1]).astype(F32) * we[2]).astype(F32)
            r2 = (((v[:, 0] * v[:, 0]).astype(F32) + (v[:, 1] * v[:, 1]).astype(F32)).astype(F32) + (v[:, 2] * v[:, 2]).astype(F32)).astype(F32)
            rr = np.sqrt(r2).astype(F32)
            cell = cell_ref(v, d)
            mean, mean2 = mo[probe[:, j], cell, 0], mo[probe[:, j], cell, 1]
            var = np.abs((mean2 - (mean * mean).astype(F32)).astype(F32))
            dd = (rr - mean).astype(F32)
            cheb = np.where(rr <= mean, F32(1), (var / (var + (dd * dd).astype(F32)).astype(F32)).astype(F32)).astype(F32)
            cheb = ((cheb * cheb).astype(F32) * cheb).astype(F32)
            vis = np.where(cheb > FLOOR, cheb, FLOOR).astype(F32)
            e3 = [((-v[:, k]) / rr).astype(F32) for k in range(3)]
            dot = (((e3[0] * nr[:, 0]).astype(F32) + (e3[1] * nr[:, 1]).astype(F32)).astype(F32) + (e3[2] * nr[:, 2]).astype(F32)).astype(F32)
            h = ((dot + F32(1)).astype(F32) * F32(0.5)).astype(F32)
            wrap = ((h * h).astype(F32) + WRAP).astype(F32)
            on = rr == 0
            vis, wrap = np.where(on, F32(1), vis).astype(F32), np.where(on, F32(1), wrap).astype(F32)
            w[:, j] = ((tri * wrap).astype(F32) * vis).astype(F32)
            W = (W + w[:, j]).astype(F32)
    return w, probe, W


def vis_grid_shade_ref(sh, moments, origin, spacing, counts, points, normals, normal_bias=0.0):
    """The visibility shading -> rgb (n, 3) float32"""
    sh = np.asarray(sh, F32).reshape(-1, 27)
    P, N = np.asarray(points, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    ok = np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1)
    out = np.zeros((len(P), 3), F32)
    if not ok.any():
        return out
    p, nr = P[ok], N[ok]
    w, probe, W = weights_ref(moments, origin, spacing, counts, p, nr, normal_bias)
    mixed = np.zeros((len(p), 27), F32)
    with np.errstate(all="ignore"):
        for j in range(8):
            k = (w[:, j] / W).astype(F32)
            mixed = (mixed + (k[:, None] * sh[probe[:, j]]).astype(F32)).astype(F32)
    rgb = shade_coefficients_ref(mixed.reshape(-1, 9, 3), nr)
    bad = ~((W > 0) & np.isfinite(W))
    if bad.any():
        rgb[bad] = grid_shade_ref(sh, origin, spacing, counts, p[bad], nr[bad])
    out[ok] = rgb
    return out


def vis_weights_f64(moments, origin, spacing, counts, points, normals, normal_bias=0.0):
    """The specification evaluated in float64 on the float32 inputs (the cell is the float32 restatement's: an integer) ->
    (k (n, 8) the normalised weights w_j / W, probe (n, 8))"""
    mo = np.asarray(moments, F32)
    d = mo.shape[2]
    mo = mo.reshape(len(mo), 6 * d * d, 2).astype(np.float64)
    p, nr = np.asarray(points, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    origin, spacing = np.asarray(origin, F32), np.asarray(spacing, F32)
    nx, ny = int(counts[0]), int(counts[1])
    ax = [grid_axis_ref(p[:, e], origin[e], spacing[e], int(counts[e])) for e in range(3)]
    n = len(p)
    w, probe = np.zeros((n, 8)), np.zeros((n, 8), np.int64)
    biased32 = (p + (F32(normal_bias) * nr).astype(F32)).astype(F32)
    for j in range(8):
        idx, tri, v, v32 = [], np.ones(n), np.zeros((n, 3)), np.zeros((n, 3), F32)
        for e in range(3):
            far = (j >> e) & 1
            i0, i1, f = ax[e]
            g = np.clip((p[:, e].astype(np.float64) - float(origin[e])) / float(spacing[e]), 0, int(counts[e]) - 1)
            f64 = np.clip(g - i0, 0, 1)   # (i0 is the float32 restatement's: a g that rounds up to an integer there gives -1e-8 here)
            idx.append(i1 if far else i0)
            tri = tri * (f64 if far else 1 - f64)
            v[:, e] = p[:, e].astype(np.float64) + float(normal_bias) * nr[:, e] - (float(origin[e]) + idx[e] * float(spacing[e]))
            v32[:, e] = (biased32[:, e] - (origin[e] + (idx[e].astype(F32) * spacing[e]).astype(F32)).astype(F32)).astype(F32)
        probe[:, j] = (idx[2] * ny + idx[1]) * nx + idx[0]
        rr = np.sqrt((v * v).sum(axis=1))
        cell = cell_ref(v32, d)
        mean, mean2 = mo[probe[:, j], cell, 0], mo[probe[:, j], cell, 1]
        var = np.abs(mean2 - mean * mean)
        with np.errstate(all="ignore"):
            cheb = np.where(rr <= mean, 1.0, var / (var + (rr - mean) ** 2)) ** 3
            h = ((-v / rr[:, None] * nr).sum(axis=1) + 1) * 0.5
        vis, wrap = np.maximum(cheb, 0.05), h * h + 0.2
        on = rr == 0
        w[:, j] = tri * np.where(on, 1.0, wrap) * np.where(on, 1.0, vis)
    return w / w.sum(axis=1, keepdims=True), probe


# ---- the two rooms of the leak tests: A = [0, 2]^3, B = [2.1, 4.1] x [0, 2]^2, a wall of 0.1 between them

ROOM_A = (np.float64([0, 0, 0]), np.float64([2, 2, 2]))
ROOM_B = (np.float64([2.1, 0, 0]), np.float64([4.1, 2, 2]))
ROOMS_GRID = (np.float32([0.5, 0.5, 0.5]), np.float32([1, 1, 1]), np.int32([4, 2, 2]))
ROOMS_M, ROOMS_D = 16, 8
ROOMS_DMAX = F32(1.5) * np.sqrt(F32(3))


def rooms_probe_points():
    o, s, cn = ROOMS_GRID
    iz, iy, ix = np.meshgrid(np.arange(cn[2]), np.arange(cn[1]), np.arange(cn[0]), indexing="ij")
    return (o + np.stack([ix, iy, iz], axis=-1).reshape(-1, 3).astype(F32) * s).astype(F32)


def box_exit_distance(p, d, box):
    """The distance from p inside the box along unit directions d (K, 3) to the box's boundary, float64"""
    lo, hi = box
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, (hi - p) / d, np.where(d < 0, (lo - p) / d, np.inf))
    return t.min(axis=1)


def rooms_moments(directions, moments_of):
    """moments (16, 6, 8, 8, 2) of the grid's probes: each probe's t is the exit distance from its own room along `directions`
    (K, 3), reduced by moments_of(t float32 (K,)) -> (6, d, d, 2)"""
    out = []
    for p in rooms_probe_points():
        box = ROOM_A if p[0] < 2.05 else ROOM_B
        t = box_exit_distance(p.astype(np.float64), np.asarray(directions, np.float64), box).astype(F32)
        out.append(moments_of(t))
    return np.stack(out).astype(F32)


def rooms_sh(lit=ROOM_A, value=1.0):
    """Band 0 only: `value` at the probes of the lit room, zeros in the other -> (16, 9, 3)"""
    P = rooms_probe_points()
    sh = np.zeros((len(P), 9, 3), F32)
    in_a = P[:, 0] < 2.05
    sh[in_a if lit is ROOM_A else ~in_a, 0, :] = value
    return sh


def rooms_points(seed=20191, n=300, side="B"):
    """n seeded points near the wall - in B with x in (2.1, 2.5), or mirrored in A with x in (1.5, 2.0) - y, z in (0.5, 1.5), and
    random unit normals"""
    rng = np.random.default_rng(seed)
    lo, hi = (2.1, 2.5) if side == "B" else (1.5, 2.0)
    p = np.stack([rng.uniform(lo, hi, n), rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)], axis=1).astype(F32)
    p[:, 0] = np.clip(p[:, 0], np.nextafter(F32(lo), F32(9)), np.nextafter(F32(hi), F32(0)))
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)
    return p, nr

