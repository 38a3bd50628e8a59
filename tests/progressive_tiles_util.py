"""Numpy restatements of the specification that opens qaray_amd/csrc/hip/qa_prog_error_dev.h: a progressive frame's error per 8x8
tile and the tiles a noisiest-first pass takes.  Written from that comment, not from the code below it."""
import numpy as np

INF = np.float32(np.inf)
FLT_MAX = np.finfo(np.float32).max


def tile_error_np(state):
    """state: uint32 [h, w, 8] -> float32 [ty, tx]."""
    state = np.asarray(state, dtype=np.uint32)
    h, w = state.shape[:2]
    ty, tx = (h + 7) // 8, (w + 7) // 8
    w1 = np.zeros((ty * 8, tx * 8), np.uint32)
    var = np.zeros((ty * 8, tx * 8, 3), np.float32)
    inside = np.zeros((ty * 8, tx * 8), bool)
    w1[:h, :w] = state[..., 1]
    var[:h, :w] = np.ascontiguousarray(state[..., 5:8]).view(np.float32)
    inside[:h, :w] = True
    finished = (w1 >> 31) == 1
    with np.errstate(all="ignore"):
        nan = np.isnan(var).any(axis=-1)
        m = np.where(nan, np.float32(0), var.max(axis=-1)).astype(np.float32)
        v = (m / w1.astype(np.float32)).astype(np.float32)           # one float32 division (n = w1: bit 31 is clear where it counts)
        good = ~nan & (v >= 0) & (v <= FLT_MAX)
        s = np.where(good, np.where(v > 0, v, np.float32(0)), INF)   # (-0 -> +0)
        s = np.where(w1 < 2, INF, s)
        s = np.where(~inside | finished, np.float32(0), s).astype(np.float32)
        a = s.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)   # slot l = 8 * row + column within the tile
        for half in (32, 16, 8, 4, 2, 1):
            a = (a[..., :half] + a[..., half:2 * half]).astype(np.float32)
        return (a[..., 0] * np.float32(0.015625)).astype(np.float32)


def tile_select_np(error, levels, target, max_tiles=0, min_error=0.0):
    """-> (bool mask of error's shape, info dict): a stable descending argsort of the candidates' errors, cut after K'."""
    error = np.asarray(error, dtype=np.float32)
    levels = np.asarray(levels, dtype=np.uint32)
    e, lv = error.ravel(), levels.ravel()
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero((lv < target) & (e > np.float32(min_error)))
    order = cand[np.argsort(-e[cand].astype(np.float64), kind="stable")]   # greater first, equal errors by ascending index
    take = len(cand) if (max_tiles == 0 or max_tiles > len(cand)) else max_tiles
    mask = np.zeros(e.shape, bool)
    mask[order[:take]] = True
    finite = e[cand][np.isfinite(e[cand])]
    info = {"selected": int(take), "candidates": int(len(cand)),
            "cut_bits": int(e[order[take - 1]:order[take - 1] + 1].view(np.uint32)[0]) if take else 0,
            "max_finite_bits": int(finite.max().reshape(1).view(np.uint32)[0]) if finite.size else 0}
    return mask.reshape(error.shape), info
