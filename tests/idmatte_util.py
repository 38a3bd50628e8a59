"""What the id matte tests share: a numpy restatement of the specification (the opening comment of
qaray_amd/csrc/hip/qa_idmatte_dev.h: the table rule, the ranking, the select product), written from that comment with Python's own
containers and sort, and the independent route of the GPU tests: the camera rays of every sample handed out
(camera_sample_rays_device), cast as rays of the caller's (cast_rays_device), and the restatement over the ids that come back."""
import numpy as np

F32 = np.float32
SLOTS = 8
EMPTY = -2 ** 31
BACKFACE = 0x40000000
MISS = F32(1.0e30)
KEYS = ("node", "material")


def table_ref(hit, keys):
    """One pixel: hit (n,) bool, keys (n,) int -> (ids (8,) int32, counts (8,) uint32, other int).  The rule as the comment states it:
    a hit adds 1 to the slot that holds its key, else takes the first free slot, else adds 1 to `other`; then the occupied slots by
    count descending, equal counts by id ascending, and the free slots behind them."""
    slots, other = [], 0   # [id, count] in the order the ids arrived
    for h, k in zip(np.asarray(hit, bool).reshape(-1), np.asarray(keys).reshape(-1)):
        if not h:
            continue
        k = int(k)
        for s in slots:
            if s[0] == k:
                s[1] += 1
                break
        else:
            if len(slots) < SLOTS:
                slots.append([k, 1])
            else:
                other += 1
    slots.sort(key=lambda s: (-s[1], s[0]))
    ids = np.full(SLOTS, EMPTY, np.int32)
    counts = np.zeros(SLOTS, np.uint32)
    for i, (k, c) in enumerate(slots):
        ids[i], counts[i] = k, c
    return ids, counts, other


def planes_ref(hit, keys, n):
    """Whole planes: hit (h, w, S) bool, keys (h, w, S) int, n (h, w) the samples each pixel takes (its first n of S) -> dict of the
    four planes"""
    h, w = n.shape
    out = {"ids": np.full((h, w, SLOTS), EMPTY, np.int32), "counts": np.zeros((h, w, SLOTS), np.uint32), "other": np.zeros((h, w), np.uint32),
           "samples": np.asarray(n, np.uint32).copy()}
    for y in range(h):
        for x in range(w):
            k = int(n[y, x])
            out["ids"][y, x], out["counts"][y, x], out["other"][y, x] = table_ref(hit[y, x, :k], keys[y, x, :k])
    return out


def select_ref(ids, counts, samples, select):
    """(float) c / (float) n per pixel, c the integer sum of the counts of the slots whose id is in `select`; 0 where n == 0"""
    ids, counts, samples = np.asarray(ids, np.int64), np.asarray(counts, np.int64), np.asarray(samples, np.int64)
    chosen = np.isin(ids, np.asarray(list(select), np.int64).reshape(-1))
    c = (counts * chosen).sum(axis=-1)
    with np.errstate(all="ignore"):
        q = np.divide(c.astype(F32), samples.astype(F32), dtype=F32)
    return np.where(samples == 0, F32(0), q).astype(F32)


def material_key(word):
    """QA_GBUFFER_MATERIAL: the back-face bit cleared; a negative word stays as it is"""
    word = np.asarray(word, np.int32)
    return np.where(word < 0, word, word & ~np.int32(BACKFACE)).astype(np.int32)


def key_of(ids2, key):
    """The key of hits from an ids plane (.., 2) of gbuffer / cast_rays"""
    return np.asarray(ids2[..., 0], np.int32) if key == "node" else material_key(ids2[..., 1])


def route(ctx, region, spp):
    """The independent route: the camera rays of samples 0 .. spp - 1 of the region's pixels, cast as rays of the caller's
    -> (hit (h, w, spp) bool, ids (h, w, spp, 2) int32)"""
    h, w = region[3] - region[1], region[2] - region[0]
    r = ctx.camera_sample_rays_device(region, 0, spp, outputs=("origins", "dirs"))
    got = ctx.cast_rays_device(r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3))
    ctx.synchronize()
    hit = got["t"].cpu().numpy().reshape(h, w, spp) != MISS
    return hit, got["ids"].cpu().numpy().reshape(h, w, spp, 2)


def route_planes(hit, ids2, key, n=None):
    """The restatement over the route's ids -> the four planes; n: the samples each pixel takes (None: all of them)"""
    n = np.full(hit.shape[:2], hit.shape[2], np.uint32) if n is None else np.asarray(n, np.uint32)
    return planes_ref(hit, key_of(ids2, key), n)


def same_planes(a, b):
    """-> the names of the planes that differ (exact comparison; uint32 planes may arrive as int32 tensors' bits)"""
    bad = []
    for k in ("ids", "counts", "other", "samples"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            bad.append(k)
    return bad


def occupied(planes):
    """occupied slots per pixel"""
    return (np.asarray(planes["counts"]).view(np.uint32) > 0).sum(axis=-1)
