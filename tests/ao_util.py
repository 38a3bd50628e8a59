"""What the ambient-occlusion tests share: a float32 numpy restatement of the specification (the opening comment of
qaray_amd/csrc/hip/qa_ao_dev.h: the counter-based words, Marsaglia's sphere point, the cosine-weighted direction, the facing normal),
written from that comment, and the independent route of the GPU tests: the camera rays of every sample handed out
(camera_sample_rays_device), cast as rays of the caller's (cast_rays_device), the directions made on the host, and the shadow rays
tested one by one (occluded_device)."""
import numpy as np

F32 = np.float32
U32 = np.uint32
MISS = F32(1.0e30)
GOLDEN_RATIO = 0x9E3779B9
COUNTER_SALT = 0x632BE5AB
ATTEMPTS = 8
PLANES = ("open", "rays", "ao")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def u32(a):
    """Words as uint32 arrays (their products and sums wrap, as the header's do)"""
    a = np.asarray(a)
    if a.dtype == np.uint32:
        return a
    return (a.astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32) if a.dtype.kind in "iu" else a.astype(np.uint32)


def mix(h):
    """The finaliser of qa_pixel_rand"""
    h = np.atleast_1d(u32(h)).copy()
    h ^= h >> U32(16)
    h *= U32(0x85EBCA6B)
    h ^= h >> U32(13)
    h *= U32(0xC2B2AE35)
    h ^= h >> U32(16)
    return h


def key_of(seed, stream):
    return mix(U32(int(seed) & 0xFFFFFFFF) ^ (np.atleast_1d(u32(stream)) * U32(GOLDEN_RATIO)))


def ray_key(key, c):
    return mix(u32(key) ^ mix(np.atleast_1d(u32(c)) + U32(COUNTER_SALT)))


def signed_unit(w):
    """(float) (w >> 8) * 2^-23 - 1: both steps are exact in float32"""
    return ((u32(w) >> U32(8)).astype(F32) * F32(2.0 ** -23) - F32(1)).astype(F32)


def sphere_ref(kr):
    """kr (n,) -> (s (n, 3) float32, fallback (n,) bool, attempts (n,) the index of the attempt taken, 8 for none)"""
    kr = u32(kr).reshape(-1)
    n = len(kr)
    s = np.zeros((n, 3), F32)
    s[:, 2] = 1
    taken = np.full(n, ATTEMPTS, np.int64)
    open_ = np.arange(n)   # the records that have not taken an attempt yet
    for a in range(ATTEMPTS):
        if not len(open_):
            break
        k = kr[open_]
        x0 = signed_unit(mix(k ^ U32(((2 * a + 1) * GOLDEN_RATIO) & 0xFFFFFFFF)))
        x1 = signed_unit(mix(k ^ U32(((2 * a + 2) * GOLDEN_RATIO) & 0xFFFFFFFF)))
        q = (x0 * x0 + x1 * x1).astype(F32)
        ok = q < F32(1)
        i = open_[ok]
        x0, x1, q = x0[ok], x1[ok], q[ok]
        r = np.sqrt((F32(1) - q).astype(F32)).astype(F32)
        s[i, 0] = (F32(2) * x0).astype(F32) * r
        s[i, 1] = (F32(2) * x1).astype(F32) * r
        s[i, 2] = F32(1) - (F32(2) * q).astype(F32)
        taken[i] = a
        open_ = open_[~ok]
    return s, taken == ATTEMPTS, taken


def direction_from_ref(n, s):
    """n (count, 3) or (3,), s (count, 3) -> d (count, 3) float32"""
    s = np.asarray(s, F32).reshape(-1, 3)
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, F32), s.shape))
    v = (n + s).astype(F32)
    l2 = ((v[:, 0] * v[:, 0]).astype(F32) + (v[:, 1] * v[:, 1]).astype(F32)).astype(F32) + (v[:, 2] * v[:, 2]).astype(F32)
    l2 = l2.astype(F32)
    with np.errstate(all="ignore"):
        d = (v / np.sqrt(l2).astype(F32)[:, None]).astype(F32)
    return np.where((l2 > F32(1e-6))[:, None], d, n).astype(F32)


def directions_ref(seed, stream, c, n):
    s, _, _ = sphere_ref(ray_key(key_of(seed, np.asarray(stream).reshape(-1)), np.asarray(c).reshape(-1)))
    return direction_from_ref(n, s)


def face_normal_ref(N, d):
    N, d = np.asarray(N, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    c = ((N[:, 0] * d[:, 0]).astype(F32) + (N[:, 1] * d[:, 1]).astype(F32)).astype(F32) + (N[:, 2] * d[:, 2]).astype(F32)
    return np.where((c.astype(F32) <= F32(0))[:, None], N, -N).astype(F32)


def ao_ref(open_, rays):
    """rays ? (float) open / (float) rays : 1"""
    open_, rays = np.asarray(open_, np.uint32), np.asarray(rays, np.uint32)
    with np.errstate(all="ignore"):
        q = np.divide(open_.astype(F32), rays.astype(F32), dtype=F32)
    return np.where(rays == 0, F32(1), q).astype(F32)


def samples_ref(ns, first, spp):
    """min(max(ns - first, 0), spp)"""
    return np.minimum(np.maximum(np.asarray(ns, np.int64) - first, 0), spp).astype(np.uint32)


def stream_ids(region, width):
    x0, y0, x1, y1 = region
    yy, xx = np.mgrid[y0:y1, x0:x1]
    return (yy * width + xx).astype(np.uint32)


def first_hits(ctx, region, first, spp):
    """The camera rays of samples first .. first + spp - 1 of the region's pixels, cast as rays of the caller's
    -> dict hit (h, w, spp) bool, point, N (as cast), normal (faced), dirs (h, w, spp, 3) float32"""
    from qaray_amd import hip
    h, w = region[3] - region[1], region[2] - region[0]
    r = ctx.camera_sample_rays_device(region, first, spp, outputs=("origins", "dirs"))
    got = ctx.cast_rays_device(r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3))
    ctx.synchronize()
    dirs = r["dirs"].cpu().numpy().reshape(-1, 3)
    raw = got["normal"].cpu().numpy()
    normal = hip.ao_face_normal_host(raw, dirs)
    return {"N": raw.reshape(h, w, spp, 3), "hit": got["t"].cpu().numpy().reshape(h, w, spp) != MISS, "point": got["point"].cpu().numpy().reshape(h, w, spp, 3),
            "normal": normal.reshape(h, w, spp, 3), "dirs": dirs.reshape(h, w, spp, 3)}


def route(ctx, region, width, first, spp, K, radius, seed, n=None, hits=None):
    """The composition the fused call must equal: first hits through the public queries, the directions of the counters s * K + k of
    the pixels' streams from the host hook, occluded_device on every ray -> dict of the three planes.  n: (h, w) the samples each
    pixel takes (None: spp); hits: first_hits' result when the caller has it already"""
    import torch
    from qaray_amd import hip
    h, w = region[3] - region[1], region[2] - region[0]
    f = first_hits(ctx, region, first, spp) if hits is None else hits
    n = np.full((h, w), spp, np.uint32) if n is None else np.asarray(n, np.uint32)
    use = f["hit"] & (np.arange(spp)[None, None, :] < n[:, :, None])                       # (h, w, spp)
    stream = np.broadcast_to(stream_ids(region, width)[:, :, None, None], (h, w, spp, K))
    c = ((first + np.arange(spp, dtype=np.uint64))[None, None, :, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, None, None, :])
    c = np.broadcast_to(c, (h, w, spp, K))
    sel = np.broadcast_to(use[..., None], (h, w, spp, K))
    nrm = np.broadcast_to(f["normal"][:, :, :, None, :], (h, w, spp, K, 3))[sel]
    pts = np.ascontiguousarray(np.broadcast_to(f["point"][:, :, :, None, :], (h, w, spp, K, 3))[sel], F32)
    d = hip.ao_directions_host(seed, stream[sel], c[sel], nrm)
    open_ = np.zeros((h, w, spp, K), np.uint32)
    if len(pts):
        dev = torch.device("cuda", ctx.device_id)
        occ = ctx.occluded_device(torch.from_numpy(pts).to(dev), torch.from_numpy(d).to(dev), float(radius))
        ctx.synchronize()
        open_[sel] = 1 - occ.cpu().numpy()
    rays = (use.sum(axis=2) * K).astype(np.uint32)
    opened = open_.sum(axis=(2, 3)).astype(np.uint32)
    return {"open": opened, "rays": rays, "ao": ao_ref(opened, rays)}


def planes_numpy(out):
    """ao_device's tensors -> numpy, the integer planes as uint32"""
    return {k: (v.cpu().numpy() if k == "ao" else v.cpu().numpy().view(np.uint32)) for k, v in out.items()}


def differing(a, b):
    """-> the names of the planes that differ (exact comparison, ao by its bits)"""
    return [k for k in PLANES if k in a and k in b and not (a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])))]


def extent_of(hits):
    """The scene's extent as the tests take it: the diagonal of the box around the frame's first-hit points"""
    p = hits["point"][hits["hit"]].astype(np.float64)
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
