"""What the tests of the reprojection with node motion and colour clamp share: a float64 numpy restatement of the SPECIFICATION
comment of qaray_amd/csrc/hip/qa_reproject_motion_dev.h (written from that comment and the one of qa_reproject_dev.h it builds on,
not from the code below them), and the analytic scene of tests/reproject_util.py with a sphere that may stand elsewhere and be
turned: the floor is node 0, the wall node 1, the sphere node 2 (word 0 of the ids planes)."""
import numpy as np

import reproject_util as ru
from qaray_amd import hip
from reproject_util import FLT_MAX, MISS, NEAR, H, W, _c64, rays

MOTION, CLAMP = 1, 2
# Measured on the host build against restate_motion() (tests/test_reproject_motion_host.py prints them):
# - qa_reproject_node_motion: |M_k Wcur(k)(p) - Wprev(k)(p)| as a fraction of the largest |Wprev(k)(p)|, M's float32 entries applied
#   in float64 to the float64 Wcur(k)(p), over a chain of three nodes and 500 points: 7.3e-8 (the rounding of M's entries, and of
#   the float32 itm the inverse runs through);
# - both flags on, decided pixels of motion_inputs(seed=1): colour 9.0e-6 of the largest component, length 9.1e-6 of the largest
#   length with a moving camera (2.2e-6 and 6.2e-6 with a still one): the old form's figures, as the additions add little to them.
NODE_MOTION_MEASURED = 7.3e-8
BOTH_MEASURED = 9.1e-6
NODE_MOTION_BOUND, BOTH_BOUND = 4 * NODE_MOTION_MEASURED, 4 * BOTH_MEASURED


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def instance_table(placements, parents=None):
    """An INSTANCE_DTYPE table: node k has tm = R_k, itm = R_k^-1 (both rounded to float32, column-major), pos = t_k;
    parents[k] (default: every node a root)."""
    n = len(placements)
    t = np.zeros(n, hip.INSTANCE_DTYPE)
    parents = [-1] * n if parents is None else parents
    for k, (R, pos) in enumerate(placements):
        R = np.asarray(R, np.float64)
        t[k]["tm"], t[k]["itm"], t[k]["pos"] = R.T.reshape(-1), np.linalg.inv(R).T.reshape(-1), pos
        t[k]["parent"], t[k]["mesh"], t[k]["mtlset"] = parents[k], -1, -1
        d, a = 0, parents[k]
        while a >= 0:
            d, a = d + 1, parents[a]
        t[k]["depth"] = d
    for k in range(n):   # pre-order: the subtree of k ends before the first later node that is not its descendant
        e = k + 1
        while e < n and t[e]["depth"] > t[k]["depth"]:
            e += 1
        t[k]["subtree_end"] = e
    return t


def world(table, k, p):
    """W(k)(p) in float64 from the table's float32 values: W(k)(p) = W(parent(k))(tm_k p + pos_k)."""
    p = np.asarray(p, np.float64)
    while k >= 0:
        tm = np.asarray(table[k]["tm"], np.float64).reshape(3, 3).T
        p = p @ tm.T + np.asarray(table[k]["pos"], np.float64)
        k = int(table[k]["parent"])
    return p


IDENTITY = (np.eye(3), (0.0, 0.0, 0.0))
# the sphere of the scene before and after its move: 0.6 to the left (against camera C1's move to the right, so that the two
# uncover different ground), 0.2 up, 0.3 nearer, turned 25 degrees about a slanted axis (the way
# that adds to the shift on the side the cameras see)
SPHERE_PREV = (np.eye(3), tuple(ru.SPHERE_C))
SPHERE_CUR = (rotation((0.3, 1.0, 0.2), -25.0), (-0.6, 1.7, -4.7))


def scene_tables():
    """(prev, cur): floor, wall, sphere; only the sphere moves."""
    return instance_table([IDENTITY, IDENTITY, SPHERE_PREV]), instance_table([IDENTITY, IDENTITY, SPHERE_CUR])


def trace(cam, centre, w=W, h=H, origin=(0, 0)):
    """reproject_util.trace with the sphere around `centre` -> depth, ids, points."""
    d = rays(cam, w, h, origin)
    o = _c64(cam)["cam_pos"]
    t = np.full((h, w), 1e30)
    sid = np.full((h, w), -1)
    with np.errstate(all="ignore"):
        tf = -o[1] / d[..., 1]
        P = o + d * tf[..., None]
        m = (tf > 0) & np.isfinite(tf) & (np.abs(P[..., 0]) < 8) & (P[..., 2] > -10) & (P[..., 2] < 10) & (tf < t)
        t[m], sid[m] = tf[m], 0
        tw = (-10 - o[2]) / d[..., 2]
        P = o + d * tw[..., None]
        m = (tw > 0) & np.isfinite(tw) & (np.abs(P[..., 0]) < 8) & (P[..., 1] > 0) & (P[..., 1] < 8) & (tw < t)
        t[m], sid[m] = tw[m], 1
        oc = o - np.asarray(centre, np.float64)
        b = (d * oc).sum(-1)
        disc = b * b - (oc @ oc - ru.SPHERE_R * ru.SPHERE_R)
        ts = -b - np.sqrt(disc)
        m = (disc > 0) & (ts > 0) & (ts < t)
        t[m], sid[m] = ts[m], 2
    depth = t.astype(np.float32)
    ids = np.stack([sid, np.where(sid >= 0, sid + 10, -1)], axis=-1).astype(np.int32)
    return depth, ids, o + d * depth.astype(np.float64)[..., None]


def hidden_by_sphere(points, cam, centre):
    """Whether the sphere around `centre` lies between cam and each point."""
    o = _c64(cam)["cam_pos"]
    v = points - o
    z = np.linalg.norm(v, axis=-1)
    d = v / z[..., None]
    oc = o - np.asarray(centre, np.float64)
    b = (d * oc).sum(-1)
    disc = b * b - (oc @ oc - ru.SPHERE_R * ru.SPHERE_R)
    with np.errstate(all="ignore"):
        ts = -b - np.sqrt(disc)
    return (disc > 0) & (ts > 0) & (ts < z * (1 - 1e-6))


def sphere_local(points, placement):
    R, c = placement
    return (points - np.asarray(c, np.float64)) @ np.asarray(R, np.float64)   # R^T (P - c), row-wise


def local_colour(local):
    """A linear function of the object-local position, within [0.3, 1.7] on the sphere."""
    return np.stack([0.4 * local[..., 0] + 1, 0.4 * local[..., 1] + 1, 0.4 * local[..., 2] + 1], axis=-1)


_FRAMES = {}


def moved_frames(still, w=W, h=H, origin=(0, 0)):
    """The scene before (camera C0, sphere at SPHERE_PREV) and after (C0 when still, else C1; sphere at SPHERE_CUR): dict c0, c1,
    depth0/1, ids0/1, points0/1, motion (hip.node_motion of scene_tables()).  Computed once; read-only arrays."""
    key = (still, w, h, tuple(origin))
    if key not in _FRAMES:
        c0, c1 = ru.cam0(), (ru.cam0() if still else ru.cam1())
        d0, i0, p0 = trace(c0, SPHERE_PREV[1], w, h, origin)
        d1, i1, p1 = trace(c1, SPHERE_CUR[1], w, h, origin)
        f = dict(c0=c0, c1=c1, depth0=d0, ids0=i0, points0=p0, depth1=d1, ids1=i1, points1=p1, motion=hip.node_motion(*scene_tables()))
        for v in f.values():
            if isinstance(v, np.ndarray) and v.ndim:
                v.flags.writeable = False
        _FRAMES[key] = f
    return _FRAMES[key]


def motion_inputs(w=W, h=H, origin=(0, 0), seed=1, still=False, voids=True):
    """reproject_util.inputs() on moved_frames(): a random current colour, the position colour as history, a few void pixels and
    history pixels without history; and the motion table."""
    f = moved_frames(still, w, h, origin)
    r = np.random.default_rng(seed)
    rgb = r.random((h, w, 3), dtype=np.float32)
    ns = np.full((h, w), 4, np.uint32)
    depth = f["depth1"].copy()
    hlen = r.integers(1, 20, (h, w)).astype(np.float32)
    if voids and w * h >= 35:
        flat = r.choice(w * h, 6, replace=False)
        ns.reshape(-1)[flat[0:2]] = 0
        rgb.reshape(-1, 3)[flat[2], 1] = np.nan
        depth.reshape(-1)[flat[3]] = np.inf
        hlen.reshape(-1)[flat[4:6]] = 0
    return dict(c0=f["c0"], c1=f["c1"], cur=(rgb, depth, ns), hist=(ru.position_colour(f["points0"], f["depth0"]), f["depth0"].copy(), hlen),
                origin=tuple(origin), ids=f["ids1"].copy(), hist_ids=f["ids0"].copy(), motion=f["motion"].copy())


def call_motion(fn, a, motion=True, ids=True, **kw):
    """fn = hip.reproject_motion_host or restate_motion on a dict of motion_inputs() (or of reproject_util.inputs(), motion=False)."""
    kw = dict(kw, origin=a["origin"], ids=a["ids"] if ids else None, hist_ids=a["hist_ids"] if ids else None, motion=a["motion"] if motion else None)
    if fn is restate_motion:
        return fn(a["c0"], a["c1"], a["cur"], a["hist"], **kw)
    return fn(a["cur"], a["hist"], a["c0"], a["c1"], **kw)


def window_stats(rgb, depth, ns, radius):
    """Step 5' in float64 -> (k, mean (h, w, 3), sigma (h, w, 3)) of every pixel's window, and the class plane (0 void, 1 miss, 2 hit)."""
    c = np.asarray(rgb, np.float64)
    h, w = c.shape[:2]
    with np.errstate(all="ignore"):
        void = (np.asarray(ns) == 0) | ~np.isfinite(np.asarray(rgb)).all(-1) | ~np.isfinite(np.asarray(depth))
        cls = np.where(void, 0, np.where(np.asarray(depth, np.float32) == MISS, 1, 2))
        r = radius
        pc = np.zeros((h + 2 * r, w + 2 * r, 3))
        pk = np.zeros((h + 2 * r, w + 2 * r), np.int64)
        pc[r:r + h, r:r + w], pk[r:r + h, r:r + w] = np.where(void[..., None], 0.0, c), cls
        k, s = np.zeros((h, w), np.int64), np.zeros((h, w, 3))
        offsets = [(dy, dx) for dy in range(2 * r + 1) for dx in range(2 * r + 1)]
        for dy, dx in offsets:
            on = (pk[dy:dy + h, dx:dx + w] == cls) & (cls != 0)
            k += on
            s += np.where(on[..., None], pc[dy:dy + h, dx:dx + w], 0.0)
        mean = s / np.maximum(k, 1)[..., None]
        q = np.zeros((h, w, 3))
        for dy, dx in offsets:
            on = (pk[dy:dy + h, dx:dx + w] == cls) & (cls != 0)
            q += np.where(on[..., None], (pc[dy:dy + h, dx:dx + w] - mean) ** 2, 0.0)
        sigma = np.sqrt(q / np.maximum(k, 1)[..., None])
    return k, mean, sigma, cls


def restate_motion(c0, c1, cur, hist, origin=(0, 0), ids=None, hist_ids=None, motion=None, clamp=False, clamp_radius=1, clamp_gamma=1.0,
                   depth_tolerance=0.05, max_history=64.0, identity_motion=False):
    """The specification in float64 -> reproject_util.restate's dict, and: moved (the MOVED pixels), unclamped (c_h before 5'),
    lo, hi, k (the window's box and count; with clamp).  motion: a NODE_MOTION_DTYPE table (sets QA_REPROJECT_MOTION).
    identity_motion: every record's m replaced by the identity (the tests show with it that their bounds would see a history
    fetched from where the node is instead of where it was)."""
    rgb, depth, ns = cur
    hrgb, hdepth, hlen = hist
    c = np.asarray(rgb, np.float64)
    z = np.asarray(depth, np.float64)
    h, w = z.shape
    x0, y0 = origin
    with np.errstate(all="ignore"):
        void = (np.asarray(ns) == 0) | ~np.isfinite(np.asarray(rgb)).all(-1) | ~np.isfinite(np.asarray(depth))
        miss = ~void & (np.asarray(depth, np.float32) == MISS)
        hit = ~void & ~miss
        n = np.asarray(ns, np.float64)
        tx, ty = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        und = np.zeros((h, w), bool)
        moved = np.zeros((h, w), bool)
        if motion is not None:
            assert ids is not None and hist_ids is not None
            node = np.asarray(ids)[..., 0].astype(np.int64)
            inside = (node >= 0) & (node < len(motion))
            moved = hit & inside & (np.asarray(motion["moved"])[np.where(inside, node, 0)] != 0)
        still = all(np.array_equal(c0[k], c1[k]) for k in hip.CAMERA_DTYPE.names)
        k0, k1 = _c64(c0), _c64(c1)
        d = rays(c1, w, h, origin)
        zz = np.where(hit, z, 0.0)
        P = k1["cam_pos"] + d * zz[..., None]
        if moved.any() and not identity_motion:
            m = np.asarray(motion["m"], np.float64)[np.where(moved, node, 0)]     # (h, w, 12)
            A = m[..., :9].reshape(h, w, 3, 3)
            P = np.where(moved[..., None], np.einsum("hwij,hwj->hwi", A, P) + m[..., 9:], P)
        wv = np.where(hit[..., None], P - k0["cam_pos"], d)
        a = k0["screenA"] - k0["cam_pos"]
        nrm = np.cross(k0["screenU"], k0["screenV"])
        vn, nu = np.cross(k0["screenV"], nrm), np.cross(nrm, k0["screenU"])
        wn = wv @ nrm
        s = (a @ nrm) / wn
        r = s[..., None] * wv - a
        u = (r @ vn) / (k0["screenU"] @ vn)
        v = (r @ nu) / (k0["screenV"] @ nu)
        ul, vl = u - x0, v - y0
        ww = (wv * wv).sum(-1)
        zp = np.where(hit, np.sqrt(ww), 0.0)
        ok = ~void & (wn != 0) & (s > 0) & np.isfinite(ul) & np.isfinite(vl) & (ul >= -1) & (ul < w) & (vl >= -1) & (vl < h)
        ok &= ~(hit & (ww > FLT_MAX))
        u1 = ~void & (np.abs(wn) <= NEAR * np.sqrt(ww) * np.linalg.norm(nrm))
        fin = np.isfinite(ul) & np.isfinite(vl)
        u1 |= ~void & fin & ((np.abs(ul + 1) <= NEAR) | (np.abs(ul - w) <= NEAR * w) | (np.abs(vl + 1) <= NEAR) | (np.abs(vl - h) <= NEAR * h))
        shortcut = np.full((h, w), still) & ~moved      # step 4': equal cameras and an unmoved pixel
        ul, vl, zp = np.where(shortcut, tx, ul), np.where(shortcut, ty, vl), np.where(shortcut, np.where(hit, z, 0.0), zp)
        ok = np.where(shortcut, ~void, ok)
        und |= u1 & ~shortcut
        uls, vls = np.where(ok, ul, 0.0), np.where(ok, vl, 0.0)
        i0, j0 = np.floor(uls), np.floor(vls)
        fx, fy = uls - i0, vls - j0
        i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
        sw, sl, sc, taps = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w), np.int64)
        thr = depth_tolerance * zp
        for dj in (0, 1):
            for di in (0, 1):
                wt = (fx if di else 1 - fx) * (fy if dj else 1 - fy)
                i, j = i0 + di, j0 + dj
                inside = ok & (wt != 0) & (i >= 0) & (i < w) & (j >= 0) & (j < h)
                ic, jc = np.clip(i, 0, w - 1), np.clip(j, 0, h - 1)
                tr, tz, tl = np.asarray(hrgb)[jc, ic], np.asarray(hdepth)[jc, ic], np.asarray(hlen)[jc, ic]
                val = inside & (tl > 0) & np.isfinite(tr).all(-1) & np.isfinite(tz) & ((tz.astype(np.float32) == MISS) == miss)
                dz = np.abs(tz.astype(np.float64) - zp)
                und |= val & hit & (np.abs(dz - thr) <= NEAR * thr) & ~(shortcut & (dz == 0))
                val &= np.where(hit, dz <= thr, True)
                if ids is not None and hist_ids is not None:
                    val &= (np.asarray(hist_ids)[jc, ic] == np.asarray(ids)).all(-1)
                wt = np.where(val, wt, 0.0)
                sw += wt
                sc += wt[..., None] * np.where(val[..., None], tr, 0.0).astype(np.float64)
                sl += wt * np.where(val, tl, 0.0).astype(np.float64)
                taps += val
        und |= ok & (np.abs(sw - 0.25) <= NEAR * 0.25)
        has = ok & (sw >= 0.25)
        den = np.where(has, sw, 1.0)
        ch = sc / den[..., None]
        unclamped = ch
        extra = {}
        if clamp:
            k, mean, sigma, _ = window_stats(rgb, depth, ns, clamp_radius)
            lo, hi = mean - clamp_gamma * sigma, mean + clamp_gamma * sigma
            box = has & (k >= 2) & np.isfinite(lo).all(-1) & np.isfinite(hi).all(-1)
            ch = np.where(box[..., None], np.minimum(np.maximum(ch, lo), hi), ch)
            extra = dict(lo=lo, hi=hi, k=k, box=box)
        L = np.minimum(sl / den, max_history)
        kk = n / np.where(has, L + n, 1.0)
        out = np.where(has[..., None], ch + (c - ch) * kk[..., None], c)
        length = np.where(void, 0.0, np.where(has, L + n, n))
    return dict(out=out, length=length, has=has, c_h=ch, unclamped=unclamped, u=ul + x0, v=vl + y0, ul=ul, vl=vl, sw=sw, taps=taps, undecided=und,
                void=void, hit=hit, moved=moved, **extra)


def all_moved_motion():
    """A table in which every node of the scene is moved: the floor and the wall a little (so that most of their pixels keep a
    history), the sphere as in scene_tables()."""
    prev, cur = scene_tables()
    cur = instance_table([(rotation((0, 1, 0), 1.0), (0.05, 0.0, 0.02)), (np.eye(3), (0.1, 0.0, 0.0)), SPHERE_CUR])
    m = hip.node_motion(prev, cur)
    assert m["moved"].all()
    return m


# ---- previews of the renderer's own frames (GPU): tests/test_gpu_reproject_motion.py and tools/gpu_reproject_motion_quality.py ------

PREVIEW_SCENE, PREVIEW_SIZE, PREVIEW_SPP, PREVIEW_FRAMES = "custom_softshadow.xml", (64, 48), 4, 8
NODE_S1, NODE_GROUP, NODE_GROUP_END = 2, 3, 7     # custom_softshadow.xml: s1; group and its subtree (s2, wall, knob)


def luma(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def luma_rmse(x, truth):
    return float(np.sqrt(np.mean((luma(np.asarray(x, np.float64)) - luma(np.asarray(truth, np.float64))) ** 2)))


def preview_run(ctx, blob, scenario, **preview_kw):
    """PREVIEW_FRAMES frames of PREVIEW_SPP samples of `blob` (PREVIEW_SCENE at PREVIEW_SIZE), a new seed each, through a
    hip.TemporalPreview(ctx, region, **preview_kw) with ids and without a reset.  scenario: "still"; "light" (the first light's
    intensity is quartered before frame 5); "nodes" (before every frame but the first s1 moves 0.15 along x and group turns one
    degree about z, through edit_instances, and every push brings the instance table).
    -> dict raw (the last frame), acc, length, ids (numpy), truth (256 spp of the final scene), moved (pixels of a node that moved)."""
    import torch
    w, h = PREVIEW_SIZE
    region = (0, 0, w, h)
    ctx.upload_scene(blob)
    work = blob.copy()
    cam = hip.blob_camera(work).copy()
    inst, lights = hip.blob_table(work, "instances"), hip.blob_table(work, "lights")
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    ns = torch.empty((h, w), dtype=torch.int32, device=dev)
    ids = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tp = hip.TemporalPreview(ctx, region, **preview_kw)
    turn = rotation((0, 0, 1), 1.0).astype(np.float32)
    for k in range(PREVIEW_FRAMES):
        if scenario == "light" and k == 4:
            lights[0]["intensity"] *= np.float32(0.25)
            ctx.edit_lights(0, lights[0:1])
        if scenario == "nodes" and k > 0:
            inst[NODE_S1]["pos"] += np.array([0.15, 0.0, 0.0], np.float32)
            inst["tm"][NODE_GROUP] = (turn @ inst["tm"][NODE_GROUP].reshape(3, 3).T).T.reshape(9)      # (column-major storage)
            inst["itm"][NODE_GROUP] = (inst["itm"][NODE_GROUP].reshape(3, 3).T @ turn.T).T.reshape(9)
            ctx.edit_instances(NODE_S1, inst[NODE_S1:NODE_GROUP + 1])
        seed = 1000 + k
        ctx.render_region_device(region, PREVIEW_SPP, rgb, depth, ns, seed=seed, stream=s.cuda_stream)
        ctx.gbuffer_device(region, seed, ids=ids, stream=s.cuda_stream)
        acc, length = tp.push(cam, rgb, depth, ns, ids, instances=inst if scenario == "nodes" else None, stream=s.cuda_stream)
        s.synchronize()
    out = dict(raw=rgb.cpu().numpy(), acc=acc.cpu().numpy(), length=length.cpu().numpy(), ids=ids.cpu().numpy())
    assert np.array_equal(ctx.download_scene(), work)
    out["truth"] = ctx.render_region(region, 256, seed=77)[0]
    node = out["ids"][..., 0]
    out["moved"] = (node == NODE_S1) | ((node >= NODE_GROUP) & (node < NODE_GROUP_END))
    return out
