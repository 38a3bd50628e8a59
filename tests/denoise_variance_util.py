"""What the variance denoiser's tests share: a float64 numpy restatement of the VARIANCE FORM section of the opening comment of
qaray_amd/csrc/hip/qa_denoise_dev.h on top of the sections it extends (written from that text, not from its code; the iterations
are tests/denoise_guided_util.py's restatement over again, since that function has no way in for another pass 0), the frames the
host and the device tests run, and the accumulated previews of the oracle's frames behind the one claim about quality."""
import numpy as np

from denoise_guided_util import guide_bits, guided_frame
from denoise_util import EPS_L, H5, HIT, MISS, SLOPE_FLOOR, VOID, _shift, bits, classes, luma  # noqa: F401

SIGMA_A = float(np.float32(0.02))
VARIANCE_SCALES = (0.25, 1.0, 4.0, 16.0)     # the sweep of DESIGN.md 4k
# the host build against denoise_variance_ref(), as a fraction of the frame's largest input component: measured 1.34e-5
# (tests/test_denoise_variance_host.py prints it per size), asserted at 4 x, which stays inside the 1e-4 of the forms below it
RESTATEMENT_MEASURED = 1.34e-5
RESTATEMENT_BOUND = min(4 * RESTATEMENT_MEASURED, 1e-4)


def trusted_plane(cls, variance):
    t = np.asarray(variance, np.float32)
    with np.errstate(invalid="ignore"):
        return (cls != VOID) & np.isfinite(t) & (t >= 0)


def pass0_variance(cls, l, variance, variance_scale):
    """Pass 0 of the base form and of the VARIANCE FORM -> (var, spatial var, trusted)."""
    live = cls != VOID
    members = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, ok = _shift(l, dx, dy)
            cq, _ = _shift(cls, dx, dy)
            members.append((lq, ok & live & (cq == cls), dx, dy))
    n = sum(m.astype(np.float64) for _, m, _, _ in members)
    mean = sum(np.where(m, lq, 0.0) for lq, m, _, _ in members) / np.maximum(n, 1)
    var = sum(np.where(m, (lq - mean) ** 2, 0.0) for lq, m, _, _ in members) / np.maximum(n, 1)
    spatial = np.where(n > 1, var, 0.0)
    if variance is None:
        return spatial, spatial, np.zeros(cls.shape, bool)
    tr = trusted_plane(cls, variance)
    t = np.where(tr, np.asarray(variance, np.float64), 0.0)
    sw, st = np.zeros(cls.shape), np.zeros(cls.shape)
    for _, m, dx, dy in members:
        tq, _ = _shift(t, dx, dy)
        trq, _ = _shift(tr, dx, dy, False)
        w = (2.0 if dx == 0 else 1.0) * (2.0 if dy == 0 else 1.0)
        on = m & trq
        sw += np.where(on, w, 0.0)
        st += np.where(on, w * tq, 0.0)
    return np.where(tr, variance_scale * (st / np.maximum(sw, 1.0)), spatial), spatial, tr


def denoise_variance_ref(rgb, depth, ns, normal=None, albedo=None, variance=None, iterations=5, sigma_color=4.0, sigma_depth=1.0, sigma_normal=0.1,
                         variance_scale=4.0):
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
    var, _, _ = pass0_variance(cls, luma(c), variance, variance_scale)
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


def variance_frame(w, h, seed):
    """denoise_guided_util.guided_frame and a variance plane: about a third of the pixels -1 in patches and singly, the others the size
    of the frame's spatial variance (colours in [0, 2): 0.1 and less); a few NaN, infinite, negative and 0 values."""
    rgb, depth, ns, normal, albedo = guided_frame(w, h, seed)
    r = np.random.default_rng(seed + 7)
    y, x = np.mgrid[0:h, 0:w]
    var = (0.1 * r.random((h, w))).astype(np.float32)
    var[(x // 6 + y // 4) % 3 == 0] = -1
    k = r.random((h, w))
    var[k < 0.1] = -1
    var[(k >= 0.10) & (k < 0.12)] = np.nan
    var[(k >= 0.12) & (k < 0.14)] = np.inf
    var[(k >= 0.14) & (k < 0.16)] = -0.5
    var[(k >= 0.16) & (k < 0.18)] = 0
    return rgb, depth, ns, normal, albedo, var


VARIANCE_SIZES = ((1, 1), (17, 13), (33, 35))   # (w, h): a lone pixel, a partial tile on both axes, three tiles by three


# ---- the oracle's frames, accumulated (tests/test_denoise_variance_host.py, tools/reproject_moments_quality.py) ----------

QUALITY_SCENES = {"textures": "custom_textures.xml", "box": "example_project12_box.xml"}
QUALITY_SIZE, QUALITY_SPP, QUALITY_FRAMES = (64, 64), 4, 8
_PREVIEWS = {}


def oracle_preview(which):
    """QUALITY_FRAMES oracle frames of QUALITY_SPP samples and different seeds of a still camera, accumulated on the CPU by
    hip.reproject_moments_host with MOMENTS (defaults) -> dict acc, variance, length, depth, ns (the last frame's), albedo (the frame of the scene's emission twin at one sample and no bounce, as tests/test_gbuffer_host.py shows it to be),
    raw (the last frame), truth (256 spp).  Computed once per scene; read-only."""
    if which not in _PREVIEWS:
        from gbuffer_util import emission_twin, scene_blob
        from oracle import binding as oracle
        from qaray_amd import hip
        w, h = QUALITY_SIZE
        region = (0, 0, w, h)
        blob = scene_blob(QUALITY_SCENES[which], size=QUALITY_SIZE)
        cam = hip.blob_camera(blob).copy()
        hist, mom, res, raw, depth, ns = None, None, None, None, None, None
        for k in range(QUALITY_FRAMES):
            raw, depth, ns = oracle.render(blob, region, QUALITY_SPP, seed=1000 + k)[:3]
            raw = raw.astype(np.float32)
            if hist is None:
                hist = (np.zeros_like(raw), depth, np.zeros(depth.shape, np.float32))
            res = hip.reproject_moments_host((raw, depth, ns), hist, cam, cam, hist_moments=mom, moments=True)
            hist, mom = (res[0], depth, res[1]), res[2]
        albedo = oracle.render(emission_twin(blob), region, 1, max_bounce=0)[0].astype(np.float32)
        truth = oracle.render(blob, region, 256, seed=77)[0]
        p = dict(acc=res[0], variance=res[3], length=res[1], depth=depth, ns=ns, albedo=albedo, raw=raw, truth=truth)
        for v in p.values():
            v.flags.writeable = False
        _PREVIEWS[which] = p
    return _PREVIEWS[which]


def device_quality(ctx, which):
    """Section 4's variance_scale row on the device: eight 4-spp frames of the renderer through hip.TemporalPreview(moments=True), the
    accumulated frame filtered by denoise_guided_device (i) and denoise_variance_device (ii) at their defaults, both guides from
    gbuffer_device -> luma RMSE to 256 spp of raw, acc, i, ii, and the fraction of trusted pixels."""
    import torch
    from gbuffer_util import scene_blob
    from qaray_amd import hip
    w, h = QUALITY_SIZE
    region = (0, 0, w, h)
    blob = scene_blob(QUALITY_SCENES[which], size=QUALITY_SIZE)
    ctx.upload_scene(blob)
    cam = hip.blob_camera(blob).copy()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
    rgb, depth, ns, ids = new((h, w, 3)), new((h, w)), new((h, w), torch.int32), new((h, w, 2), torch.int32)
    normal, albedo = new((h, w, 3)), new((h, w, 3))
    torch.cuda.synchronize()
    tp = hip.TemporalPreview(ctx, region, moments=True)
    for k in range(QUALITY_FRAMES):
        ctx.render_region_device(region, QUALITY_SPP, rgb, depth, ns, seed=1000 + k, stream=s.cuda_stream)
        ctx.gbuffer_device(region, 1000 + k, normal=normal, albedo=albedo, ids=ids, stream=s.cuda_stream)
        acc, length = tp.push(cam, rgb, depth, ns, ids, stream=s.cuda_stream)
    guided = ctx.denoise_guided_device(acc, depth, ns, normal, albedo, stream=s.cuda_stream)
    with_var = ctx.denoise_variance_device(acc, depth, ns, normal, albedo, tp.variance, stream=s.cuda_stream)
    s.synchronize()
    truth = ctx.render_region(region, 256, seed=77)[0]
    e = lambda t: luma_rmse(t.cpu().numpy(), truth)   # noqa: E731
    return dict(raw=e(rgb), acc=e(acc), i=e(guided), ii=e(with_var), trusted=float((tp.variance >= 0).float().mean()))


def luma_rmse(x, truth):
    return float(np.sqrt(np.mean((luma(np.asarray(x, np.float64)) - luma(np.asarray(truth, np.float64))) ** 2)))
