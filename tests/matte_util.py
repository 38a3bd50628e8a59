"""What the matte tests share: float32 numpy restatements of the specification (the opening comment of
qaray_amd/csrc/hip/qa_matte_dev.h), the edge frames of the RGBA product, the scenes (gbuffer_util's, the sphere scene and a
teapot view that shows silhouettes) and the two twins of a scene whose oracle frames ARE the albedo and the backdrop planes."""
import os

import numpy as np

from gbuffer_util import REGION, SCENES, SIZE, bits, emission_twin, scene_blob   # noqa: F401  (re-exported)

F32 = np.float32
SPHERES = "example_project3_sphere.xml"
TEAPOT = "example_project11_teapot.xml"
TEAPOT_FAR = "teapot_far"     # the teapot scene seen from further back: the <RES=0, TEX=0> instance with silhouettes in the region
# the teapot scene's own view from eight times the distance, where the far edge of the floor crosses REGION, rolled so that the edge
# is not a pixel row: 18 pixels of REGION are partly covered at 5 spp and 14 at 4 (CPU oracle)
TEAPOT_FAR_CAMERA = dict(pos=(0.0, -560.0, 179.0), target=(0.0, 0.0, 3.0), up=(0.3, 0.0, 1.0))
SPPS = (1, 4, 5)              # 5 is not a power of two: the divisions round
MIN_PARTIAL = 8               # pixels of the region with 0 < hits < spp that a silhouette scene must show at spp = 5

# scene -> must it show MIN_PARTIAL partly covered pixels (issue: the box and the teapot's own view have none in the region)
MATTE_SCENES = dict({s: s != "example_project12_box.xml" and s != TEAPOT for s in SCENES}, **{SPHERES: True, TEAPOT_FAR: True})


def matte_blob(scene, size=SIZE):
    if scene != TEAPOT_FAR:
        return scene_blob(scene, size)
    from conftest import ensure_assets
    from qaray_amd.host import HostScene, SCENES_DIR
    ensure_assets()
    hs = HostScene(os.path.join(SCENES_DIR, TEAPOT), size=size)
    try:
        hs.set_camera(**TEAPOT_FAR_CAMERA)
        return hs.flatten()
    finally:
        hs.close()


def black_twin(blob, background=None):
    """A copy of the blob in which every material's five colours are 0 and untextured: its frame at no bounce is the part of the
    colour that came from camera rays which met nothing.  background: a plain colour in place of the scene's own backdrop."""
    from qaray_amd import hip
    twin = blob.copy()
    m = hip.blob_table(twin, "materials")
    for k in ("diffuse", "specular", "reflection", "refraction", "emission"):
        m[k]["color"] = 0
        m[k]["texmap"] = -1
    if background is not None:
        bg, _ = hip.blob_backdrop(twin)
        bg["color"] = background
        bg["texmap"] = -1
    return twin


def oracle_hits(blob, region, spp):
    """-> the number of a pixel's `spp` camera rays that hit something, from the oracle's frame of the black twin before a plain white
    background: its red channel is the running mean of 1 on a miss and 0 on a hit, which lies strictly inside (0, 1) exactly where
    some but not all samples hit (a mean of values in [0, 1] with both present cannot round to either end in fp32 for these spp)."""
    from oracle import binding as oracle
    rgb = oracle.render(black_twin(blob, (1.0, 1.0, 1.0)), region, spp, max_bounce=0)[0]
    return rgb[..., 0]


def partial_pixels(blob, region, spp):
    miss = oracle_hits(blob, region, spp)
    return int(((miss > 0) & (miss < 1)).sum())


# ---- the per-pixel reduction ------------------------------------------------------------------------------------------------------
def mean_step(m, x, k):
    """m + (x - m) / (float) k, every operation one float32 operation"""
    with np.errstate(all="ignore"):
        d = np.subtract(x, m, dtype=F32)
        q = np.divide(d, F32(k), dtype=F32)
        return np.add(m, q, dtype=F32)


def accumulate_ref(values, normals, hit):
    """One pixel: values (n, 3) f32, normals (n, 3) f32, hit (n,) bool -> dict of the four planes' values"""
    values, normals = np.asarray(values, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    hit = np.asarray(hit, bool).reshape(-1)
    n = len(hit)
    albedo, backdrop, normal = np.zeros(3, F32), np.zeros(3, F32), np.zeros(3, F32)
    hits = 0
    for s in range(n):
        albedo = mean_step(albedo, values[s], s + 1)
        backdrop = mean_step(backdrop, np.zeros(3, F32) if hit[s] else values[s], s + 1)
        if hit[s]:
            hits += 1
            normal = mean_step(normal, normals[s], hits)
    with np.errstate(all="ignore"):
        coverage = np.divide(F32(hits), F32(n), dtype=F32) if n else F32(0)
    return {"coverage": F32(coverage), "albedo": albedo, "normal": normal, "backdrop": backdrop}


def running_mean_planes(x, hit):
    """Whole planes at once: x (S, ..., 3) f32 per-sample values, hit (S, ...) bool -> the mean of x over the samples where hit, the
    divisor counting those samples, in sample order (the normal plane's rule); 0 where none."""
    m = np.zeros(x.shape[1:], F32)
    k = np.zeros(hit.shape[1:], np.int64)
    for s in range(x.shape[0]):
        k = k + hit[s]
        step = mean_step(m, x[s], np.maximum(k, 1).astype(F32)[..., None])
        m = np.where(hit[s][..., None], step, m)
    return m


# ---- the RGBA product -------------------------------------------------------------------------------------------------------------
def linear_byte(c):
    """displayColorByte(c, false) restated: MIN(1, c), MAX(0, .) as the macros expand (a NaN passes both), roundf of the float32
    product with 255 (exact in float64: floor(x + 0.5) for the x >= 0 that arrive), the x86 conversion (a NaN gives byte 0)."""
    c = np.asarray(c, F32)
    with np.errstate(all="ignore"):
        lo = np.where(F32(1) < c, F32(1), c)
        v = np.where(F32(0) > lo, F32(0), lo)
        x = np.multiply(v, F32(255), dtype=F32).astype(np.float64)
        r = np.floor(x + 0.5)
    return np.where(np.isnan(r), 0, r).astype(np.int64).astype(np.uint8)


def colour_bytes(c, srgb):
    """The colour bytes of float32 components c (.., 3): the linear ones restated above; the sRGB ones through hip.display_host, whose
    bytes tests/test_display_host.py pins to the FrameBuffer (the byte functions are included by qa_matte_dev.h, not restated)."""
    from qaray_amd import hip
    c = np.ascontiguousarray(c, F32)
    if not srgb:
        return linear_byte(c)
    n = c.size // 3
    return hip.display_host(c.reshape(-1, 3), np.ones(n, F32), np.ones(n, np.uint32), 1, True).color.reshape(c.shape)


def rgba_ref(rgb, backdrop, coverage, ns, srgb):
    rgb, backdrop, coverage = (np.asarray(a, F32) for a in (rgb, backdrop, coverage))
    a = coverage[..., None]
    with np.errstate(all="ignore"):
        f = np.subtract(rgb, backdrop, dtype=F32)
        c = np.where(a > 0, np.divide(f, a, dtype=F32), F32(0)).astype(F32)
    out = np.concatenate([colour_bytes(c, srgb), linear_byte(coverage)[..., None]], axis=-1)
    out[np.asarray(ns) == 0] = 0
    return out


def rgba_edge_frames():
    """name -> (rgb (h, w, 3), backdrop (h, w, 3), coverage (h, w), ns (h, w)): 1x1, 17x13 and 33x35 frames of random colours in which
    every edge case of the specification is planted at several pixels: a in {0, 1/5, 1}, ns == 0, rgb below the backdrop by an ulp,
    NaN and infinite components, and a == 1 over a zero backdrop."""
    rng = np.random.default_rng(20251)
    frames = {}
    for (w, h) in ((1, 1), (17, 13), (33, 35)):
        n = w * h
        rgb = rng.uniform(0, 1.5, (n, 3)).astype(F32)
        cov = (rng.integers(0, 6, n) / F32(5)).astype(F32)
        back = (rgb * rng.uniform(0, 1, (n, 1)).astype(F32) * (1 - cov)[:, None]).astype(F32)
        ns = rng.integers(1, 6, n).astype(np.uint32)
        cases = ("a0", "a_fifth", "a1", "ns0", "ulp_below", "nan_rgb", "nan_cov", "inf_rgb", "neg_inf", "inf_both", "opaque")
        for q in range(n):
            case = cases[q % len(cases)] if n > 1 else "ulp_below"
            if case == "a0":
                cov[q] = 0
            elif case == "a_fifth":
                cov[q] = F32(1) / F32(5)
            elif case == "a1":
                cov[q] = 1
            elif case == "ns0":
                ns[q] = 0
            elif case == "ulp_below":
                back[q] = np.nextafter(rgb[q], F32(np.inf))
                cov[q] = (F32(1) / F32(5), F32(1))[q % 2]
            elif case == "nan_rgb":
                rgb[q, q % 3] = np.nan
            elif case == "nan_cov":
                cov[q] = np.nan
            elif case == "inf_rgb":
                rgb[q, q % 3] = np.inf
            elif case == "neg_inf":
                rgb[q, q % 3] = -np.inf
            elif case == "inf_both":
                rgb[q, q % 3] = np.inf
                back[q, q % 3] = np.inf
            elif case == "opaque":
                cov[q] = 1
                back[q] = 0
        frames[f"{w}x{h}"] = (rgb.reshape(h, w, 3), back.reshape(h, w, 3), cov.reshape(h, w), ns.reshape(h, w))
    return frames
