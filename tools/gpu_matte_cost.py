#!/usr/bin/env python3
"""What the matte planes cost, on the frames of bench.py's C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml,
3840x2160) at 4 and 64 spp: between two events on the caller's stream, warm-up calls, then the median of --repeats, of
  matte all       Context.matte_device, all four planes (40 bytes written per pixel)
  matte coverage  Context.matte_device, the coverage plane alone (no material or texture is looked up)
  twin frame      the yardstick, how an anti-aliased albedo was obtained before this call: Context.render_region_device of the uploaded
                  "emission := diffuse" twin of the scene at the same spp with max_bounce = 0, in a context of its own (it shades
                  every sample and writes rgb, depth and ns: 20 bytes per pixel)
  rgba            Context.rgba_device over the frame's rgb, the matte's backdrop and coverage and the frame's ns
The expectation is: matte all <= twin frame's median + the twin frame's own min-max spread; `within` says whether it held.  Each
configuration and spp runs in a child process of its own under a time limit (--limit seconds), by the rule of tools/cost.py.  Needs
a GPU: there is no fallback."""
import statistics
import sys

import cost

TOOL = "gpu_matte_cost"
SPPS = (4, 64)


def emission_twin(blob, hip):
    """A copy of the blob in which every material emits its diffuse colour (texture included) and does nothing else"""
    twin = blob.copy()
    m = hip.blob_table(twin, "materials")
    m["emission"] = m["diffuse"]
    for k in ("diffuse", "specular", "reflection", "refraction"):
        m[k]["color"] = 0
    return twin


def measure(tag, spp, warmup, repeats):
    ctx, blob, region, dev, s = cost.open_scene(TOOL, tag)
    torch, hip = cost.gpu(TOOL)
    scene, w, h = cost.CONFIGS[tag]
    twin = hip.Context(0)
    twin.upload_scene(emission_twin(blob, hip))
    rgb, depth, ns = cost.frame_tensors(dev, w, h)
    m = ctx.matte_device(region, spp, stream=s.cuda_stream)
    rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    twin.render_region_device(region, spp, rgb, depth, ns, max_bounce=0, stream=s.cuda_stream)
    s.synchronize()
    steps = [("twin frame", lambda: twin.render_region_device(region, spp, rgb, depth, ns, max_bounce=0, stream=s.cuda_stream)),
             ("matte all", lambda: ctx.matte_device(region, spp, stream=s.cuda_stream, **m)),
             ("matte coverage", lambda: ctx.matte_device(region, spp, coverage=m["coverage"], stream=s.cuda_stream)),
             ("rgba", lambda: ctx.rgba_device(rgb, m["backdrop"], m["coverage"], ns, out=rgba, stream=s.cuda_stream))]
    yard = None
    for name, call in steps:
        spans = cost.timed(s, call, warmup, repeats)
        ms = statistics.median(spans)
        if name == "twin frame":
            yard = (ms, max(spans) - min(spans))
        within = {"library": cost.library(), "within": bool(ms <= yard[0] + yard[1])} if name.startswith("matte") else {}
        cost.emit(TOOL, f"{tag} {spp} spp {name}", config=tag, scene=scene, size=[w, h], spp=spp, what=name, **cost.summary(spans),
                  share_of_twin_frame=round(ms / yard[0], 4), **within)
    ctx.close()
    twin.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    ap.add_argument("--spp", type=int, choices=SPPS)
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.spp or SPPS[0], a.warmup, a.repeats)
    cost.run_children(__file__, [[tag, "--spp", str(spp)] for tag in cost.TAGS for spp in SPPS], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
