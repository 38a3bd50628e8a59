#!/usr/bin/env python3
"""What the ray queries cost, on the frames of bench.py's C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml,
3840x2160), one ray per pixel: windows of --launches calls queued back to back between two events on the caller's stream (the
stream is held busy while the host enqueues them, so a window holds device time only), warm-up windows, then the median of
--repeats windows, per call, of
  gbuffer        Context.gbuffer_device, all four planes: the yardstick (the same walk from rays it builds itself, 8x8 pixel tiles)
  cast           Context.cast_rays_device of camera_rays_device's rays in their own order (rows of the frame), all four outputs
  cast shuffled  the same rays in a fixed random permutation: what divergence costs
  occluded       Context.occluded_device of the rays of `cast` with tmax = 1e30
Every figure in milliseconds and Mrays/s, and as a multiple of gbuffer.  Each configuration runs in a child process of its own
under a time limit (--limit seconds), by the rule of tools/cost.py.  The lines are printed and written to --out (default
profiles/ray_query_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import cost

TOOL = "gpu_ray_query_cost"


def measure(tag, warmup, repeats, launches, hold_cycles):
    ctx, _, region, dev, s = cost.open_scene(TOOL, tag)
    torch, hip = cost.gpu(TOOL)
    scene, w, h = cost.CONFIGS[tag]
    n = w * h
    with torch.cuda.stream(s):
        g = ctx.gbuffer_device(region, stream=s.cuda_stream)
        o, d = ctx.camera_rays_device(region, stream=s.cuda_stream)
        perm = torch.randperm(n, device=dev, generator=torch.Generator(dev).manual_seed(20240611))
        so, sd = o[perm].contiguous(), d[perm].contiguous()
        tmax = torch.full((n,), 1e30, dtype=torch.float32, device=dev)
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        out = ctx.cast_rays_device(o, d, stream=s.cuda_stream)
    s.synchronize()
    hits = int((out["t"] != hip.QA_RAY_MISS).sum())
    steps = [("gbuffer", lambda: ctx.gbuffer_device(region, stream=s.cuda_stream, **g)),
             ("cast", lambda: ctx.cast_rays_device(o, d, stream=s.cuda_stream, **out)),
             ("cast shuffled", lambda: ctx.cast_rays_device(so, sd, stream=s.cuda_stream, **out)),
             ("occluded", lambda: ctx.occluded_device(o, d, tmax, out=occ, stream=s.cuda_stream))]
    yard = None
    for name, call in steps:
        spans = cost.timed(s, call, warmup, repeats, launches=launches, hold_cycles=hold_cycles)   # (windows behind a held stream: cost._span has the reasons)
        ms = statistics.median(spans)
        yard = ms if name == "gbuffer" else yard
        cost.emit(TOOL, f"{tag} {name}", config=tag, scene=scene, size=[w, h], rays=n, hits=hits, what=name, **cost.summary(spans), mrays_per_s=round(n / ms / 1e3, 1),
                  times_gbuffer=round(ms / yard, 3), launches_per_window=launches, kernel=ctx.kernel_name())
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    ap.add_argument("--launches", type=int, default=20, help="calls per timed window; a figure is the window over this")
    ap.add_argument("--hold", type=int, default=40_000_000, help="device clock cycles the stream is held busy before a window, so that its calls queue up")
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "ray_query_cost.txt"))
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats, a.launches, a.hold)
    rows = cost.run_children(__file__, [[tag] for tag in cost.TAGS], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_ray_query_cost.py (median of {a.repeats} windows after {a.warmup} warm-ups, each {a.launches} queued calls between two events on the caller's stream, per call), one run on one MI355X"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + [json.dumps(row) for row in rows]) + "\n")


if __name__ == "__main__":
    main()
