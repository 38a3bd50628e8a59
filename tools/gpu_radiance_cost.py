#!/usr/bin/env python3
"""What the radiance queries cost, on the frames of bench.py's C2 (Cornell box, 1920x1080) and C5
(trc_scene_tower.xml, 3840x2160) at 16 samples per pixel, cooperative walks off: windows of --launches calls queued back to back
between two events on the caller's stream (the stream is held busy while the host enqueues them, so a window holds device time
only), warm-up windows, then the median, minimum and maximum of --repeats windows, per call, of
  frame           Context.render_region_device: the yardstick.  With --parent DIR also `frame (parent)`: the same call in a process
                  of its own that imports the package of DIR, a built checkout of the parent commit - the ratios are to that row
  radiance        Context.radiance_rays_device of that frame's own camera_sample_rays_device (all outputs, rays per sample)
  radiance shuffled  the same rays, pixel by pixel, in a fixed random permutation: what divergence costs
Every figure in milliseconds and Msamples/s, and as a multiple of the yardstick.  Each configuration runs in a child process of
its own under a time limit (--limit seconds), by the rule of tools/cost.py.  The lines are printed and written to --out (default
profiles/radiance_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import cost

TOOL = "gpu_radiance_cost"
SPP = 16


def measure(tag, warmup, repeats, launches, hold_cycles, frame_only, root):
    # (the package of the parent checkout for its row, else this tree's)
    ctx, _, region, dev, s = cost.open_scene(TOOL, tag, root=root, options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL, root)
    scene, w, h = cost.CONFIGS[tag]
    n = w * h
    with torch.cuda.stream(s):
        rgb = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
        ns = torch.zeros((h, w), dtype=torch.int32, device=dev)
        ctx.render_region_device(region, SPP, rgb, depth, ns, stream=s.cuda_stream)
    s.synchronize()
    kernel = ctx.kernel_name()
    steps = [("frame (parent)" if frame_only else "frame", lambda: ctx.render_region_device(region, SPP, rgb, depth, ns, stream=s.cuda_stream))]
    bytes_per_sample = 0
    if not frame_only:
        with torch.cuda.stream(s):
            rays = ctx.camera_sample_rays_device(region, 0, SPP, stream=s.cuda_stream)
            perm = torch.randperm(n, device=dev, generator=torch.Generator(dev).manual_seed(20250131))
            shuffled = {k: v[perm].contiguous() for k, v in rays.items()}
            out = (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev))
        s.synchronize()
        bytes_per_sample = sum(v.element_size() * v[0].numel() // SPP for k, v in rays.items() if k != "stream_ids")

        def radiance(r):
            return lambda: ctx.radiance_rays_device(r["origins"], r["dirs"], spp=SPP, dx=r["dx"], dy=r["dy"], screen=r["screen"], stream_ids=r["stream_ids"],
                                                    rgb=out[0], t=out[1], ns=out[2], stream=s.cuda_stream)
        steps += [("radiance", radiance(rays)), ("radiance shuffled", radiance(shuffled))]
    for name, call in steps:
        spans = cost.timed(s, call, warmup, repeats, launches=launches, hold_cycles=hold_cycles)   # (windows behind a held stream: cost._span has the reasons)
        ms = statistics.median(spans)
        cost.emit(TOOL, f"{tag} {SPP} spp {name}", config=tag, scene=scene, size=[w, h], spp=SPP, what=name, **cost.summary(spans),
                  msamples_per_s=round(n * SPP / ms / 1e3, 1), ray_bytes_per_sample=bytes_per_sample, launches_per_window=launches, kernel=kernel,
                  tree="parent" if frame_only else "this", library=cost.library(root))
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    ap.add_argument("--launches", type=int, default=3, help="calls per timed window; a figure is the window over this")
    ap.add_argument("--hold", type=int, default=40_000_000, help="device clock cycles the stream is held busy before a window, so that its calls queue up")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its frame is the yardstick")
    ap.add_argument("--root", default=cost.ROOT, help="with --one: the tree whose package is imported")
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "radiance_cost.txt"))
    ap.add_argument("--frame-only", action="store_true", help="with --one: the frame row alone (the parent library's child)")
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats, a.launches, a.hold, a.frame_only, os.path.abspath(a.root))
    for root in [cost.ROOT] + ([a.parent] if a.parent else []):   # the stand-in meshes of C5, in each tree's own scenes
        cost.assets(root)
    lines = [f"# tools/gpu_radiance_cost.py (median of {a.repeats} windows after {a.warmup} warm-ups, each {a.launches} queued calls between two events on the caller's stream, per call), "
             f"{SPP} spp, coop 0, one run on one MI355X"]
    for tag in cost.TAGS:
        rows = cost.run_children(__file__, ([[tag, "--frame-only", "--root", a.parent]] if a.parent else []) + [[tag]], sys.argv[1:], a.limit, through=False)
        yard = rows[0]["median_ms"]   # the parent's frame when there is one, else this library's
        for row in rows:
            row["times_" + rows[0]["what"].replace(" ", "_").replace("(", "").replace(")", "")] = round(row["median_ms"] / yard, 3)
            row.update(tool=row.pop("tool"), id=row.pop("id"))   # (they stay last)
            print(json.dumps(row), flush=True)
            lines.append(json.dumps(row))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
