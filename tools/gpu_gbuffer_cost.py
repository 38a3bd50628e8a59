#!/usr/bin/env python3
"""What the first-hit guide planes and the guided filter cost, on the frames of bench.py's C2 (Cornell box,
1920x1080) and C5 (trc_scene_tower.xml, 3840x2160): between two events on the caller's stream, warm-up calls, then the median of
--repeats, of
  gbuffer     Context.gbuffer_device, all four planes (36 bytes written per pixel)
  frame4      the 4-spp frame the preview shows (Context.render_region_device), the yardstick of 4g's last column
  guided N    Context.denoise_guided_device with both guides at N = 1, 3, 5 iterations, on that frame and those planes
  unguided N  Context.denoise_device on the same frame, for the difference
Every figure is also given as a share of the 4-spp frame.  Each configuration runs in a child process of its own under a time
limit (--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no fallback."""
import statistics
import sys

import cost

TOOL = "gpu_gbuffer_cost"
ITERATIONS = (1, 3, 5)


def measure(tag, warmup, repeats):
    ctx, _, region, dev, s = cost.open_scene(TOOL, tag)
    scene, w, h = cost.CONFIGS[tag]
    rgb, depth, ns = cost.frame_tensors(dev, w, h)
    out = rgb.new_empty(rgb.shape)
    g = ctx.gbuffer_device(region, stream=s.cuda_stream)
    s.synchronize()
    steps = [("frame4", lambda: ctx.render_region_device(region, 4, rgb, depth, ns, stream=s.cuda_stream)),
             ("gbuffer", lambda: ctx.gbuffer_device(region, stream=s.cuda_stream, **g))]
    for n in ITERATIONS:
        steps.append((f"guided {n}", lambda n=n: ctx.denoise_guided_device(rgb, depth, ns, g["normal"], g["albedo"], out=out, iterations=n, stream=s.cuda_stream)))
        steps.append((f"unguided {n}", lambda n=n: ctx.denoise_device(rgb, depth, ns, out=out, iterations=n, stream=s.cuda_stream)))
    frame = None
    for name, call in steps:
        spans = cost.timed(s, call, warmup, repeats)
        ms = statistics.median(spans)
        frame = ms if name == "frame4" else frame
        cost.emit(TOOL, f"{tag} {name}", config=tag, scene=scene, size=[w, h], what=name, **cost.summary(spans), share_of_4spp_frame=round(ms / frame, 4),
                  kernel=ctx.kernel_name())
    ctx.close()


def main():
    a = cost.arguments(__doc__, one=cost.TAGS).parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    cost.run_children(__file__, [[tag] for tag in cost.TAGS], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
