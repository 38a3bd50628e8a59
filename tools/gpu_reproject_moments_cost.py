#!/usr/bin/env python3
"""What the moments, the shortened length and the variance plane cost beside the calls they extend, on the frames of
tools/gpu_reproject_cost.py: bench.py's C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml, 3840x2160) at 4 spp with ids, view
0 as the history and the view one degree round the scene as the current frame, the motion table of tools/gpu_reproject_motion_cost.py
(every node but the root moved by a thousandth of a unit).

Reprojection: Context.reproject_motion_device (motion + clamp, r = 1), the yardstick, then Context.reproject_moments_device with
the new flags off, with QA_REPROJECT_MOMENTS, and with QA_REPROJECT_MOMENTS | QA_REPROJECT_SHORTEN (the history's moments plane is
the history's luma and its square).  Filter, at 5 iterations with both guides: Context.denoise_guided_device, the yardstick, then
Context.denoise_variance_device with the variance plane the reprojection wrote.

The variants take turns inside every repeat, each call between two events on the caller's stream: warm-up rounds, then the median
of --repeats per variant and its ratio to its yardstick's in the same process.  Each configuration runs in a child process of its own
under a time limit (--limit seconds), by the rule of tools/cost.py; the parent writes the table to --out.  Needs a GPU: there is no
fallback."""
import os
import statistics

import cost
from gpu_reproject_cost import CONFIGS, main, two_views
from gpu_reproject_motion_cost import motion_table

TOOL = "gpu_reproject_moments_cost"
REPROJECT = ("motion call", "new flags off", "moments", "moments + shorten")
FILTER = ("guided filter", "variance filter")


def measure(tag, warmup, repeats):
    ctx, blob, region, dev, s = cost.open_scene(TOOL, tag)
    torch, hip = cost.gpu(TOOL)
    scene, w, h = CONFIGS[tag]
    new = lambda shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    cam0, cam1, (rgb0, depth0, ns0, ids0, _, _), (rgb1, depth1, ns1, ids1, normal1, albedo1) = two_views(ctx, blob, region, s, dev, guides=True)
    history = (rgb0, depth0, 4 * ns0.to(torch.float32))     # (four frames behind every pixel: the variance is trusted)
    luma0 = 0.2126 * rgb0[..., 0] + 0.7152 * rgb0[..., 1] + 0.0722 * rgb0[..., 2]
    hist_moments = torch.stack([luma0, luma0 * luma0 + 0.01], dim=-1).contiguous()
    out, out_length, out_moments, out_variance, filtered = new((h, w, 3)), new((h, w)), new((h, w, 2)), new((h, w)), new((h, w, 3))
    _, table = motion_table(hip, blob, dev)
    torch.cuda.synchronize()
    common = dict(ids=ids1, hist_ids=ids0, motion=table, clamp=True, clamp_radius=1, out=out, out_length=out_length, stream=s.cuda_stream)

    def moments_call(**kw):
        return lambda: ctx.reproject_moments_device((rgb1, depth1, ns1), history, cam0, cam1, hist_moments=hist_moments, out_moments=out_moments,
                                                    out_variance=out_variance, **common, **kw)

    calls = {"motion call": lambda: ctx.reproject_motion_device((rgb1, depth1, ns1), history, cam0, cam1, **common),
             "new flags off": moments_call(), "moments": moments_call(moments=True), "moments + shorten": moments_call(moments=True, shorten=True),
             "guided filter": lambda: ctx.denoise_guided_device(out, depth1, ns1, normal1, albedo1, out=filtered, iterations=5, stream=s.cuda_stream),
             "variance filter": lambda: ctx.denoise_variance_device(out, depth1, ns1, normal1, albedo1, out_variance, out=filtered, iterations=5,
                                                                    stream=s.cuda_stream)}
    trusted = [0.0]

    def trust(name):
        if name == "moments + shorten":
            trusted[0] = float((out_variance >= 0).float().mean())

    # (the filters last: they read the planes "moments + shorten" has just written)
    spans = cost.timed_turns(s, calls, (*REPROJECT, *FILTER), warmup, repeats, after=trust)
    for group in (REPROJECT, FILTER):
        base = statistics.median(spans[group[0]])
        for name in group:
            ms = statistics.median(spans[name])
            cost.emit(TOOL, f"{tag} {name}", config=tag, scene=scene, size=[w, h], variant=name, yardstick=group[0], **cost.summary(spans[name]),
                      ratio=round(ms / base, 3), pixels_trusted=round(trusted[0], 4))
    ctx.close()


def write_table(rows, out, warmup, repeats):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("tools/gpu_reproject_moments_cost.py: Context.reproject_moments_device beside Context.reproject_motion_device (motion + clamp, r = 1), and\n"
                "Context.denoise_variance_device beside Context.denoise_guided_device (5 iterations, both guides), with ids, view 0 -> the view one degree\n"
                f"round the scene, 4-spp frames.  One run, one MI355X; the variants take turns, median of {repeats} after {warmup} warm-up rounds, each call\n"
                "between two events on the caller's stream; each configuration in its own process.  ratio: to the yardstick's median in the same process.\n\n")
        f.write(f"{'frame':<40}{'variant':<22}{'median ms (min - max)':<28}{'ratio':<8}{'yardstick':<16}{'trusted pixels'}\n")
        for r in rows:
            name = f"{r['config']} {r['scene']} {r['size'][0]}x{r['size'][1]}"
            span = f"{r['median_ms']:.3f} ({r['min_ms']:.3f} - {r['max_ms']:.3f})"
            f.write(f"{name:<40}{r['variant']:<22}{span:<28}{r['ratio']:<8.3f}{r['yardstick']:<16}{r['pixels_trusted']:.4f}\n")
        f.write(f"\nlibrary {rows[0]['library']}\n" if rows else "\n")


if __name__ == "__main__":
    main(__file__, __doc__, measure, write_table, repeats=9)
