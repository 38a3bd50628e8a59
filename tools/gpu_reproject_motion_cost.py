#!/usr/bin/env python3
"""What following moved nodes and clamping stale history cost beside the plain reprojection:
Context.reproject_motion_device with its flags off, with QA_REPROJECT_MOTION, with QA_REPROJECT_CLAMP at radius 1 and 2, and with
both, beside Context.reproject_device on the same frames in the same process - the frames of tools/gpu_reproject_cost.py: bench.py's
C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml, 3840x2160) at 4 spp with ids, view 0 as the history and the view one degree
round the scene as the current frame.  The motion table marks every node but the root as moved, by a thousandth of a unit: every
hit pixel loads its record and is taken through it (the scene itself is not edited, so the history is found as before).

The variants take turns inside every repeat (old, off, motion, ...; then again), each call between two events on the caller's
stream: warm-up rounds, then the median of --repeats per variant and its ratio to the old call's.  The 4-spp frame is timed the
same way.  Each configuration runs in a child process of its own under a time limit (--limit seconds), by the rule of
tools/cost.py; the parent writes the table to --out.  Needs a GPU: there is no fallback."""
import os
import statistics

import cost
from gpu_reproject_cost import CONFIGS, main, two_views

TOOL = "gpu_reproject_motion_cost"
VARIANTS = ("old call", "flags off", "motion", "clamp r=1", "clamp r=2", "motion + clamp r=1")


def motion_table(hip, blob, dev):
    """Every node but the root moved by a thousandth of a unit -> the table on the host, its bytes on the device"""
    import torch
    inst = hip.blob_table(blob, "instances")
    nudged = inst.copy()
    nudged["pos"][1:] += 1e-3
    table_host = hip.node_motion(inst, nudged)
    return table_host, torch.from_numpy(table_host.view("u1")).to(dev)


def measure(tag, warmup, repeats):
    ctx, blob, region, dev, s = cost.open_scene(TOOL, tag)
    torch, hip = cost.gpu(TOOL)
    scene, w, h = CONFIGS[tag]
    cam0, cam1, (rgb0, depth0, ns0, ids0, _, _), (rgb1, depth1, ns1, ids1, _, _) = two_views(ctx, blob, region, s, dev)
    history = (rgb0, depth0, ns0.to(torch.float32))
    out, out_length = torch.empty_like(rgb1), torch.empty_like(depth1)
    table_host, table = motion_table(hip, blob, dev)
    torch.cuda.synchronize()
    common = dict(ids=ids1, hist_ids=ids0, out=out, out_length=out_length, stream=s.cuda_stream)

    def motion_call(**kw):
        return lambda: ctx.reproject_motion_device((rgb1, depth1, ns1), history, cam0, cam1, **common, **kw)

    calls = {"old call": lambda: ctx.reproject_device((rgb1, depth1, ns1), history, cam0, cam1, **common),
             "flags off": motion_call(), "motion": motion_call(motion=table), "clamp r=1": motion_call(clamp=True, clamp_radius=1),
             "clamp r=2": motion_call(clamp=True, clamp_radius=2), "motion + clamp r=1": motion_call(motion=table, clamp=True, clamp_radius=1),
             "4-spp frame": lambda: ctx.render_region_device(region, 4, rgb1, depth1, ns1, seed=2, stream=s.cuda_stream)}
    kept = {}

    def with_history(name):
        if name != "4-spp frame":
            kept[name] = float((out_length > ns1).float().mean())

    # (the frame last: it rewrites rgb1 with the same seed, so with the same bits)
    spans = cost.timed_turns(s, calls, (*VARIANTS, "4-spp frame"), warmup, repeats, after=with_history)
    frame_ms = statistics.median(spans["4-spp frame"])
    old_ms = statistics.median(spans["old call"])
    for name in VARIANTS:
        ms = statistics.median(spans[name])
        cost.emit(TOOL, f"{tag} {name}", config=tag, scene=scene, size=[w, h], variant=name, **cost.summary(spans[name]), ratio_to_old_call=round(ms / old_ms, 3),
                  frame4_ms=round(frame_ms, 4), share_of_4spp_frame=round(ms / frame_ms, 4), pixels_with_history=round(kept[name], 4),
                  nodes_moved=int(table_host["moved"].sum()), nodes=len(table_host))
    ctx.close()


def write_table(rows, out, warmup, repeats):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("tools/gpu_reproject_motion_cost.py: Context.reproject_motion_device beside Context.reproject_device (the old call), with ids, view 0 -> the\n"
                "view one degree round the scene, 4-spp frames; the motion table marks every node but the root as moved.\n"
                f"One run, one MI355X; the variants take turns, median of {repeats} after {warmup} warm-up rounds, each call between two events on the caller's\n"
                "stream; each configuration in its own process.  ratio: to the old call's median in the same process.\n\n")
        f.write(f"{'frame':<40}{'variant':<22}{'median ms (min - max)':<28}{'ratio':<8}{'4-spp frame ms':<16}{'share':<9}{'with history'}\n")
        for r in rows:
            name = f"{r['config']} {r['scene']} {r['size'][0]}x{r['size'][1]}"
            span = f"{r['median_ms']:.3f} ({r['min_ms']:.3f} - {r['max_ms']:.3f})"
            f.write(f"{name:<40}{r['variant']:<22}{span:<28}{r['ratio_to_old_call']:<8.3f}{r['frame4_ms']:<16.3f}{r['share_of_4spp_frame']:<9.4f}"
                    f"{r['pixels_with_history']:.4f}\n")
        for tag in sorted({r["config"] for r in rows}):
            r = next(x for x in rows if x["config"] == tag)
            f.write(f"\n{tag}: {r['nodes_moved']} of {r['nodes']} nodes moved in the table; library {r['library']}")
        f.write("\n")


if __name__ == "__main__":
    main(__file__, __doc__, measure, write_table, repeats=9)
