#!/usr/bin/env python3
"""What following moved nodes and clamping stale history cost beside the plain reprojection:
Context.reproject_motion_device with its flags off, with QA_REPROJECT_MOTION, with QA_REPROJECT_CLAMP at radius 1 and 2, and with
both, beside Context.reproject_device on the same frames in the same process - the frames of tools/gpu_reproject_cost.py: bench.py's
C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml, 3840x2160) at 4 spp with ids, view 0 as the history and the view one degree
round the scene as the current frame.  The motion table marks every node but the root as moved, by a thousandth of a unit: every
hit pixel loads its record and is taken through it (the scene itself is not edited, so the history is found as before).

The variants take turns inside every repeat (old, off, motion, ...; then again), each call between two events on the caller's
stream: warm-up rounds, then the median of --repeats per variant and its ratio to the old call's.  The 4-spp frame is timed the
same way.  Each configuration runs in a child process of its own under a time limit (--limit seconds); the parent never opens the
GPU, stops at the first child that fails and writes the table to --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_reproject_cost import CONFIGS, turned   # noqa: E402

VARIANTS = ("old call", "flags off", "motion", "clamp r=1", "clamp r=2", "motion + clamp r=1")


def measure(tag, warmup, repeats):
    import torch
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    if not torch.cuda.is_available():
        raise SystemExit("gpu_reproject_motion_cost: no GPU (nothing is measured without one)")
    scene, w, h = CONFIGS[tag]
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    blob = load_scene_blob(os.path.join(SCENES_DIR, scene), size=(w, h))
    ctx.upload_scene(blob)
    region = (0, 0, w, h)
    s = torch.cuda.Stream(dev)

    def frame(seed):
        rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((h, w), dtype=torch.float32, device=dev)
        ns = torch.empty((h, w), dtype=torch.int32, device=dev)
        ids = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=seed, stream=s.cuda_stream)
        ctx.gbuffer_device(region, seed, ids=ids, stream=s.cuda_stream)
        s.synchronize()
        return rgb, depth, ns, ids

    cam0 = hip.blob_camera(blob).copy()
    rgb0, depth0, ns0, ids0 = frame(1)
    hits = depth0[depth0 < 1e29]
    cam1 = turned(cam0, w, h, float(hits.median()) if hits.numel() else 1.0, 1.0)
    ctx.edit_camera(cam1)
    rgb1, depth1, ns1, ids1 = frame(2)
    history = (rgb0, depth0, ns0.to(torch.float32))
    out, out_length = torch.empty_like(rgb1), torch.empty_like(depth1)
    inst = hip.blob_table(blob, "instances")
    nudged = inst.copy()
    nudged["pos"][1:] += 1e-3
    table_host = hip.node_motion(inst, nudged)
    table = torch.from_numpy(table_host.view("u1")).to(dev)
    torch.cuda.synchronize()
    common = dict(ids=ids1, hist_ids=ids0, out=out, out_length=out_length, stream=s.cuda_stream)

    def motion_call(**kw):
        return lambda: ctx.reproject_motion_device((rgb1, depth1, ns1), history, cam0, cam1, **common, **kw)

    calls = {"old call": lambda: ctx.reproject_device((rgb1, depth1, ns1), history, cam0, cam1, **common),
             "flags off": motion_call(), "motion": motion_call(motion=table), "clamp r=1": motion_call(clamp=True, clamp_radius=1),
             "clamp r=2": motion_call(clamp=True, clamp_radius=2), "motion + clamp r=1": motion_call(motion=table, clamp=True, clamp_radius=1),
             "4-spp frame": lambda: ctx.render_region_device(region, 4, rgb1, depth1, ns1, seed=2, stream=s.cuda_stream)}
    spans = {k: [] for k in calls}
    kept = {}
    for i in range(warmup + repeats):
        for name in (*VARIANTS, "4-spp frame"):    # (the frame last: it rewrites rgb1 with the same seed, so with the same bits)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                calls[name]()
                e1.record()
            s.synchronize()
            if i >= warmup:
                spans[name].append(e0.elapsed_time(e1))
            if name != "4-spp frame":
                kept[name] = float((out_length > ns1).float().mean())
    frame_ms = statistics.median(spans["4-spp frame"])
    old_ms = statistics.median(spans["old call"])
    for name in VARIANTS:
        ms = statistics.median(spans[name])
        print(json.dumps({"config": tag, "scene": scene, "size": [w, h], "variant": name, "median_ms": round(ms, 4), "min_ms": round(min(spans[name]), 4),
                          "max_ms": round(max(spans[name]), 4), "ratio_to_old_call": round(ms / old_ms, 3), "frame4_ms": round(frame_ms, 4),
                          "share_of_4spp_frame": round(ms / frame_ms, 4), "pixels_with_history": round(kept[name], 4),
                          "nodes_moved": int(table_host["moved"].sum()), "nodes": len(table_host), "library": os.path.relpath(hip.HIP_LIB_PATH, ROOT)}),
              flush=True)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_motion_cost.txt"))
    ap.add_argument("--one", choices=sorted(CONFIGS), help="measure this configuration in this process")
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    rows = []
    for tag in sorted(CONFIGS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", tag, "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                               timeout=a.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"gpu_reproject_motion_cost: {tag} did not finish in {a.limit} s; nothing more is started")
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            raise SystemExit(f"gpu_reproject_motion_cost: {tag} ended with {r.returncode}; nothing more is started")
        rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    write_table(rows, a.out, a.warmup, a.repeats)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
