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
under a time limit (--limit seconds); the parent never opens the GPU, stops at the first child that fails and writes the table to
--out.  Needs a GPU: there is no fallback."""
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

REPROJECT = ("motion call", "new flags off", "moments", "moments + shorten")
FILTER = ("guided filter", "variance filter")


def measure(tag, warmup, repeats):
    import torch
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    if not torch.cuda.is_available():
        raise SystemExit("gpu_reproject_moments_cost: no GPU (nothing is measured without one)")
    scene, w, h = CONFIGS[tag]
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    blob = load_scene_blob(os.path.join(SCENES_DIR, scene), size=(w, h))
    ctx.upload_scene(blob)
    region = (0, 0, w, h)
    s = torch.cuda.Stream(dev)
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731

    def frame(seed, guides=False):
        rgb, depth, ns, ids = new((h, w, 3)), new((h, w)), new((h, w), torch.int32), new((h, w, 2), torch.int32)
        normal, albedo = (new((h, w, 3)), new((h, w, 3))) if guides else (None, None)
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=seed, stream=s.cuda_stream)
        ctx.gbuffer_device(region, seed, normal=normal, albedo=albedo, ids=ids, stream=s.cuda_stream)
        s.synchronize()
        return rgb, depth, ns, ids, normal, albedo

    cam0 = hip.blob_camera(blob).copy()
    rgb0, depth0, ns0, ids0, _, _ = frame(1)
    hits = depth0[depth0 < 1e29]
    cam1 = turned(cam0, w, h, float(hits.median()) if hits.numel() else 1.0, 1.0)
    ctx.edit_camera(cam1)
    rgb1, depth1, ns1, ids1, normal1, albedo1 = frame(2, guides=True)
    history = (rgb0, depth0, 4 * ns0.to(torch.float32))     # (four frames behind every pixel: the variance is trusted)
    luma0 = 0.2126 * rgb0[..., 0] + 0.7152 * rgb0[..., 1] + 0.0722 * rgb0[..., 2]
    hist_moments = torch.stack([luma0, luma0 * luma0 + 0.01], dim=-1).contiguous()
    out, out_length, out_moments, out_variance, filtered = new((h, w, 3)), new((h, w)), new((h, w, 2)), new((h, w)), new((h, w, 3))
    inst = hip.blob_table(blob, "instances")
    nudged = inst.copy()
    nudged["pos"][1:] += 1e-3
    table_host = hip.node_motion(inst, nudged)
    table = torch.from_numpy(table_host.view("u1")).to(dev)
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
    spans = {k: [] for k in calls}
    trusted = 0.0
    for i in range(warmup + repeats):
        for name in (*REPROJECT, *FILTER):    # (the filters last: they read the planes "moments + shorten" has just written)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                calls[name]()
                e1.record()
            s.synchronize()
            if i >= warmup:
                spans[name].append(e0.elapsed_time(e1))
            if name == "moments + shorten":
                trusted = float((out_variance >= 0).float().mean())
    for group in (REPROJECT, FILTER):
        base = statistics.median(spans[group[0]])
        for name in group:
            ms = statistics.median(spans[name])
            print(json.dumps({"config": tag, "scene": scene, "size": [w, h], "variant": name, "yardstick": group[0], "median_ms": round(ms, 4),
                              "min_ms": round(min(spans[name]), 4), "max_ms": round(max(spans[name]), 4), "ratio": round(ms / base, 3),
                              "pixels_trusted": round(trusted, 4), "library": os.path.relpath(hip.HIP_LIB_PATH, ROOT)}), flush=True)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_moments_cost.txt"))
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
            raise SystemExit(f"gpu_reproject_moments_cost: {tag} did not finish in {a.limit} s; nothing more is started")
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            raise SystemExit(f"gpu_reproject_moments_cost: {tag} ended with {r.returncode}; nothing more is started")
        rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    write_table(rows, a.out, a.warmup, a.repeats)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
