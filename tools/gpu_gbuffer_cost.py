#!/usr/bin/env python3
"""What the first-hit guide planes and the guided filter cost, on the frames of bench.py's C2 (Cornell box,
1920x1080) and C5 (trc_scene_tower.xml, 3840x2160): between two events on the caller's stream, warm-up calls, then the median of
--repeats, of
  gbuffer     Context.gbuffer_device, all four planes (36 bytes written per pixel)
  frame4      the 4-spp frame the preview shows (Context.render_region_device), the yardstick of 4g's last column
  guided N    Context.denoise_guided_device with both guides at N = 1, 3, 5 iterations, on that frame and those planes
  unguided N  Context.denoise_device on the same frame, for the difference
Every figure is also given as a share of the 4-spp frame.  Each configuration runs in a child process of its own under a time
limit (--limit seconds); the parent never opens the GPU and stops at the first child that fails.  Needs a GPU: there is no
fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": ("example_project12_box.xml", 1920, 1080), "c5": ("trc_scene_tower.xml", 3840, 2160)}
ITERATIONS = (1, 3, 5)


def measure(tag, warmup, repeats):
    import torch
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    if not torch.cuda.is_available():
        raise SystemExit("gpu_gbuffer_cost: no GPU (nothing is measured without one)")
    scene, w, h = CONFIGS[tag]
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    ctx.upload_scene(load_scene_blob(os.path.join(SCENES_DIR, scene), size=(w, h)))
    region = (0, 0, w, h)
    s = torch.cuda.Stream(dev)
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    ns = torch.empty((h, w), dtype=torch.int32, device=dev)
    out = torch.empty_like(rgb)
    g = ctx.gbuffer_device(region, stream=s.cuda_stream)
    s.synchronize()

    def timed(call):
        spans = []
        for _ in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                call()
                e1.record()
            s.synchronize()
            spans.append(e0.elapsed_time(e1))
        spans = spans[warmup:]
        return statistics.median(spans), min(spans), max(spans)

    steps = [("frame4", lambda: ctx.render_region_device(region, 4, rgb, depth, ns, stream=s.cuda_stream)),
             ("gbuffer", lambda: ctx.gbuffer_device(region, stream=s.cuda_stream, **g))]
    for n in ITERATIONS:
        steps.append((f"guided {n}", lambda n=n: ctx.denoise_guided_device(rgb, depth, ns, g["normal"], g["albedo"], out=out, iterations=n, stream=s.cuda_stream)))
        steps.append((f"unguided {n}", lambda n=n: ctx.denoise_device(rgb, depth, ns, out=out, iterations=n, stream=s.cuda_stream)))
    frame = None
    for name, call in steps:
        ms, lo, hi = timed(call)
        frame = ms if name == "frame4" else frame
        print(json.dumps({"config": tag, "scene": scene, "size": [w, h], "what": name, "median_ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                          "share_of_4spp_frame": round(ms / frame, 4), "kernel": ctx.kernel_name(), "library": os.path.relpath(hip.HIP_LIB_PATH, ROOT)}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration's child process may take")
    ap.add_argument("--one", choices=sorted(CONFIGS), help="measure this configuration in this process")
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    for tag in sorted(CONFIGS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", tag, "--warmup", str(a.warmup), "--repeats", str(a.repeats)], timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"gpu_gbuffer_cost: {tag} did not finish in {a.limit} s; nothing more is started")
        if r.returncode != 0:
            raise SystemExit(f"gpu_gbuffer_cost: {tag} ended with {r.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
