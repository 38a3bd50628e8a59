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
configuration and spp runs in a child process of its own under a time limit (--limit seconds); the parent never opens the GPU and
stops at the first child that fails.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": ("example_project12_box.xml", 1920, 1080), "c5": ("trc_scene_tower.xml", 3840, 2160)}
SPPS = (4, 64)


def emission_twin(blob):
    """A copy of the blob in which every material emits its diffuse colour (texture included) and does nothing else"""
    from qaray_amd import hip
    twin = blob.copy()
    m = hip.blob_table(twin, "materials")
    m["emission"] = m["diffuse"]
    for k in ("diffuse", "specular", "reflection", "refraction"):
        m[k]["color"] = 0
    return twin


def measure(tag, spp, warmup, repeats):
    import torch
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    if not torch.cuda.is_available():
        raise SystemExit("gpu_matte_cost: no GPU (nothing is measured without one)")
    scene, w, h = CONFIGS[tag]
    dev = torch.device("cuda", 0)
    blob = load_scene_blob(os.path.join(SCENES_DIR, scene), size=(w, h))
    ctx, twin = hip.Context(0), hip.Context(0)
    ctx.upload_scene(blob)
    twin.upload_scene(emission_twin(blob))
    region = (0, 0, w, h)
    s = torch.cuda.Stream(dev)
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    ns = torch.empty((h, w), dtype=torch.int32, device=dev)
    m = ctx.matte_device(region, spp, stream=s.cuda_stream)
    rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    twin.render_region_device(region, spp, rgb, depth, ns, max_bounce=0, stream=s.cuda_stream)
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

    steps = [("twin frame", lambda: twin.render_region_device(region, spp, rgb, depth, ns, max_bounce=0, stream=s.cuda_stream)),
             ("matte all", lambda: ctx.matte_device(region, spp, stream=s.cuda_stream, **m)),
             ("matte coverage", lambda: ctx.matte_device(region, spp, coverage=m["coverage"], stream=s.cuda_stream)),
             ("rgba", lambda: ctx.rgba_device(rgb, m["backdrop"], m["coverage"], ns, out=rgba, stream=s.cuda_stream))]
    yard = None
    for name, call in steps:
        ms, lo, hi = timed(call)
        if name == "twin frame":
            yard = (ms, hi - lo)
        rec = {"config": tag, "scene": scene, "size": [w, h], "spp": spp, "what": name, "median_ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
               "share_of_twin_frame": round(ms / yard[0], 4), "library": os.path.relpath(hip.HIP_LIB_PATH, ROOT)}
        if name.startswith("matte"):
            rec["within"] = bool(ms <= yard[0] + yard[1])
        print(json.dumps(rec), flush=True)
    ctx.close()
    twin.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration's child process may take")
    ap.add_argument("--one", choices=sorted(CONFIGS), help="measure this configuration in this process (with --spp)")
    ap.add_argument("--spp", type=int, choices=SPPS)
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.spp or SPPS[0], a.warmup, a.repeats)
    for tag in sorted(CONFIGS):
        for spp in SPPS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", tag, "--spp", str(spp), "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                                   timeout=a.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"gpu_matte_cost: {tag} at {spp} spp did not finish in {a.limit} s; nothing more is started")
            if r.returncode != 0:
                raise SystemExit(f"gpu_matte_cost: {tag} at {spp} spp ended with {r.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
