#!/usr/bin/env python3
"""What probe visibility costs, on the workload of profiles/probe_cost.txt and against the calls it extends, on the same
build and in the same run.  Each configuration in a child process of its own under a time limit (--limit seconds), by the rule of
tools/cost.py:
  c2, c5      the scenes of bench.py's C2 (Cornell box) and C5 (trc_scene_tower.xml), cooperative walks off.  The 16 x 16 x 16 grid of
              tools/gpu_probe_cost.py (over the middle half of the box around the first hits of a 64 x 48 frame's camera rays), m = 16,
              1 sample, d = 8, dmax = 1.5 |spacing|.  The two bakes take turns inside every repeat, each between two events on one
              caller's stream:
                probe_sh      Context.probe_sh_device on the grid's points: the yardstick
                probevis_sh   Context.probevis_sh_device on them: what the moments add to a bake
              then, taking turns likewise, at 1920 x 1080 points spread over the grid's box and half a cell around it, unit normals:
                shade         ProbeGrid.shade_device: the yardstick
                shade_vis     ProbeGrid.shade_device(visibility=True): what the visibility costs per point
After warm-up rounds, the median, minimum and maximum of --repeats rounds.  Two numbers are called different by the band rule of
tools/cost.py (tools/cost_ab.py's): the new call's median against the yardstick's min - max range of the same run, or 3 % around its
median where that range is narrower; the row says inside, above or below.  Nothing is fixed in advance: the rows are the measurement.
The lines are printed and written to --out (default profiles/probevis_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import numpy as np

import cost
from gpu_probe_cost import GRID, M, SHADE, first_hits

TOOL = "gpu_probevis_cost"
D = 8


def against(yard, span):
    """The band rule for one yardstick and one new call of the same run -> fields of the new call's row"""
    one = lambda t: [(statistics.median(t), min(t), max(t))]   # noqa: E731
    b = cost.band(one(yard), one(span))
    return {"times_yardstick": round(b["new_median"] / b["parent_median"], 3), "band": [round(b["allowed"][0], 4), round(b["allowed"][1], 4)],
            "band_kind": b["kind"], "verdict": b["verdict"]}


def measure(tag, warmup, repeats):
    scene = cost.CONFIGS[tag][0]
    ctx, _, region, dev, s = cost.open_scene(TOOL, (scene, 64, 48), options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL)
    with torch.cuda.stream(s):
        p, _, ok = first_hits(ctx, torch, dev, region, s)
    s.synchronize()
    p = p[ok].cpu().numpy().astype(np.float64)
    lo, hi = np.percentile(p, 10, axis=0), np.percentile(p, 90, axis=0)
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    grid = hip.ProbeGrid(ctx, mid - half, np.maximum(2 * half / (GRID - 1), 1e-3), (GRID,) * 3)
    n, K = grid.probes, 6 * M * M
    dmax = float(np.float32(1.5) * np.sqrt((grid.spacing * grid.spacing).sum(dtype=np.float32)))
    with torch.cuda.stream(s):
        tp = torch.from_numpy(grid.points()).to(dev)
        sh, hits, tmin = torch.empty((n, 9, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
        mo = torch.empty((n, 6, D, D, 2), device=dev)
    s.synchronize()
    calls = {"probe_sh": lambda: ctx.probe_sh_device(tp, M, 1, sh=sh, hits=hits, tmin=tmin, stream=s.cuda_stream),
             "probevis_sh": lambda: ctx.probevis_sh_device(tp, D, dmax, M, 1, sh=sh, hits=hits, tmin=tmin, moments=mo, stream=s.cuda_stream)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    for name, span in spans.items():
        ms = statistics.median(span)
        more = against(spans["probe_sh"], span) if name != "probe_sh" else {}
        cost.emit(TOOL, f"{tag} grid {name}", config=tag, scene=scene, probes=n, m=M, d=D, rays=n * K, spp=1, what=name, **cost.summary(span),
                  mrays_per_s=round(n * K / ms / 1e3, 1), **more)
    # the evaluation a viewer calls every frame
    grid.sh, grid.hits, grid.tmin, grid.moments, grid.d, grid.dmax = sh, hits, tmin, mo, D, np.float32(dmax)
    npts = SHADE[0] * SHADE[1]
    with torch.cuda.stream(s):
        g = torch.Generator(device=dev).manual_seed(1)
        span_ = torch.from_numpy((grid.spacing * (GRID - 1)).astype(np.float32)).to(dev)
        at = torch.from_numpy(grid.origin - 0.5 * grid.spacing).to(dev) + torch.rand((npts, 3), device=dev, generator=g) * (span_ + torch.from_numpy(grid.spacing).to(dev))
        nr = torch.nn.functional.normalize(torch.randn((npts, 3), device=dev, generator=g), dim=1).contiguous()
        at = at.contiguous()
        out = torch.empty((npts, 3), device=dev)
    s.synchronize()
    calls = {"shade": lambda: grid.shade_device(at, nr, out=out, stream=s.cuda_stream),
             "shade_vis": lambda: grid.shade_device(at, nr, out=out, stream=s.cuda_stream, visibility=True)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    for name, span in spans.items():
        ms = statistics.median(span)
        more = against(spans["shade"], span) if name != "shade" else {}
        cost.emit(TOOL, f"{tag} grid {name}", config=tag, scene=scene, probes=n, d=D, points=list(SHADE),
                  what="ProbeGrid.shade_device" + ("(visibility=True)" if name == "shade_vis" else ""), **cost.summary(span),
                  ns_per_point=round(ms * 1e6 / npts, 4), mpoints_per_s=round(npts / ms / 1e3, 1), **more)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "probevis_cost.txt"))
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    cost.assets()
    rows = cost.run_children(__file__, [[tag] for tag in cost.TAGS], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_probevis_cost.py (median, minimum and maximum of {a.repeats} rounds after {a.warmup} warm-up rounds; the yardstick and the new call "
             f"take turns inside a round, each between two events on one caller's stream), a {GRID}^3 grid at m = {M}, d = {D}, 1 spp, coop 0, one run on one MI355X"]
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
