#!/usr/bin/env python3
"""What reflection probes cost, on the workload of profiles/probe_cost.txt and against the calls they follow, on the same
build and in the same run.  Each configuration in a child process of its own under a time limit (--limit seconds), by the rule of
tools/cost.py:
  c2, c5      the scenes of bench.py's C2 (Cornell box) and C5 (trc_scene_tower.xml), cooperative walks off.  The 16 x 16 x 16 grid of
              tools/gpu_probe_cost.py, m = 16, 1 sample, a chain of L = 5 levels.  The two calls take turns inside every repeat, each
              between two events on one caller's stream:
                probe_sh_cube   Context.probe_sh_device(cube=...) on the grid's points: the bake the prefilter follows
                prefilter       Context.reflprobe_prefilter_device on that cube: 4096 probes x 510 filtered texels x 1536 source
                                texels = 3.21 G pairs, and the copy of level 0
              then, taking turns likewise, at 1920 x 1080 points spread over the grid's box and half a cell around it, unit directions
              and levels uniform in [0, 4]:
                shade           ProbeGrid.shade_device: the yardstick (the diffuse lookup of the same grid)
                reflect         ProbeGrid.reflect_device: the glossy lookup
After warm-up rounds, the median, minimum and maximum of --repeats rounds.  The prefilter is set beside the bake as a ratio, and
beside its VALU floor: the pairs times the vector instructions a pair takes in the kept gfx950 assembly of the level-1 pair loop
(PAIR_VALU below, counted by hand in qa_reflprobe-hip-amdgcn-amd-amdhsa-gfx950.s), over 256 CUs x 64 lanes at 2.4 GHz; the guide's four
SIMD-32 per CU retire 128 lanes a clock, so the share of that stricter floor is half the one reported and is given beside it.
reflect is set against shade by the band rule of tools/cost.py.  Nothing is fixed in advance: the rows are the measurement.
The lines are printed and written to --out (default profiles/reflprobe_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import numpy as np

import cost
from gpu_probe_cost import GRID, M, SHADE, first_hits
from gpu_probevis_cost import against

TOOL = "gpu_reflprobe_cost"
LEVELS = 5
# the level-1 loop (five squarings) of qa_reflprobe_prefilter, per pair: the two address moves of the record read ahead, the dot
# product (3 multiplies, 2 adds), the clamp, 5 squarings, the compare - 14 - and under the lanes' mask q and the four accumulators
# (4 multiplies, 4 adds), issued whether or not a lane's lobe is 0
PAIR_VALU = 22
LANES_PER_CLOCK = 256 * 64
CLOCK_HZ = 2.4e9


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
    lay = hip.reflprobe_layout(M, LEVELS)
    pairs = n * (lay["texels"] - K) * K
    with torch.cuda.stream(s):
        tp = torch.from_numpy(grid.points()).to(dev)
        sh, hits, tmin = torch.empty((n, 9, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
        cube = torch.empty((n, 6, M, M, 3), device=dev)
        chain = torch.empty((n, lay["texels"], 3), device=dev)
    s.synchronize()
    calls = {"probe_sh_cube": lambda: ctx.probe_sh_device(tp, M, 1, sh=sh, cube=cube, hits=hits, tmin=tmin, stream=s.cuda_stream),
             "prefilter": lambda: ctx.reflprobe_prefilter_device(cube, LEVELS, chain=chain, stream=s.cuda_stream)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    bake = statistics.median(spans["probe_sh_cube"])
    for name, span in spans.items():
        ms = statistics.median(span)
        more = {}
        if name == "prefilter":
            floor_ms = pairs * PAIR_VALU / (LANES_PER_CLOCK * CLOCK_HZ) * 1e3
            more = {"levels": LEVELS, "pairs": pairs, "gpairs_per_s": round(pairs / ms / 1e6, 1), "times_bake": round(ms / bake, 3), "valu_per_pair": PAIR_VALU,
                    "valu_floor_ms": round(floor_ms, 4), "share_of_floor": round(floor_ms / ms, 3), "share_at_128_lanes_per_cu": round(0.5 * floor_ms / ms, 3)}
        cost.emit(TOOL, f"{tag} grid {name}", config=tag, scene=scene, probes=n, m=M, what=name, **cost.summary(span), **more)
    # the lookups a viewer calls every frame
    grid.sh, grid.hits, grid.tmin, grid.chain, grid.m, grid.levels = sh, hits, tmin, chain, M, LEVELS
    npts = SHADE[0] * SHADE[1]
    with torch.cuda.stream(s):
        g = torch.Generator(device=dev).manual_seed(1)
        span_ = torch.from_numpy((grid.spacing * (GRID - 1)).astype(np.float32)).to(dev)
        at = torch.from_numpy(grid.origin - 0.5 * grid.spacing).to(dev) + torch.rand((npts, 3), device=dev, generator=g) * (span_ + torch.from_numpy(grid.spacing).to(dev))
        nr = torch.nn.functional.normalize(torch.randn((npts, 3), device=dev, generator=g), dim=1).contiguous()
        level = (torch.rand((npts,), device=dev, generator=g) * (LEVELS - 1)).contiguous()
        at = at.contiguous()
        out = torch.empty((npts, 3), device=dev)
    s.synchronize()
    calls = {"shade": lambda: grid.shade_device(at, nr, out=out, stream=s.cuda_stream),
             "reflect": lambda: grid.reflect_device(at, nr, level, out=out, stream=s.cuda_stream)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    for name, span in spans.items():
        ms = statistics.median(span)
        more = against(spans["shade"], span) if name != "shade" else {}
        cost.emit(TOOL, f"{tag} grid {name}", config=tag, scene=scene, probes=n, points=list(SHADE),
                  what="ProbeGrid.reflect_device" if name == "reflect" else "ProbeGrid.shade_device", **cost.summary(span),
                  ns_per_point=round(ms * 1e6 / npts, 4), mpoints_per_s=round(npts / ms / 1e3, 1), **more)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "reflprobe_cost.txt"))
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    cost.assets()
    rows = cost.run_children(__file__, [[tag] for tag in cost.TAGS], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_reflprobe_cost.py (median, minimum and maximum of {a.repeats} rounds after {a.warmup} warm-up rounds; the calls of a pair take turns "
             f"inside a round, each between two events on one caller's stream), a {GRID}^3 grid at m = {M}, L = {LEVELS}, 1 spp, coop 0, one run on one MI355X"]
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
