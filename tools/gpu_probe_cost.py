#!/usr/bin/env python3
"""What the light probes cost.  Each configuration in a child process of its own under a time limit (--limit seconds),
by the rule of tools/cost.py:
  c2, c5      the scenes of bench.py's C2 (Cornell box) and C5 (trc_scene_tower.xml), cooperative walks off.  A 16 x 16 x 16 grid of
              probes over the middle half of the box around the first hits of a 64 x 48 frame's camera rays, m = 16 (1 536 rays per
              probe, 6.3 M rays), 1 sample.  The calls take turns inside every repeat, each between two events on one caller's stream:
                probe_sh     Context.probe_sh_device on the grid's points (default chunks)
                radiance     Context.radiance_rays_device on the same rays, built beforehand (probe_directions_host, the streams
                             S * K + k, miss_environment): the yardstick - the ratio is what ray generation, the scratch traffic and
                             the projection add
              then ProbeGrid.shade_device at 1920 x 1080 points spread over the grid's box and half a cell around it, unit normals:
              ms, and GB/s against the 36 bytes per point it must move (point, normal, rgb; the 442 KB of coefficients stay cached).
  accuracy    the Cornell box at 64 x 48: at the hits of the frame's first camera rays, probes 0.01 * N off the surface (N the normal
              turned towards the camera; m = 16, 16 samples) shaded with N by probe_shade_device, against irradiance_points_device at
              the hits (256 samples): the relative RMS difference over all channels.  Not a bound: the size of the order-2 truncation
              plus the difference between starting at the surface and 0.01 above it.
After warm-up rounds, the median, minimum and maximum of --repeats rounds.  Nothing is fixed in advance: the rows are the measurement.
The lines are printed and written to --out (default profiles/probe_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import numpy as np

import cost

TOOL = "gpu_probe_cost"
GRID, M = 16, 16
SHADE = (1920, 1080)


def first_hits(ctx, torch, dev, region, s):
    """-> (points, facing normals, hit mask) of the region's first camera rays, tensors"""
    n = (region[2] - region[0]) * (region[3] - region[1])
    rays = ctx.camera_sample_rays_device(region, 0, 1, outputs=("origins", "dirs"), stream=s.cuda_stream)
    o, d = rays["origins"].reshape(n, 3), rays["dirs"].reshape(n, 3)
    hit = ctx.cast_rays_device(o, d, t=torch.empty(n, device=dev), normal=torch.empty((n, 3), device=dev), point=torch.empty((n, 3), device=dev),
                               stream=s.cuda_stream)
    normals = (-hit["normal"] * torch.sign((hit["normal"] * d).sum(dim=1, keepdim=True))).contiguous()
    return hit["point"], normals, hit["t"] < 1e30


def measure_grid(tag, warmup, repeats):
    scene = cost.CONFIGS[tag][0]
    ctx, _, region, dev, s = cost.open_scene(TOOL, (scene, 64, 48), options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL)
    with torch.cuda.stream(s):
        p, _, ok = first_hits(ctx, torch, dev, region, s)
    s.synchronize()
    p = p[ok].cpu().numpy().astype(np.float64)
    lo, hi = np.percentile(p, 10, axis=0), np.percentile(p, 90, axis=0)
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    grid = hip.ProbeGrid(ctx, mid - half, np.maximum(2 * half / (GRID - 1), 1e-3), (GRID,) * 3)   # (a flat set of hits still gives a grid)
    n, K = grid.probes, 6 * M * M
    pts = grid.points()
    d, _, rs = hip.probe_directions_host(M, np.arange(n, dtype=np.uint32))
    with torch.cuda.stream(s):
        tp = torch.from_numpy(pts).to(dev)
        ro = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pts[:, None, :], (n, K, 3))).reshape(-1, 3)).to(dev)
        rd = torch.from_numpy(d.reshape(-1, 3)).to(dev)
        rid = torch.from_numpy(rs.reshape(-1).view(np.int32)).to(dev)
        sh, hits, tmin = torch.empty((n, 9, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
        rgb, t, ns = torch.empty((n * K, 3), device=dev), torch.empty(n * K, device=dev), torch.empty(n * K, dtype=torch.int32, device=dev)
    s.synchronize()
    calls = {"probe_sh": lambda: ctx.probe_sh_device(tp, M, 1, sh=sh, hits=hits, tmin=tmin, stream=s.cuda_stream),
             "radiance": lambda: ctx.radiance_rays_device(ro, rd, spp=1, stream_ids=rid, miss_environment=True, rgb=rgb, t=t, ns=ns, stream=s.cuda_stream)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    yard = statistics.median(spans["radiance"])
    hit_share = float(hits.float().mean()) / K
    for name, span in spans.items():
        ms = statistics.median(span)
        cost.emit(TOOL, f"{tag} grid {name}", config=tag, scene=scene, probes=n, m=M, rays=n * K, spp=1, what=name, **cost.summary(span),
                  mrays_per_s=round(n * K / ms / 1e3, 1), rays_that_hit=round(hit_share, 4), times_radiance=round(ms / yard, 3))
    # the evaluation a viewer calls every frame
    grid.sh, grid.hits, grid.tmin = sh, hits, tmin
    npts = SHADE[0] * SHADE[1]
    with torch.cuda.stream(s):
        g = torch.Generator(device=dev).manual_seed(1)
        span_ = torch.from_numpy((grid.spacing * (GRID - 1)).astype(np.float32)).to(dev)
        at = torch.from_numpy(grid.origin - 0.5 * grid.spacing).to(dev) + torch.rand((npts, 3), device=dev, generator=g) * (span_ + torch.from_numpy(grid.spacing).to(dev))
        nr = torch.nn.functional.normalize(torch.randn((npts, 3), device=dev, generator=g), dim=1).contiguous()
        at = at.contiguous()
        out = torch.empty((npts, 3), device=dev)
    s.synchronize()
    span = cost.timed(s, lambda: grid.shade_device(at, nr, out=out, stream=s.cuda_stream), warmup, repeats)
    ms = statistics.median(span)
    cost.emit(TOOL, f"{tag} grid shade", config=tag, scene=scene, probes=n, points=list(SHADE), what="ProbeGrid.shade_device", **cost.summary(span),
              gb_per_s=round(npts * 36 / ms / 1e6, 1), mpoints_per_s=round(npts / ms / 1e3, 1))
    ctx.close()


def measure_accuracy():
    scene = cost.CONFIGS["c2"][0]
    ctx, _, region, dev, s = cost.open_scene(TOOL, (scene, 64, 48), options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL)
    with torch.cuda.stream(s):
        p, nr, ok = first_hits(ctx, torch, dev, region, s)
        p, nr = p[ok].contiguous(), nr[ok].contiguous()
        keep = (nr != 0).any(dim=1)
        p, nr = p[keep].contiguous(), nr[keep].contiguous()
        probes = ctx.probe_sh_device((p + 0.01 * nr).contiguous(), M, 16, stream=s.cuda_stream)
        shaded = ctx.probe_shade_device(probes["sh"], nr, stream=s.cuda_stream)
        want, _ = ctx.irradiance_points_device(p, nr, 256, stream=s.cuda_stream)
    s.synchronize()
    a, b = shaded.double(), want.double()
    rel = float(torch.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))
    cost.emit(TOOL, "accuracy box", config="accuracy", scene=scene, size=[64, 48], points=int(len(p)), m=M, probe_spp=16, irradiance_spp=256,
              what="probe_shade_device of probes 0.01 N off the hits against irradiance_points_device at the hits", relative_rms=round(rel, 4),
              mean_irradiance=round(float(b.mean()), 4), mean_probe=round(float(a.mean()), 4))
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS + ("accuracy",))
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "probe_cost.txt"))
    a = ap.parse_args()
    if a.one:
        return measure_accuracy() if a.one == "accuracy" else measure_grid(a.one, a.warmup, a.repeats)
    cost.assets()
    rows = cost.run_children(__file__, [[tag] for tag in cost.TAGS + ("accuracy",)], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_probe_cost.py (median, minimum and maximum of {a.repeats} rounds after {a.warmup} warm-up rounds; the two grid calls take turns inside "
             f"a round, each between two events on one caller's stream), a {GRID}^3 grid at m = {M}, 1 spp, coop 0, one run on one MI355X"]
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
