#!/usr/bin/env python3
"""What ambient occlusion costs: on the frame of bench.py's C2 (Cornell box, 1920x1080) and of C5
(trc_scene_tower.xml, 3840x2160, meshes in global memory), at 4 spp, K in {4, 16} rays per hit, radius unbounded and a tenth of the
scene's extent (the diagonal of the box around what 32 rows of the frame's first samples hit).  Per configuration the calls take
turns inside every repeat, each between two events on the caller's stream, same library, same stream:
  gbuffer      Context.gbuffer_device, all planes: the yardstick of the earlier cost files (one camera ray per pixel)
  ao           Context.ao_device, the three planes (12 bytes written per pixel)
  composition  what a caller had to assemble before: camera_sample_rays_device -> cast_rays_device -> the facing normals and
               cosine-weighted directions built with torch -> occluded_device -> the sums per pixel, in strips of rows of at most
               2^24 shadow rays (the whole frame's would not fit: 28 bytes a ray).  The directions are torch's own random numbers,
               not the library's generator: the row is a cost, its planes are not compared
After warm-up rounds, the medians of --repeats rounds.  Nothing about ao against the composition is fixed in advance: the rows are
the measurement, with their ratio.  --only ao times the ao rows alone (what an A/B of two builds of the kernel runs, tools/cost_ab.py);
--other-lib PATH adds the ao rows of a second build of the library ("ao other form").  Each configuration runs in a child process of
its own under a time limit (--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no fallback."""
import os
import sys

import cost

TOOL = "gpu_ao_cost"
SPP = 4
KS = (4, 16)
STRIP_RAYS = 1 << 24


def extent(ctx, torch, region, s):
    """The diagonal of the box around the first hits of 32 rows of the frame"""
    w, h = region[2], region[3]
    lo, hi = None, None
    with torch.cuda.stream(s):
        for y in range(0, h, max(1, h // 32)):
            r = ctx.camera_sample_rays_device((0, y, w, y + 1), 0, 1, outputs=("origins", "dirs"), stream=s.cuda_stream)
            got = ctx.cast_rays_device(r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3), stream=s.cuda_stream)
            p = got["point"][got["t"] < 1e29]
            if len(p):
                lo = p.min(dim=0).values if lo is None else torch.minimum(lo, p.min(dim=0).values)
                hi = p.max(dim=0).values if hi is None else torch.maximum(hi, p.max(dim=0).values)
    s.synchronize()
    return float((hi - lo).norm())


def composition(ctx, torch, region, k, radius, s, out):
    """One frame's open counts through the public queries, strip by strip, everything on stream s"""
    w, h = region[2], region[3]
    rows = max(1, STRIP_RAYS // (w * SPP * k))
    with torch.cuda.stream(s):
        for y in range(0, h, rows):
            y1 = min(h, y + rows)
            r = ctx.camera_sample_rays_device((0, y, w, y1), 0, SPP, outputs=("origins", "dirs"), stream=s.cuda_stream)
            d = r["dirs"].reshape(-1, 3)
            got = ctx.cast_rays_device(r["origins"].reshape(-1, 3), d, stream=s.cuda_stream)
            n = got["normal"]
            n = torch.where(((n * d).sum(dim=1, keepdim=True) <= 0), n, -n)
            hit = (got["t"] < 1e29).repeat_interleave(k)
            sph = torch.nn.functional.normalize(torch.randn((n.shape[0] * k, 3), device=n.device), dim=1)
            dirs = torch.nn.functional.normalize(n.repeat_interleave(k, dim=0) + sph, dim=1).contiguous()
            occ = ctx.occluded_device(got["point"].repeat_interleave(k, dim=0).contiguous(), dirs, radius, stream=s.cuda_stream)
            out[y:y1] = ((occ == 0) & hit).view(y1 - y, w, SPP * k).sum(dim=2)


def measure(tag, warmup, repeats, only):
    ctx, blob, region, dev, s = cost.open_scene(TOOL, tag)
    torch, hip = cost.gpu(TOOL)
    scene, w, h = cost.CONFIGS[tag]
    tenth = extent(ctx, torch, region, s) / 10.0
    planes = ctx.ao_device(region, SPP, stream=s.cuda_stream)
    guide = ctx.gbuffer_device(region, stream=s.cuda_stream)
    counts = torch.empty((h, w), dtype=torch.int64, device=dev)
    s.synchronize()
    other = bool(os.environ.get("QA_AO_COST_OTHER"))
    for k in KS:
        for rname, radius in (("unbounded", float("inf")), ("tenth", tenth)):
            calls = {"ao": lambda: ctx.ao_device(region, SPP, k, radius, stream=s.cuda_stream, **planes)}
            if not only:
                calls["gbuffer"] = lambda: ctx.gbuffer_device(region, stream=s.cuda_stream, **guide)
                calls["composition"] = lambda: composition(ctx, torch, region, k, radius, s, counts)
            spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
            ao = cost.summary(spans["ao"])
            open_share = float(planes["open"].sum()) / max(1.0, float(planes["rays"].sum()))
            for name, t in spans.items():
                row = cost.summary(t)
                more = {"ao_over_this": round(ao["median_ms"] / row["median_ms"], 4)} if name != "ao" else {"open_share": round(open_share, 4)}
                what = "ao other form" if (other and name == "ao") else name
                cost.emit(TOOL, f"{tag} K {k} {rname} {what}", config=tag, scene=scene, size=[w, h], spp=SPP, K=k, radius=rname,
                          radius_value=None if radius == float("inf") else round(radius, 4), what=what, **row, **more)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    ap.add_argument("--only", choices=("ao",), help="time the ao rows alone")
    ap.add_argument("--other-lib", help="a second build of libqaray_hip.so: its ao rows are added as 'ao other form'")
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats, a.only or ("ao" if os.environ.get("QA_AO_COST_OTHER") else None))
    rest = []
    args = sys.argv[1:]
    i = 0
    while i < len(args):   # (the children do not take --other-lib)
        if args[i] == "--other-lib":
            i += 2
            continue
        if args[i].startswith("--other-lib="):
            i += 1
            continue
        rest.append(args[i])
        i += 1
    cost.run_children(__file__, [[tag] for tag in cost.TAGS], rest, a.limit)
    if a.other_lib:
        os.environ["QA_HIP_LIB"] = os.path.abspath(a.other_lib)
        os.environ["QA_AO_COST_OTHER"] = "1"
        cost.run_children(__file__, [[tag] for tag in cost.TAGS], rest, a.limit)


if __name__ == "__main__":
    main()
