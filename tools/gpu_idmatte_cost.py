#!/usr/bin/env python3
"""What the id matte costs against the coverage-only matte, which casts the same rays: on the frame of bench.py's C2
(Cornell box, 1920x1080) at 512 spp and of C5 (trc_scene_tower.xml, 3840x2160, meshes in global memory) at its own 2048 spp.  The
calls take turns inside every repeat, each between two events on the caller's stream, same library, same stream:
  matte coverage   Context.matte_device, the coverage plane alone (4 bytes written per pixel)
  idmatte node     Context.idmatte_device, key "node", all four planes (72 bytes written per pixel)
  idmatte material the same with key "material" (the hit's material set is looked up per sample)
  select           Context.idmatte_select_device over those planes, one id
After warm-up rounds, the medians of --repeats rounds, and the band rule of tools/cost.py (cost.band) with the coverage matte as the
parent: `verdict` says whether the id matte's median lies inside the coverage matte's own min - max range (or 3 % band).  Nothing is
fixed in advance: the rows are the measurement.  Each configuration runs in a child process of its own under a time limit (--limit
seconds), by the rule of tools/cost.py.  Needs a GPU: there is no fallback."""
import sys

import cost

TOOL = "gpu_idmatte_cost"
SPP = {"c2": 512, "c5": 2048}   # the frames' own spp (bench.py's configs)


def measure(tag, warmup, repeats):
    ctx, blob, region, dev, s = cost.open_scene(TOOL, tag)
    torch, hip = cost.gpu(TOOL)
    scene, w, h = cost.CONFIGS[tag]
    spp = SPP[tag]
    cov = torch.empty((h, w), dtype=torch.float32, device=dev)
    out = torch.empty((h, w), dtype=torch.float32, device=dev)
    m = ctx.idmatte_device(region, spp, "node", stream=s.cuda_stream)
    s.synchronize()
    first = int(m["ids"][h // 2, w // 2, 0])
    calls = {"matte coverage": lambda: ctx.matte_device(region, spp, coverage=cov, stream=s.cuda_stream),
             "idmatte node": lambda: ctx.idmatte_device(region, spp, "node", stream=s.cuda_stream, **m),
             "idmatte material": lambda: ctx.idmatte_device(region, spp, "material", stream=s.cuda_stream, **m),
             "select": lambda: ctx.idmatte_select_device(m["ids"], m["counts"], m["samples"], [first], out=out, stream=s.cuda_stream)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    parent = cost.summary(spans["matte coverage"])
    yard = [(parent["median_ms"], parent["min_ms"], parent["max_ms"])]
    for name, t in spans.items():
        row = cost.summary(t)
        more = {}
        if name.startswith("idmatte"):
            b = cost.band(yard, [(row["median_ms"], row["min_ms"], row["max_ms"])])
            more = {"allowed_ms": [round(v, 4) for v in b["allowed"]], "band": b["kind"], "verdict": b["verdict"], "percent": round(b["percent"], 2)}
        cost.emit(TOOL, f"{tag} {spp} spp {name}", config=tag, scene=scene, size=[w, h], spp=spp, what=name, **row,
                  share_of_coverage_matte=round(row["median_ms"] / parent["median_ms"], 4), **more)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS)
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    cost.run_children(__file__, [[tag] for tag in cost.TAGS], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
