#!/usr/bin/env python3
"""What the irradiance queries cost.  Two kinds of configuration, each in a child process of its own under a time limit
(--limit seconds), by the rule of tools/cost.py:
  c2, c5      the frames of bench.py's C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml, 3840x2160), cooperative walks off, 16
              samples.  The points are the hits of the frame's first camera rays (camera_sample_rays_device sample 0 through
              cast_rays_device; normals turned towards the camera; a miss is a void point), one per pixel, in pixel order, with the
              pixel's stream id.  The calls take turns inside every repeat, each between two events on one caller's stream:
                irradiance   Context.irradiance_points_device at those points
                radiance     Context.radiance_rays_device of those camera rays (one ray per pixel, miss_environment): the same work plus
                             one cast per sample - the yardstick
  cube, c3    Context.bake_light on the two meshes of profiles/bake_cost.txt (the cube of custom_textures.xml, 12 faces; the first
              textured mesh of example_project7_object.xml, 27 794 faces) at 256 x 256 and 1024 x 1024 texels, 16 samples: the mesh's own
              file texture is given that size in the blob before the upload (grey texels), and the whole call is timed by the wall clock
              up to the synchronise behind it - download_scene, the upload of the present bytes, the five device calls, the texel edit.
After warm-up rounds, the median, minimum and maximum of --repeats rounds.  Nothing is fixed in advance: the rows are the measurement.
The lines are printed and written to --out (default profiles/irradiance_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import numpy as np

import cost

TOOL = "gpu_irradiance_cost"
SPP = 16
BAKES = {"cube": "custom_textures.xml", "c3": "example_project7_object.xml"}
SIZES = (256, 1024)


def measure_points(tag, warmup, repeats):
    ctx, _, region, dev, s = cost.open_scene(TOOL, tag, options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL)
    scene, w, h = cost.CONFIGS[tag]
    n = w * h
    with torch.cuda.stream(s):
        rays = ctx.camera_sample_rays_device(region, 0, 1, outputs=("origins", "dirs", "stream_ids"), stream=s.cuda_stream)
        o, d = rays["origins"].reshape(n, 3), rays["dirs"].reshape(n, 3)
        hit = ctx.cast_rays_device(o, d, normal=torch.empty((n, 3), device=dev), point=torch.empty((n, 3), device=dev), stream=s.cuda_stream)
        points = hit["point"]
        normals = (-hit["normal"] * torch.sign((hit["normal"] * d).sum(dim=1, keepdim=True))).contiguous()
        void = float((normals == 0).all(dim=1).float().mean())
        rgb, t, ns = torch.empty((n, 3), device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    s.synchronize()
    calls = {"irradiance": lambda: ctx.irradiance_points_device(points, normals, SPP, stream_ids=rays["stream_ids"], rgb=rgb, ns=ns, stream=s.cuda_stream),
             "radiance": lambda: ctx.radiance_rays_device(o, d, spp=SPP, stream_ids=rays["stream_ids"], miss_environment=True, rgb=rgb, t=t, ns=ns,
                                                          stream=s.cuda_stream)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    yard = statistics.median(spans["radiance"])
    for name, span in spans.items():
        ms = statistics.median(span)
        cost.emit(TOOL, f"{tag} {SPP} spp {name}", config=tag, scene=scene, size=[w, h], spp=SPP, what=name, **cost.summary(span),
                  msamples_per_s=round(n * SPP / ms / 1e3, 1), void_points=round(void, 4), times_radiance=round(ms / yard, 3))
    ctx.close()


def lightmap(hip, blob):
    """-> (node, texmap, texture) of the first mesh node with texture vertices one of whose materials has a file texture for its diffuse"""
    inst, meshes, sets, mats = (hip.blob_table(blob, k) for k in ("instances", "meshes", "mtlsets", "materials"))
    maps, textures = hip.blob_table(blob, "texmaps"), hip.blob_table(blob, "textures")
    for node, rec in enumerate(inst):
        if rec["obj_type"] != 3 or meshes[rec["mesh"]]["num_texcoords"] == 0 or rec["mtlset"] < 0:
            continue
        ms = sets[rec["mtlset"]]
        for m in range(int(ms["first"]), int(ms["first"]) + max(1, int(ms["count"]))):
            tm = int(mats[m]["diffuse"]["texmap"])
            if tm >= 0 and int(maps[tm]["texture"]) >= 0 and int(textures[int(maps[tm]["texture"])]["type"]) == hip.QA_TEX_FILE:
                return node, tm, int(maps[tm]["texture"])
    raise SystemExit(f"{TOOL}: no mesh with texture vertices and a file texture in the scene")


def with_texture_size(hip, blob, tex, w, h):
    """A copy of the blob whose file texture `tex` is w x h grey texels, appended behind everything else"""
    at = (len(blob) + 15) // 16 * 16
    out = np.concatenate([blob, np.zeros(at - len(blob), np.uint8), np.full(3 * w * h, 128, np.uint8)])
    out[8:16].view(np.uint64)[0] = len(out)   # qa_flat_header::total_bytes
    rec = hip.blob_table(out, "textures")[tex:tex + 1]
    rec["width"], rec["height"], rec["off_texels"] = w, h, at
    return out


def measure_bake(tag, warmup, repeats):
    torch, hip = cost.gpu(TOOL)
    cost.assets()
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob(BAKES[tag], size=(256, 192))
    node, texmap, tex = lightmap(hip, blob)
    faces = int(hip.blob_table(blob, "meshes")[hip.blob_table(blob, "instances")[node]["mesh"]]["num_faces"])
    for size in SIZES:
        ctx = hip.Context(0)
        ctx.upload_scene(with_texture_size(hip, blob, tex, size, size))
        kept = {}

        def bake(k):
            kept.update(ctx.bake_light(node, texmap, spp=SPP))
            torch.cuda.synchronize()
            ctx.synchronize()
        spans = cost.walls(bake, warmup, repeats)
        covered = float((kept["face"] >= 0).float().mean())
        cost.emit(TOOL, f"{tag} {size} bake_light", config=tag, scene=BAKES[tag], node=node, faces=faces, texels=[size, size], spp=SPP,
                  covered=round(covered, 4), what="bake_light (wall clock)", **cost.summary(spans))
        ctx.close()


def main():
    ap = cost.arguments(__doc__, one=cost.TAGS + tuple(BAKES))
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "irradiance_cost.txt"))
    a = ap.parse_args()
    if a.one:
        return (measure_points if a.one in cost.TAGS else measure_bake)(a.one, a.warmup, a.repeats)
    cost.assets()
    rows = cost.run_children(__file__, [[tag] for tag in cost.TAGS + tuple(BAKES)], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_irradiance_cost.py (median, minimum and maximum of {a.repeats} rounds after {a.warmup} warm-up rounds; c2, c5: the two calls take turns "
             f"inside a round, each between two events on one caller's stream; cube, c3: wall clock of the whole call), {SPP} spp, coop 0, one run on one MI355X"]
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
