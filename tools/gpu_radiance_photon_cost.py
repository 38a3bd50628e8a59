#!/usr/bin/env python3
"""What the batches that gather from photon maps cost (QA_RADIANCE_PHOTON_MAPS).  Three configurations, each in a child
process of its own under a time limit (--limit seconds), by the rule of tools/cost.py:
  frame     custom_photon.xml at 1920x1080, 4 samples, default-sized maps (build_photon_maps()).  Two calls take turns inside every
            repeat, each between two events on one caller's stream:
              frame      (a) render_region_device with the maps built - the yardstick
              batch      (b) radiance_rays_device(photon_maps=True) of the frame's own sample rays (camera_sample_rays_device, all
                         outputs, per sample): the same work from ray arrays
  points    the same scene, frame and maps: (c) irradiance_points_device(photon_maps=True) at the first hits of the frame's first
            camera rays (normals turned towards the camera; a miss is a void point), 4 samples, and then the same call without the
            flag once the maps are cleared: the price of the gathers
  bake      Context.bake_light on the fixture of tests/golden/bake_light with its ball made of custom_photon.xml's glass and its light
            map given 256 x 256 texels, 16 samples: with photon_maps=True (the maps are built again ahead of every call, outside the
            clock: the call's texel edit drops them) and plain, wall clock of the whole call up to the synchronise behind it
After warm-up rounds, the median, minimum and maximum of --repeats rounds.  Nothing is fixed in advance: the rows are the measurement.
The lines are printed and written to --out (default profiles/radiance_photon_cost.txt).  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import numpy as np

import cost
from gpu_irradiance_cost import with_texture_size

TOOL = "gpu_radiance_photon_cost"
FRAME = ("custom_photon.xml", 1920, 1080)
SPP, BAKE_SPP, BAKE_SIZE = 4, 16, 256
BAKE_MAPS = ((2000, 20, 0.5), (200, 20, 1.0))   # (tests/test_gpu_bake_light_photon.py: they fill on this scene)
FIXTURE = os.path.join(cost.ROOT, "tests", "golden", "bake_light")
CONFIGS = ("frame", "points", "bake")


def measure_frame(warmup, repeats):
    ctx, _, region, dev, s = cost.open_scene(TOOL, FRAME, options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL)
    scene, w, h = FRAME
    n = w * h
    ctx.build_photon_maps()
    rgb, depth, ns = cost.frame_tensors(dev, w, h)
    with torch.cuda.stream(s):
        rays = ctx.camera_sample_rays_device(region, 0, SPP, stream=s.cuda_stream)
        b_rgb, b_t, b_ns = torch.empty((n, 3), device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    s.synchronize()
    calls = {"frame": lambda: ctx.render_region_device(region, SPP, rgb, depth, ns, stream=s.cuda_stream),
             "batch": lambda: ctx.radiance_rays_device(rays["origins"], rays["dirs"], spp=SPP, dx=rays["dx"], dy=rays["dy"], screen=rays["screen"],
                                                       stream_ids=rays["stream_ids"], rgb=b_rgb, t=b_t, ns=b_ns, stream=s.cuda_stream, photon_maps=True)}
    spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
    same = bool(torch.equal(rgb.reshape(n, 3).view(torch.int32), b_rgb.view(torch.int32)))
    yard = statistics.median(spans["frame"])
    for name, span in spans.items():
        ms = statistics.median(span)
        cost.emit(TOOL, f"frame {SPP} spp {name}", config="frame", scene=scene, size=[w, h], spp=SPP, kernel=ctx.kernel_name(), what=name,
                  **cost.summary(span), msamples_per_s=round(n * SPP / ms / 1e3, 1), same_bits_as_frame=same, times_frame=round(ms / yard, 3))
    ctx.close()


def measure_points(warmup, repeats):
    ctx, _, region, dev, s = cost.open_scene(TOOL, FRAME, options=(("coop", 0),))
    torch, hip = cost.gpu(TOOL)
    scene, w, h = FRAME
    n = w * h
    with torch.cuda.stream(s):
        rays = ctx.camera_sample_rays_device(region, 0, 1, outputs=("origins", "dirs", "stream_ids"), stream=s.cuda_stream)
        o, d = rays["origins"].reshape(n, 3), rays["dirs"].reshape(n, 3)
        hit = ctx.cast_rays_device(o, d, normal=torch.empty((n, 3), device=dev), point=torch.empty((n, 3), device=dev), stream=s.cuda_stream)
        points = hit["point"]
        normals = (-hit["normal"] * torch.sign((hit["normal"] * d).sum(dim=1, keepdim=True))).contiguous()
        void = float((normals == 0).all(dim=1).float().mean())
        rgb, ns = torch.empty((n, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    s.synchronize()
    spans = {}
    ctx.build_photon_maps()
    spans["with maps"] = cost.timed(s, lambda: ctx.irradiance_points_device(points, normals, SPP, stream_ids=rays["stream_ids"], rgb=rgb, ns=ns,
                                                                           stream=s.cuda_stream, photon_maps=True), warmup, repeats)
    ctx.clear_photon_maps()
    spans["maps cleared"] = cost.timed(s, lambda: ctx.irradiance_points_device(points, normals, SPP, stream_ids=rays["stream_ids"], rgb=rgb, ns=ns,
                                                                              stream=s.cuda_stream), warmup, repeats)
    yard = statistics.median(spans["maps cleared"])
    for name, span in spans.items():
        ms = statistics.median(span)
        cost.emit(TOOL, f"points {SPP} spp {name}", config="points", scene=scene, size=[w, h], spp=SPP, what="irradiance_points_device, " + name,
                  **cost.summary(span), msamples_per_s=round(n * SPP / ms / 1e3, 1), void_points=round(void, 4), times_cleared=round(ms / yard, 3))
    ctx.close()


def glass_ball_fixture(hip):
    """The fixture's blob with the ball's material replaced by custom_photon.xml's glass -> blob, node, texmap, texture"""
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob(os.path.join(FIXTURE, "scene.xml"), size=(48, 36), asset_root=FIXTURE).copy()
    donor = hip.blob_table(load_scene_blob("custom_photon.xml", size=(48, 36)), "materials")
    (glass,) = [m for m in donor if np.allclose(m["refraction"]["color"], 0.95) and float(m["ior"]) == 1.5]
    mats = hip.blob_table(blob, "materials")
    (ball,) = [i for i, m in enumerate(mats) if np.allclose(m["diffuse"]["color"], (0.7, 0.6, 0.5))]
    mats[ball] = glass
    maps, textures = hip.blob_table(blob, "texmaps"), hip.blob_table(blob, "textures")
    (texmap,) = [i for i in range(len(maps)) if int(textures[int(maps[i]["texture"])]["type"]) == hip.QA_TEX_FILE]
    return blob, 3, texmap, int(maps[texmap]["texture"])   # (node 3: floor, ball, chart behind the root)


def measure_bake(warmup, repeats):
    torch, hip = cost.gpu(TOOL)
    blob, node, texmap, tex = glass_ball_fixture(hip)
    ctx = hip.Context(0)
    ctx.upload_scene(with_texture_size(hip, blob, tex, BAKE_SIZE, BAKE_SIZE))
    kept, spans = {}, {"photon_maps": [], "plain": []}

    def bake(flag):
        kept.update(ctx.bake_light(node, texmap, spp=BAKE_SPP, photon_maps=flag))
        torch.cuda.synchronize()
        ctx.synchronize()
    for k in range(warmup + repeats):
        for name in spans:
            if name == "photon_maps":
                ctx.build_photon_maps(*BAKE_MAPS)
                ctx.synchronize()
            ms = cost.wall(lambda: bake(name == "photon_maps"))
            if k >= warmup:
                spans[name].append(ms)
    covered = float((kept["face"] >= 0).float().mean())
    yard = statistics.median(spans["plain"])
    for name, span in spans.items():
        cost.emit(TOOL, f"bake {BAKE_SIZE} {name}", config="bake", scene="tests/golden/bake_light/scene.xml, glass ball", node=node,
                  texels=[BAKE_SIZE, BAKE_SIZE], spp=BAKE_SPP, covered=round(covered, 4), what=f"bake_light {name} (wall clock)", **cost.summary(span),
                  times_plain=round(statistics.median(span) / yard, 3))
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=CONFIGS)
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "radiance_photon_cost.txt"))
    a = ap.parse_args()
    if a.one:
        return {"frame": measure_frame, "points": measure_points, "bake": measure_bake}[a.one](a.warmup, a.repeats)
    cost.assets()
    rows = cost.run_children(__file__, [[c] for c in CONFIGS], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_radiance_photon_cost.py (median, minimum and maximum of {a.repeats} rounds after {a.warmup} warm-up rounds; frame: the two calls "
             f"take turns inside a round, each between two events on one caller's stream; points: each call between two events; bake: wall clock of the "
             f"whole call), coop 0, one run on one MI355X"]
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
