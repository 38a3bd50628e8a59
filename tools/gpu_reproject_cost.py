#!/usr/bin/env python3
"""What carrying a preview across a camera move costs: Context.reproject_device between two events on the caller's
stream, on the frames of bench.py's C2 (Cornell box, 1920x1080) and C5 (trc_scene_tower.xml, 3840x2160), with and without the ids
planes: warm-up calls, then the median of --repeats.  The two frames are rendered in the same process at 4 spp: the scene's own
view as the history, the view one degree round what it shows as the current frame (the camera record turned about the vertical
through the point at the median depth in front of it); the 4-spp frame is timed the same way, and every figure is also given
as a share of it.

Beside the milliseconds, the algorithmic bytes as GB/s and as a share of the HBM peak (8.0 TB/s specified).  Per pixel: the
current frame 20 (rgb, depth, sample count), the history about 20 unique (rgb, depth, length: the four taps of a pixel are its
neighbours' taps too, so every history pixel is needed about once), the outputs 16; the ids planes add 8 to each side: 56 without
ids, 72 with.

Each configuration runs in a child process of its own under a time limit (--limit seconds), by the rule of tools/cost.py; the parent
writes the table to --out.  Needs a GPU: there is no fallback."""
import os
import statistics
import sys

import numpy as np

import cost
from cost import CONFIGS   # noqa: F401  (the frames of the three reprojection tools)

TOOL = "gpu_reproject_cost"
HBM_PEAK = 8.0e12
BYTES = {False: 56, True: 72}


def turned(cam, w, h, distance, degrees):
    """The camera record turned by `degrees` about the image's vertical through the point `distance` in front of the image centre."""
    v = {k: np.asarray(cam[k], np.float64) for k in ("screenA", "screenU", "screenV", "screenX", "screenY", "cam_pos")}
    forward = v["screenA"] + v["screenU"] * (w / 2) + v["screenV"] * (h / 2) - v["cam_pos"]
    forward /= np.linalg.norm(forward)
    axis = -v["screenV"] / np.linalg.norm(v["screenV"])
    pivot = v["cam_pos"] + forward * distance
    a = np.radians(degrees)

    def rot(x):   # Rodrigues
        return x * np.cos(a) + np.cross(axis, x) * np.sin(a) + axis * (axis @ x) * (1 - np.cos(a))

    out = cam.copy()
    for k in ("screenU", "screenV", "screenX", "screenY"):
        out[k] = rot(v[k])
    for k in ("screenA", "cam_pos"):
        out[k] = pivot + rot(v[k] - pivot)
    return out


def two_views(ctx, blob, region, s, dev, guides=False):
    """4-spp frames of the scene's own view (seed 1) and of the view one degree round what it shows (seed 2, the context is left at
    it), each as rgb, depth, ns, ids, normal, albedo - the last two None but for the second frame with `guides` -> cam0, cam1,
    frame 0, frame 1"""
    hip = sys.modules["qaray_amd.hip"]
    w, h = region[2:]

    def frame(seed, guides):
        rgb, depth, ns, ids = cost.frame_tensors(dev, w, h, ids=True)
        normal, albedo = (rgb.new_empty(rgb.shape), rgb.new_empty(rgb.shape)) if guides else (None, None)
        ctx.render_region_device(region, 4, rgb, depth, ns, seed=seed, stream=s.cuda_stream)
        ctx.gbuffer_device(region, seed, normal=normal, albedo=albedo, ids=ids, stream=s.cuda_stream)
        s.synchronize()
        return rgb, depth, ns, ids, normal, albedo

    cam0 = hip.blob_camera(blob).copy()
    frame0 = frame(1, False)
    hits = frame0[1][frame0[1] < 1e29]
    cam1 = turned(cam0, w, h, float(hits.median()) if hits.numel() else 1.0, 1.0)
    ctx.edit_camera(cam1)
    return cam0, cam1, frame0, frame(2, guides)


def measure(tag, warmup, repeats):
    ctx, blob, region, dev, s = cost.open_scene(TOOL, tag)
    torch, _ = cost.gpu(TOOL)
    scene, w, h = CONFIGS[tag]
    cam0, cam1, (rgb0, depth0, ns0, ids0, _, _), (rgb1, depth1, ns1, ids1, _, _) = two_views(ctx, blob, region, s, dev)
    history = (rgb0, depth0, ns0.to(torch.float32))
    out, out_length = torch.empty_like(rgb1), torch.empty_like(depth1)
    torch.cuda.synchronize()

    def reproject(with_ids):
        return ctx.reproject_device((rgb1, depth1, ns1), history, cam0, cam1, ids=ids1 if with_ids else None, hist_ids=ids0 if with_ids else None, out=out,
                                    out_length=out_length, stream=s.cuda_stream)

    frame_ms = statistics.median(cost.timed(s, lambda: ctx.render_region_device(region, 4, rgb1, depth1, ns1, seed=2, stream=s.cuda_stream), warmup, repeats))
    for with_ids in (True, False):
        spans = cost.timed(s, lambda: reproject(with_ids), warmup, repeats)
        ms = statistics.median(spans)
        kept = float((out_length > ns1).float().mean())
        moved = w * h * BYTES[with_ids]
        cost.emit(TOOL, f"{tag} ids={with_ids}", config=tag, scene=scene, size=[w, h], ids=with_ids, **cost.summary(spans), frame4_ms=round(frame_ms, 4),
                  share_of_4spp_frame=round(ms / frame_ms, 4), bytes_per_pixel=BYTES[with_ids], GBps=round(moved / (ms * 1e-3) / 1e9, 1),
                  share_of_hbm_peak_8TBps=round(moved / (ms * 1e-3) / HBM_PEAK, 4), pixels_with_history=round(kept, 4))
    ctx.close()


def write_table(rows, out, warmup, repeats):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("tools/gpu_reproject_cost.py: Context.reproject_device, view 0 -> the view one degree round the scene, 4-spp frames.\n"
                f"One run, one MI355X; median of {repeats} after {warmup} warm-ups between two events on the caller's stream; each configuration in its own process.\n"
                "bytes: algorithmic bytes per pixel (current 20, history about 20 unique, outputs 16; + 8 + 8 with ids); peak: 8.0 TB/s HBM.\n\n")
        f.write(f"{'frame':<40}{'ids':<5}{'median ms (min - max)':<28}{'4-spp frame ms':<16}{'share':<8}{'B/px':<6}{'GB/s':<9}{'of peak':<9}{'with history'}\n")
        for r in rows:
            name = f"{r['config']} {r['scene']} {r['size'][0]}x{r['size'][1]}"
            span = f"{r['median_ms']:.3f} ({r['min_ms']:.3f} - {r['max_ms']:.3f})"
            f.write(f"{name:<40}{'yes' if r['ids'] else 'no':<5}{span:<28}{r['frame4_ms']:<16.3f}{r['share_of_4spp_frame']:<8.4f}{r['bytes_per_pixel']:<6}"
                    f"{r['GBps']:<9.1f}{r['share_of_hbm_peak_8TBps']:<9.4f}{r['pixels_with_history']:.4f}\n")


def main(script=__file__, doc=__doc__, measure=measure, write_table=write_table, repeats=7):
    """(also the main of the two tools that extend this one, with their own measure and table)"""
    name = os.path.basename(script)[len("gpu_"):-len(".py")]
    ap = cost.arguments(doc, repeats=repeats, one=cost.TAGS)
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", name + ".txt"))
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    rows = cost.run_children(script, [[tag] for tag in cost.TAGS], sys.argv[1:], a.limit)
    write_table(rows, a.out, a.warmup, a.repeats)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
