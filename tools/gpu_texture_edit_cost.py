#!/usr/bin/env python3
"""What repainting a texture of a resident scene costs (texture edits):

  (a) upload_scene(B): host table build (every mesh tree), a fresh allocation and copy of every table
  (b) edit_texels of a whole file texture from host memory, and from a device tensor, + synchronize
  (c) the kernel alone: edit_texels from a device tensor between two events on the caller's stream (the context's stream waits for
      that stream and that stream for the kernel, so the span holds the kernel and two event waits), with the bytes it moves -
      3 read, 3 + 16 written per texel - as GB/s

on the C3 frame (the textured objects, 1920x1080) and on custom_textures.xml (160x120).  Wall time: warm-up, then the median of
--repeats calls, each ending in a device synchronise (two images alternate, so that every call changes the scene).

--package DIR times (a) only, with the qaray_amd package of another checkout (DIR/qaray_amd with its built libraries and
DIR/scenes: the parent commit's, which has no texture edits): the yardstick.  The measurement runs in a child process under a time
limit (--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no fallback."""
import itertools
import os
import sys

import numpy as np

import cost

TOOL = "gpu_texture_edit_cost"
FRAMES = {"C3": ("example_project7_object.xml", (1920, 1080)), "custom_textures": ("custom_textures.xml", (160, 120))}
PEAK_GBS = 8000.0


def measure(a):
    torch, hip = cost.gpu(TOOL, os.path.abspath(a.package) if a.package else cost.ROOT)
    from qaray_amd import host
    cost.assets()
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    n = a.warmup + a.repeats
    for name in a.frames.split(","):
        scene, (w, h) = FRAMES[name]
        blob_a = host.load_scene_blob(scene, size=(w, h))
        rec = {"frame": name, "size": [w, h], "blob_bytes": int(blob_a.size), "library": hip.HIP_LIB_PATH}
        blobs = [blob_a, blob_a.copy()]
        if not a.package:
            tex = hip.blob_table(blob_a, "textures")
            files = [i for i in range(len(tex)) if tex[i]["type"] == 1 and tex[i]["width"] > 0]
            ti = max(files, key=lambda i: int(tex[i]["width"]) * int(tex[i]["height"]))
            th, tw = hip.blob_texels(blob_a, ti).shape[:2]
            rng = np.random.default_rng(1)
            images = [hip.blob_texels(blob_a, ti).copy(), rng.integers(0, 256, (th, tw, 3)).astype(np.uint8)]
            hip.blob_texels(blobs[1], ti)[...] = images[1]
            rec.update(texture=ti, texture_size=[tw, th], texels=tw * th)

        def upload(k):
            ctx.upload_scene(blobs[k % 2])
            ctx.synchronize()

        rec["a_upload_scene"] = cost.summary(cost.walls(upload, a.warmup, a.repeats))
        if not a.package:
            before = ctx.scene_stats()

            def edit_host(k):
                ctx.edit_texels(ti, images[k % 2])
                ctx.synchronize()

            rec["b_edit_texels_host_synchronize"] = cost.summary(cost.walls(edit_host, a.warmup, a.repeats))
            rec["host_edit_bytes_over_the_link"] = ctx.scene_stats()[2]
            tensors = [torch.from_numpy(x).to(dev) for x in images]
            torch.cuda.synchronize()

            def edit_device(k):
                ctx.edit_texels(ti, tensors[k % 2])
                ctx.synchronize()

            rec["b_edit_texels_device_synchronize"] = cost.summary(cost.walls(edit_device, a.warmup, a.repeats))
            rec["device_edit_bytes_over_the_link"] = ctx.scene_stats()[2]
            after = ctx.scene_stats()
            rec["edit_stats"] = {"mesh_builds": after[0] - before[0], "allocations": after[1] - before[1], "edits": after[3] - before[3]}
            rec["a_over_b_host"] = round(rec["a_upload_scene"]["median_ms"] / rec["b_edit_texels_host_synchronize"]["median_ms"], 1)
            rec["a_over_b_device"] = round(rec["a_upload_scene"]["median_ms"] / rec["b_edit_texels_device_synchronize"]["median_ms"], 1)
            s = torch.cuda.Stream(dev)
            k = itertools.count()
            # (the context's stream is drained before every window, and after the last)
            rec["c_kernel_between_events"] = cost.summary(cost.timed(s, lambda: ctx.edit_texels(ti, tensors[next(k) % 2], stream=s.cuda_stream), a.warmup, a.repeats,
                                                                     before=ctx.synchronize))
            ctx.synchronize()
            moved = tw * th * (3 + 3 + 16)
            gbs = moved / (rec["c_kernel_between_events"]["median_ms"] * 1e-3) / 1e9
            rec["kernel_bytes_moved"] = moved
            rec["kernel_gb_per_s"] = round(gbs, 2)
            rec["share_of_8_tb_per_s"] = round(gbs / PEAK_GBS, 5)
            assert np.array_equal(ctx.download_scene(), blobs[(n - 1) % 2])
        cost.emit(TOOL, name, **rec)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=("all",))
    ap.add_argument("--frames", default="C3,custom_textures")
    ap.add_argument("--package", default=None, help="another checkout's root: its qaray_amd is imported, only the upload is timed")
    a = ap.parse_args()
    if a.one:
        return measure(a)
    cost.run_children(__file__, [["all"]], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
