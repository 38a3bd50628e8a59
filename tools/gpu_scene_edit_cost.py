#!/usr/bin/env python3
"""What moving the camera of a resident scene costs, two ways (Cost):

  (a) upload_scene(B): host table build (every mesh tree), a fresh allocation and copy of every table
  (b) edit_camera(B's camera block) + synchronize: the scene-side rebuild on the host and a few bytes copied

on the C2 frame (Cornell box, 1920x1080) and the C5 frame (tower, 3840x2160).  Wall time: warm-up, then the median of --repeats
calls, each ending in a device synchronise (A and B alternate, so that every call changes the scene).  Also: the first frame
after an upload against the first frame after an edit (kernel time by HIP events and wall time, --spp samples per pixel), and
what the context's counters say the two ways did (mesh-table builds, device allocations, bytes copied).

--package DIR times (a) only, with the qaray_amd package of another checkout (DIR/qaray_amd with its built libraries and
DIR/scenes: the parent commit's, which has no edits): the yardstick.  The measurement runs in a child process under a time limit
(--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no fallback, and without one this fails."""
import os
import statistics
import sys

import numpy as np

import cost

TOOL = "gpu_scene_edit_cost"


def summary(t):
    return cost.summary(t, 3)


def measure(a):
    _, hip = cost.gpu(TOOL, os.path.abspath(a.package) if a.package else cost.ROOT)
    from qaray_amd import host
    cost.assets()
    ctx = hip.Context(0)
    for name in a.frames.split(","):
        scene, w, h = cost.frame(name)
        region = (0, 0, w, h)
        s = host.HostScene(os.path.join(host.SCENES_DIR, scene), size=(w, h))
        blobs = [s.flatten()]
        cams = []
        if not a.package:
            # B: the eye moved by about a degree round the scene's centre
            import xml.etree.ElementTree as ET
            cam = {e.tag: [float(e.get(k, 0)) for k in "xyz"] for e in ET.parse(os.path.join(host.SCENES_DIR, scene)).getroot().find("camera")
                   if e.tag in ("position", "target", "up")}
            cams.append(s.camera().copy())
            pos, tgt, up = (np.array(cam[k], np.float32) for k in ("position", "target", "up"))
            side = np.cross(up, pos - tgt)
            s.set_camera(pos + np.float32(0.0175) * side, tgt, up)
            cams.append(s.camera().copy())
            blobs.append(s.flatten())
        else:
            blobs.append(blobs[0].copy())
        s.close()

        def upload(k):
            ctx.upload_scene(blobs[k % 2])
            ctx.synchronize()

        rec = {"frame": name, "size": [w, h], "blob_bytes": int(blobs[0].size), "library": hip.HIP_LIB_PATH,
               "a_upload_scene": summary(cost.walls(upload, a.warmup, a.repeats))}
        if not a.package:
            rec["context_stats_after_these_uploads"] = dict(zip(("mesh_builds", "allocations", "bytes_copied", "edits"), ctx.scene_stats()))

            def edit(k):
                ctx.edit_camera(cams[k % 2])
                ctx.synchronize()

            before = ctx.scene_stats()
            rec["b_edit_camera_synchronize"] = summary(cost.walls(edit, a.warmup, a.repeats))
            after = ctx.scene_stats()
            rec["edit_stats"] = {"mesh_builds": after[0] - before[0], "allocations": after[1] - before[1], "bytes_copied_per_edit": after[2]}
            rec["a_over_b"] = round(rec["a_upload_scene"]["median_ms"] / rec["b_edit_camera_synchronize"]["median_ms"], 1)
            rec["edit_camera_call_alone"] = summary(cost.walls(lambda k: ctx.edit_camera(cams[k % 2]), a.warmup, a.repeats))
            ctx.synchronize()

            # the first frame after an upload of B against the first frame after an edit to B
            first = {}
            for how in ("upload", "edit"):
                wall, kern = [], []
                for _ in range(3):
                    ctx.upload_scene(blobs[0])
                    ctx.render_region(region, a.spp)
                    if how == "upload":
                        ctx.upload_scene(blobs[1])
                    else:
                        ctx.edit_camera(cams[1])
                    ctx.synchronize()
                    ctx.reset_kernel_time()
                    wall.append(cost.wall(lambda: ctx.render_region(region, a.spp)))
                    kern.append(ctx.kernel_time()[0])
                first[how] = {"wall_ms": round(statistics.median(wall), 3), "kernel_ms": round(statistics.median(kern), 3)}
            rec["first_frame_after"] = first
            rec["first_frame_spp"] = a.spp
        cost.emit(TOOL, name, **rec)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=("all",))
    ap.add_argument("--frames", default="C2,C5")
    ap.add_argument("--spp", type=int, default=4, help="samples per pixel of the first-frame comparison")
    ap.add_argument("--package", default=None, help="another checkout's root: its qaray_amd is imported, only the upload is timed")
    a = ap.parse_args()
    if a.one:
        return measure(a)
    cost.run_children(__file__, [["all"]], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
