#!/usr/bin/env python3
"""The table behind the defaults of the reprojection's colour clamp: eight 4-spp previews of custom_softshadow.xml at
64x48 through hip.TemporalPreview (tests/reproject_motion_util.preview_run, the harness of tests/test_gpu_reproject_motion.py), luma
RMSE of the accumulated frame to a 256-spp frame of the final scene,
  (b) with a light's intensity quartered before frame 5 and no reset (lower is better: the stale history has to leave),
  (c) on a still scene (the clamp must keep the gain of accumulating: below the midpoint of the raw frame's and the unclamped RMSE),
for clamp_radius in {1, 2} x clamp_gamma in {1, 2, 3}, beside the raw frame and the unclamped preview.  The defaults are the pair
with the lowest (b) among those that meet (c).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_motion_quality.txt"))
    a = ap.parse_args()
    import torch
    import reproject_motion_util as mu
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    if not torch.cuda.is_available():
        raise SystemExit("gpu_reproject_motion_quality: no GPU (nothing is measured without one)")
    blob = load_scene_blob(os.path.join(SCENES_DIR, mu.PREVIEW_SCENE), size=mu.PREVIEW_SIZE)
    ctx = hip.Context(0)
    lines = []

    def rmse(scenario, **kw):
        r = mu.preview_run(ctx, blob, scenario, **kw)
        return mu.luma_rmse(r["acc"], r["truth"]), mu.luma_rmse(r["raw"], r["truth"])

    (b_off, b_raw), (c_off, c_raw) = rmse("light", clamp=False), rmse("still", clamp=False)
    mid = 0.5 * (c_raw + c_off)
    lines.append(f"{'':<22}{'(b) light quartered':<22}{'(c) still scene'}")
    lines.append(f"{'raw 4-spp frame':<22}{b_raw:<22.4f}{c_raw:.4f}")
    lines.append(f"{'clamp off':<22}{b_off:<22.4f}{c_off:.4f}")
    lines.append(f"{'(c) must lie below':<22}{'':<22}{mid:.4f}")
    best = None
    for radius in (1, 2):
        for gamma in (1.0, 2.0, 3.0):
            b, c = rmse("light", clamp=True, clamp_radius=radius, clamp_gamma=gamma)[0], rmse("still", clamp=True, clamp_radius=radius, clamp_gamma=gamma)[0]
            ok = c < mid
            lines.append(f"{f'r = {radius}, gamma = {gamma:g}':<22}{b:<22.4f}{c:<10.4f}{'meets (c)' if ok else 'misses (c)'}")
            if ok and (best is None or b < best[0]):
                best = (b, radius, gamma)
    lines.append("")
    lines.append("no pair meets (c)" if best is None else f"lowest (b) among the pairs that meet (c): r = {best[1]}, gamma = {best[2]:g}")
    d = hip.ReprojectMotionParams.default()
    lines.append(f"the library's defaults: r = {d.clamp_radius}, gamma = {d.clamp_gamma:g}")
    ctx.close()
    text = ("tools/gpu_reproject_motion_quality.py: luma RMSE to the 256-spp frame of the final scene after eight 4-spp previews of "
            f"{mu.PREVIEW_SCENE} at {mu.PREVIEW_SIZE[0]}x{mu.PREVIEW_SIZE[1]}, one MI355X\n\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
