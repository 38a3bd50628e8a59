#!/usr/bin/env python3
"""The tables behind the two defaults of DESIGN.md 4k, shorten_rate (qa_reproject_moments_params) and variance_scale
(qa_denoise_variance_params).  Without --gpu everything runs on the CPU: the oracle's frames, the host builds of the reprojection
and the filter (hip.reproject_moments_host, hip.denoise_variance_host).  With --gpu the chosen rows are confirmed once on the device
with the renderer's own frames and planes (hip.TemporalPreview, gbuffer_device, denoise_variance_device) and appended to --out; the
sweeps are not rerun.

shorten_rate over {0.25, 0.5, 1, 2, 4}: the scenarios of 4j - custom_softshadow.xml at 64x48, eight 4-spp frames of new seeds, a still
camera, luma RMSE of the last accumulated frame to a 256-spp frame of the final scene -
  (b) the first light's intensity quartered before frame 5 (lower is better: the stale history has to leave),
  (c) a still scene (the gain of accumulating must stay: below the midpoint of the raw frame's and the unclamped RMSE);
the default is the rate with the lowest (b) among those that meet (c).

variance_scale over {0.25, 1, 4, 16}: custom_textures.xml and the Cornell box at 64x64, eight 4-spp frames accumulated with the
moments, the accumulated frame filtered by the guided form (i) and by the variance form (ii), luma RMSE to 256 spp; the default is
the scale with the lowest (ii) / (i) on the textured scene among those with (ii) <= 1.02 x (i) on the box.  On the CPU the guide is
the albedo plane alone (the emission twin's frame; there is no normal plane without the device); on the device both guides."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHORTEN_RATES = (0.25, 0.5, 1.0, 2.0, 4.0)


def cpu_shorten(lines):
    import reproject_motion_util as mu
    from oracle import binding as oracle
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    w, h = mu.PREVIEW_SIZE
    region = (0, 0, w, h)
    blob = load_scene_blob(os.path.join(SCENES_DIR, mu.PREVIEW_SCENE), size=mu.PREVIEW_SIZE)
    cam = hip.blob_camera(blob).copy()

    def frames(scenario):
        work = blob.copy()
        lights = hip.blob_table(work, "lights")
        out = []
        for k in range(mu.PREVIEW_FRAMES):
            if scenario == "light" and k == 4:
                lights[0]["intensity"] *= np.float32(0.25)
            rgb, depth, ns = oracle.render(work, region, mu.PREVIEW_SPP, seed=1000 + k)[:3]
            out.append((rgb.astype(np.float32), depth, ns))
        return out, oracle.render(work, region, 256, seed=77)[0]

    def run(fr, **kw):
        hist = (np.zeros_like(fr[0][0]), fr[0][1], np.zeros(fr[0][1].shape, np.float32))
        for f in fr:
            res = hip.reproject_moments_host(f, hist, cam, cam, **kw)
            hist = (res[0], f[1], res[1])
        return res

    (fb, tb), (fc, tc) = frames("light"), frames("still")
    b_raw, c_raw = mu.luma_rmse(fb[-1][0], tb), mu.luma_rmse(fc[-1][0], tc)
    b_off, c_off = mu.luma_rmse(run(fb)[0], tb), mu.luma_rmse(run(fc)[0], tc)
    b_clamp, c_clamp = mu.luma_rmse(run(fb, clamp=True)[0], tb), mu.luma_rmse(run(fc, clamp=True)[0], tc)
    mid = 0.5 * (c_raw + c_off)
    lines.append(f"{'':<24}{'(b) light quartered':<22}{'(c) still scene':<18}mean length (b) / (c)")
    lines.append(f"{'raw 4-spp frame':<24}{b_raw:<22.4f}{c_raw:.4f}")
    lines.append(f"{'clamp off':<24}{b_off:<22.4f}{c_off:.4f}")
    lines.append(f"{'clamp alone (4j)':<24}{b_clamp:<22.4f}{c_clamp:.4f}")
    lines.append(f"{'(c) must lie below':<24}{'':<22}{mid:.4f}")
    best = None
    for rate in SHORTEN_RATES:
        rb, rc = run(fb, clamp=True, shorten=True, shorten_rate=rate), run(fc, clamp=True, shorten=True, shorten_rate=rate)
        b, c = mu.luma_rmse(rb[0], tb), mu.luma_rmse(rc[0], tc)
        ok = c < mid
        lines.append(f"{f'shorten_rate = {rate:g}':<24}{b:<22.4f}{c:<18.4f}{rb[1].mean():.1f} / {rc[1].mean():.1f}    {'meets (c)' if ok else 'misses (c)'}")
        if ok and (best is None or b < best[0]):
            best = (b, rate)
    lines.append("")
    lines.append("no rate meets (c)" if best is None else f"lowest (b) among the rates that meet (c): shorten_rate = {best[1]:g}")
    lines.append(f"the library's default: shorten_rate = {hip.ReprojectMomentsParams.default().shorten_rate:g}")


def cpu_variance(lines):
    import denoise_variance_util as vu
    from qaray_amd import hip
    rows = {}
    for which in ("textures", "box"):
        p = vu.oracle_preview(which)
        ns = p["ns"].astype(np.uint32)
        i = vu.luma_rmse(hip.denoise_guided_host(p["acc"], p["depth"], ns, None, p["albedo"]), p["truth"])
        trusted = p["variance"] >= 0
        lines.append(f"{vu.QUALITY_SCENES[which]}: raw 4-spp frame {vu.luma_rmse(p['raw'], p['truth']):.4f}, accumulated {vu.luma_rmse(p['acc'], p['truth']):.4f}, "
                     f"guided (i) {i:.4f}; trusted pixels {trusted.mean():.3f}, mean out_variance {float(p['variance'][trusted].mean()):.3g}")
        for s in vu.VARIANCE_SCALES:
            ii = vu.luma_rmse(hip.denoise_variance_host(p["acc"], p["depth"], ns, None, p["albedo"], p["variance"], variance_scale=s), p["truth"])
            rows.setdefault(s, {})[which] = (ii, ii / i)
    lines.append("")
    lines.append(f"{'':<24}{'textures (ii)':<16}{'(ii) / (i)':<14}{'box (ii)':<12}{'(ii) / (i)'}")
    best = None
    for s, r in rows.items():
        ok = r["box"][1] <= 1.02
        lines.append(f"{f'variance_scale = {s:g}':<24}{r['textures'][0]:<16.4f}{r['textures'][1]:<14.4f}{r['box'][0]:<12.4f}{r['box'][1]:<10.4f}"
                     f"{'' if ok else 'box above 1.02'}")
        if ok and (best is None or r["textures"][1] < best[0]):
            best = (r["textures"][1], s)
    lines.append("")
    if best is None or best[0] >= 1.0:
        lines.append("no scale gives (ii) < (i) on the textured scene: the variance form is not worth shipping")
    else:
        lines.append(f"lowest (ii) / (i) on the textured scene among the scales within 1.02 on the box: variance_scale = {best[1]:g}")
    lines.append(f"the library's default: variance_scale = {hip.DenoiseVarianceParams.default().variance_scale:g}")


def gpu_confirm(lines):
    import torch
    import denoise_variance_util as vu
    import reproject_motion_util as mu
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    if not torch.cuda.is_available():
        raise SystemExit("reproject_moments_quality --gpu: no GPU (nothing is measured without one)")
    ctx = hip.Context(0)
    blob = load_scene_blob(os.path.join(SCENES_DIR, mu.PREVIEW_SCENE), size=mu.PREVIEW_SIZE)

    def rmse(scenario, **kw):
        r = mu.preview_run(ctx, blob, scenario, **kw)
        return mu.luma_rmse(r["acc"], r["truth"]), mu.luma_rmse(r["raw"], r["truth"]), float(r["length"].mean())

    b_off, c_off = rmse("light", clamp=False), rmse("still", clamp=False)
    b_clamp, c_clamp = rmse("light", clamp=True), rmse("still", clamp=True)
    b_short, c_short = rmse("light", clamp=True, shorten=True), rmse("still", clamp=True, shorten=True)
    lines.append(f"{'':<24}{'(b) light quartered':<22}{'(c) still scene':<18}mean length (b) / (c)")
    lines.append(f"{'raw 4-spp frame':<24}{b_off[1]:<22.4f}{c_off[1]:.4f}")
    lines.append(f"{'clamp off':<24}{b_off[0]:<22.4f}{c_off[0]:<18.4f}{b_off[2]:.1f} / {c_off[2]:.1f}")
    lines.append(f"{'clamp alone (4j)':<24}{b_clamp[0]:<22.4f}{c_clamp[0]:<18.4f}{b_clamp[2]:.1f} / {c_clamp[2]:.1f}")
    lines.append(f"{'(c) must lie below':<24}{'':<22}{0.5 * (c_off[1] + c_off[0]):.4f}")
    lines.append(f"{'clamp + shorten':<24}{b_short[0]:<22.4f}{c_short[0]:<18.4f}{b_short[2]:.1f} / {c_short[2]:.1f}")
    lines.append("")
    for which in ("textures", "box"):
        q = vu.device_quality(ctx, which)
        lines.append(f"{vu.QUALITY_SCENES[which]}: raw 4-spp frame {q['raw']:.4f}, accumulated {q['acc']:.4f}, guided (i) {q['i']:.4f}, variance form (ii) {q['ii']:.4f}, "
                     f"(ii) / (i) {q['ii'] / q['i']:.4f}; trusted pixels {q['trusted']:.3f}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpu", action="store_true", help="confirm the chosen rows on the device instead of running the CPU sweeps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_moments_quality.txt"), help="written by the CPU sweeps; --gpu appends to it")
    a = ap.parse_args()
    lines = []
    if a.gpu:
        head = "tools/reproject_moments_quality.py --gpu: the chosen rows on one MI355X, the renderer's own frames and planes\n\n"
        gpu_confirm(lines)
    else:
        head = ("tools/reproject_moments_quality.py: the sweeps behind shorten_rate and variance_scale on the CPU - the oracle's frames, the host builds "
                "of the reprojection and the filter; luma RMSE to a 256-spp frame\n\n")
        lines.append("shorten_rate: custom_softshadow.xml at 64x48, eight 4-spp frames, still camera, no ids")
        lines.append("")
        cpu_shorten(lines)
        lines += ["", "variance_scale: eight 4-spp frames at 64x64 accumulated with the moments; filters at their defaults, albedo guide only", ""]
        cpu_variance(lines)
    text = head + "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.gpu else "w") as f:
        f.write(("\n" if a.gpu else "") + text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
