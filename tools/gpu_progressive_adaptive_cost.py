#!/usr/bin/env python3
"""What a noisiest-first pass of a progressive frame costs and what it buys (profiles/progressive_adaptive_cost.txt).
One MI355X; every time is the median of --repeats after --warmup calls, between two events on one stream.  Three steps, each a run
of its own (the caller gives each its own time limit):

  overhead W H   the Cornell box at W x H, a frame of 4 .. 64 spp after advance(4).  With progressive_tile_limit 1 a pass renders
                 one tile whatever it selects, so the selection's own work shows: E = the error map alone (tile_error_device),
                 A = advance_tiles_device(8, the mask of the noisiest quarter), B = advance_adaptive(8, fraction 0.25) - the same
                 tiles, found on the device.  B - A is what the error map and the radix select add to a pass, B - A - E the select
                 alone.  U = a uniform advance(4) of the whole fresh frame (restart before each), the pass the overhead rides on.
  uniform W H    U alone, through the calls every earlier version of the library has: run it with --tree on a checkout of the
                 parent commit and its own library, in the same visit
  quality        RMSE of the preview against the finished frame as a function of the samples taken (counters), for uniform
                 doubling passes (spp_min, 2 spp_min, ...) and for advance(spp_min) followed by noisiest-quarter passes
                 (advance_adaptive(T, fraction 0.25) until no tile can gain) under two policies: "ladder", T = 2 x the lowest
                 level among the tiles that can still gain (every fourth pass it stands where the uniform frame stands), and
                 "to_spp_max", T = spp_max.  Each adaptive pass is a row: its budget and RMSE, what the uniform frame showed
                 within that budget (its last whole pass), its next pass, and what a uniform pass stopped at that budget would
                 show if all its tiles were alike (the mean square error interpolated linearly in the samples).

The step runs in a child process under a time limit (--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no
fallback."""
import os
import sys

import numpy as np

import cost

TOOL = "gpu_progressive_adaptive_cost"

QUALITY = (("example_project3_sphere.xml", (64, 48), 4, 32),      # the adaptive golden's scene and frame
           ("example_project12_box.xml", (256, 256), 8, 512),
           ("example_project7_object.xml", (256, 144), 4, 256))    # the scene of the C3 crop


def timed(stream, a, before, call):
    return cost.summary(cost.timed(stream, call, a.warmup, a.repeats, before=before))


def overhead(a, torch, hip, blob_of, uniform_only):
    w, h = a.size
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    ctx.upload_scene(blob_of("example_project12_box.xml", (w, h)))
    s = torch.cuda.Stream(dev)
    region = (0, 0, w, h)
    row = {"step": "uniform" if uniform_only else "overhead", "size": [w, h], "library": cost.library(), "kernel": None}
    with ctx.progressive(region, 4, spp_max=64) as prog:

        def fresh():
            prog.restart()
            ctx.synchronize()

        row["U_uniform_advance_4spp"] = timed(s, a, fresh, lambda: prog.advance(4, stream=s.cuda_stream))
        row["kernel"] = ctx.kernel_name()
        if not uniform_only:
            ty, tx = prog.tile_shape
            row["tiles"] = ty * tx
            fresh()
            prog.advance(4)
            mask, info = hip.tile_select_host(prog.tile_error(), prog.tile_levels(), 8, -(-ty * tx // 4))
            row["candidates"], row["selected"] = info["candidates"], info["selected"]
            d_mask = torch.from_numpy(mask.astype(np.uint8)).to(dev)
            d_err = torch.empty((ty, tx), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            row["E_error_map"] = timed(s, a, None, lambda: prog.tile_error_device(out=d_err, stream=s.cuda_stream))
            ctx.set_option("progressive_tile_limit", 1)
            row["A_masked_pass_of_one_tile"] = timed(s, a, None, lambda: prog.advance_tiles(8, d_mask, stream=s.cuda_stream))
            row["B_adaptive_pass_of_one_tile"] = timed(s, a, None, lambda: prog.advance_adaptive(8, fraction=0.25, stream=s.cuda_stream))
            ctx.set_option("progressive_tile_limit", 0)
            b, m, e = (row[k]["median_ms"] for k in ("B_adaptive_pass_of_one_tile", "A_masked_pass_of_one_tile", "E_error_map"))
            row["B_minus_A_ms"] = round(b - m, 4)
            row["select_alone_ms"] = round(b - m - e, 4)
            row["B_minus_A_share_of_U"] = round((b - m) / row["U_uniform_advance_4spp"]["median_ms"], 4)
    ctx.close()
    cost.emit(TOOL, f"{row['step']} {w}x{h}", **row)


def quality(a, torch, hip, blob_of):
    ctx = hip.Context(0)
    for scene, size, lo, hi in QUALITY:
        ctx.upload_scene(blob_of(scene, size))
        region = (0, 0) + size
        final = ctx.render_region(region, lo, spp_max=hi)[0].astype(np.float64)

        def point(prog):
            return ctx.counters()["samples"], float(np.sqrt(np.mean((prog.read()[0].astype(np.float64) - final) ** 2)))

        ctx.reset_counters()
        uniform = []
        with ctx.progressive(region, lo, spp_max=hi) as prog:
            t = lo
            while True:
                prog.advance(t)
                uniform.append((t,) + point(prog))
                if t >= hi:
                    break
                t = min(2 * t, hi)
        curves = {}
        for policy in ("ladder", "to_spp_max"):
            ctx.reset_counters()
            curve = []
            with ctx.progressive(region, lo, spp_max=hi) as prog:
                ty, tx = prog.tile_shape
                prog.advance(lo)
                curve.append(point(prog))
                for _ in range(64 * ty * tx):
                    levels, error = prog.tile_levels(), prog.tile_error()
                    if not (error > 0).any():
                        break
                    t = min(2 * int(levels[error > 0].min()), hi) if policy == "ladder" else hi
                    prog.advance_adaptive(t, fraction=0.25)
                    curve.append(point(prog))
            curves[policy] = curve
        cost.emit(TOOL, f"quality {scene}", step="quality", scene=scene, size=list(size), spp=[lo, hi], kernel=ctx.kernel_name(),
                  uniform_total_samples=uniform[-1][1], uniform_final_rmse=uniform[-1][2],
                  **{f"{p}_{k}": v for p, c in curves.items() for k, v in (("passes", len(c)), ("total_samples", c[-1][0]), ("final_rmse", c[-1][1]))})
        # at every budget an adaptive pass ended on: what the uniform frame showed by then (its last pass within the budget), and its next pass
        for policy, curve in curves.items():
            for samples, rmse in curve:
                had = [u for u in uniform if u[1] <= samples]
                nxt = [u for u in uniform if u[1] > samples]
                mix = None   # a uniform pass stopped at this budget, were its tiles all alike: the mean square error falls linearly in the samples
                if had and nxt:
                    f = (samples - had[-1][1]) / (nxt[0][1] - had[-1][1])
                    mix = round(float(np.sqrt((1 - f) * had[-1][2] ** 2 + f * nxt[0][2] ** 2)), 6)
                cost.emit(TOOL, f"quality {scene} {policy} {samples}", step="quality_row", scene=scene, policy=policy, samples=samples, rmse=round(rmse, 6),
                          uniform_stopped_here_if_tiles_alike=mix, uniform_within_budget=[had[-1][1], round(had[-1][2], 6)] if had else None,
                          uniform_next_pass=[nxt[0][1], round(nxt[0][2], 6)] if nxt else None)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=("all",))
    ap.add_argument("step", choices=("overhead", "uniform", "quality"))
    ap.add_argument("size", type=int, nargs="*", default=[1920, 1080])
    ap.add_argument("--tree", default=cost.ROOT, help="the checkout whose package and library are measured (default: this one)")
    a = ap.parse_args()
    if not a.one:
        cost.run_children(__file__, [["all"]], sys.argv[1:], a.limit)
        return
    torch, hip = cost.gpu(TOOL, os.path.abspath(a.tree))
    from qaray_amd.host import load_scene_blob
    assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
    cost.assets(a.tree)   # the object scene's stand-in mesh
    if a.step == "quality":
        quality(a, torch, hip, lambda scene, size: load_scene_blob(scene, size=size))
    else:
        if len(a.size) != 2:
            raise SystemExit("overhead / uniform: W H")
        overhead(a, torch, hip, lambda scene, size: load_scene_blob(scene, size=size), a.step == "uniform")


if __name__ == "__main__":
    main()
