#!/usr/bin/env python3
"""What filtering a preview costs: Context.denoise_device of a frame of float results between two events on the
caller's stream, at 1920x1080 and 3840x2160 and 1, 3 and 5 iterations: warm-up calls, then the median of --repeats.

Beside the milliseconds, the algorithmic bytes as GB/s and as a share of the HBM peak (8.0 TB/s specified; about 6.3 TB/s is what
a float4 copy reaches).  Algorithmic bytes per pixel: the guide kernel reads 20 (rgb, depth, sample count) and writes 24 (colour
and variance 16, depth and slope 8); an iteration reads 24 and writes 16, the last one 12 (the caller's rgb) - 44 + 40 n - 4 for
n iterations.  The 24 neighbour taps of a pixel are re-reads of those bytes (LDS at steps 1 and 2, the caches beyond).

The frame is synthetic (a noisy colour gradient on a slanted plane, a tenth of the pixels missing the scene): the filter's
work does not depend on what the pixels show, only on how many taps share a class.  The measurement runs in a child process under a
time limit (--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no fallback."""
import statistics
import sys

import numpy as np

import cost

TOOL = "gpu_denoise_cost"
SIZES = ((1920, 1080), (3840, 2160))
ITERATIONS = (1, 3, 5)
HBM_PEAK = 8.0e12


def measure(a):
    torch, hip = cost.gpu(TOOL)
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    s = torch.cuda.Stream(dev)
    for w, h in SIZES:
        r = np.random.default_rng(w)
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        rgb = (np.stack([x / w, y / h, 0.5 + 0 * x], axis=2) + 0.3 * r.random((h, w, 3), dtype=np.float32)).astype(np.float32)
        depth = (3 + 0.01 * x + 0.02 * y).astype(np.float32)
        depth[r.random((h, w)) < 0.1] = np.float32(1e30)
        t = (torch.from_numpy(rgb).to(dev), torch.from_numpy(depth).to(dev), torch.full((h, w), 4, dtype=torch.int32, device=dev))
        out = torch.empty_like(t[0])
        torch.cuda.synchronize()
        for iterations in ITERATIONS:
            spans = cost.timed(s, lambda: ctx.denoise_device(*t, out=out, iterations=iterations, stream=s.cuda_stream), a.warmup, a.repeats)
            ms = statistics.median(spans)
            moved = w * h * (44 + 40 * iterations - 4)
            cost.emit(TOOL, f"{w}x{h} iterations {iterations}", size=[w, h], iterations=iterations, **cost.summary(spans), algorithmic_bytes=moved,
                      GBps=round(moved / (ms * 1e-3) / 1e9, 1), share_of_hbm_peak_8TBps=round(moved / (ms * 1e-3) / HBM_PEAK, 4))
    ctx.close()


def main():
    a = cost.arguments(__doc__, one=("all",)).parse_args()
    if a.one:
        return measure(a)
    cost.run_children(__file__, [["all"]], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
