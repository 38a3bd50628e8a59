#!/usr/bin/env python3
"""What one preview of a progressive frame costs, two ways, in one process (Cost):

  (A) the host's way: qa_progressive_read (20 bytes per pixel of floats to the host) + FrameBuffer::Deposit (three powf per pixel
      on one host thread) + ComputeZBufferImage + ComputeSampleCountImage
  (B) qa_progressive_display: the 8-bit products computed on the device from the frame's own slabs, 7 bytes per pixel to the host

on the C2 frame (Cornell box, 1920x1080) and the C5 frame (tower, 3840x2160), mid-frame (every pixel unfinished: the running mean
out of the 32-byte state) and at the frame's end (every pixel finished).  Wall time: warm-up, then the median of --repeats calls,
each ending in a device synchronise.  Kernel time: HIP events around qa_progressive_display_device (the 16-byte reset of the
statistics block, the statistics kernel and the encode kernel) on a stream of its own, median of --repeats.  The bytes per pixel are
derived from what the kernels read and write (csrc/hip/qa_display.hip); their sum over the kernel time is the achieved bandwidth,
given as a share of the HBM peak (8.0 TB/s specified; about 6.3 TB/s is what a float4 copy reaches).

The measurement runs in a child process under a time limit (--limit seconds), by the rule of tools/cost.py.  Needs a GPU: there is no
fallback, and without one this fails."""
import ctypes as C
import statistics
import sys

import numpy as np

import cost

TOOL = "gpu_display_cost"
HBM_PEAK = 8.0e12
# bytes per pixel of the two kernels, all seven product bytes wanted (qa_display.hip)
BYTES = {"unfinished": {"statistics": 32 + 4 + 4, "encode": 32 + 4 + 4 + 7}, "finished": {"statistics": 32 + 4 + 4, "encode": 32 + 4 + 4 + 12 + 7},
         "plain": {"statistics": 4 + 4, "encode": 12 + 4 + 4 + 7}}


def measure(a):
    torch, hip = cost.gpu(TOOL)
    from qaray_amd import host
    cost.assets()
    L, H = hip.lib(), host.lib()
    ctx = hip.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    for name in a.frames.split(","):
        scene, w, h = cost.frame(name)
        n = w * h
        ctx.upload_scene(host.load_scene_blob(scene, size=(w, h)))
        prog = ctx.progressive((0, 0, w, h), a.spp)
        fb = host.FrameBuffer(w, h)
        rgb, depth, ns = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.uint32)
        out = [np.zeros((h, w, 3) if k == 0 else (h, w), np.uint8) for k in range(5)]
        dout = {k: torch.empty(3 * n if k == "color" else n, dtype=torch.uint8, device=dev) for k in ("color", "count", "zimg", "countimg", "mask")}
        dout["stats"] = torch.empty(4, dtype=torch.int32, device=dev)
        st = hip.DisplayStats()

        def way_a(k):
            hip._check(L.qa_progressive_read(ctx._h, rgb.ctypes.data, depth.ctypes.data, ns.ctypes.data))
            host._check(H.qa_fb_deposit(fb._h, 0, 0, w, h, rgb.ctypes.data, depth.ctypes.data, ns.ctypes.data, a.spp, 1))
            H.qa_fb_z_image(fb._h)
            H.qa_fb_sample_count_image(fb._h)

        def way_b(k):
            hip._check(L.qa_progressive_display(ctx._h, 1, *(x.ctypes.data for x in out), C.byref(st)))

        def kernels_ms(fn):
            return statistics.median(cost.timed(stream, fn, a.warmup, a.repeats))

        for state, target in (("unfinished", max(1, a.spp // 2)), ("finished", a.spp)):
            prog.advance(target)
            ctx.synchronize()
            ta, tb = cost.walls(way_a, a.warmup, a.repeats), cost.walls(way_b, a.warmup, a.repeats)
            ma, mb = statistics.median(ta), statistics.median(tb)
            same = bool(np.array_equal(out[0], fb.pixels) and np.array_equal(out[2], fb.z_image) and np.array_equal(out[3], fb.sample_count_image))
            k_ms = kernels_ms(lambda: prog.display_device(srgb=True, stream=stream.cuda_stream, **dout))
            bpp = sum(BYTES[state].values())
            cost.emit(TOOL, f"{name} {state}", frame=name, size=[w, h], pixels_state=state, spp_reached=target, A_read_deposit_images_ms=round(ma, 3),
                      A_min_max_ms=[round(min(ta), 3), round(max(ta), 3)], B_progressive_display_ms=round(mb, 3), B_min_max_ms=[round(min(tb), 3), round(max(tb), 3)],
                      A_over_B=round(ma / mb, 2), products_equal=same, kernels_ms=round(k_ms, 4), bytes_per_pixel=BYTES[state],
                      kernel_GBps=round(bpp * n / (k_ms * 1e-3) / 1e9, 1), share_of_hbm_peak_8TBps=round(bpp * n / (k_ms * 1e-3) / HBM_PEAK, 4),
                      bytes_to_host_per_pixel={"A": 20, "B": 7})
        # the plain-buffer source: the same two kernels over the float preview of the finished frame
        t = (torch.empty(3 * n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        prog.read_device(*t)
        ctx.synchronize()
        k_ms = kernels_ms(lambda: ctx.display_device(*t, a.spp, srgb=True, stream=stream.cuda_stream, **dout))
        bpp = sum(BYTES["plain"].values())
        cost.emit(TOOL, f"{name} plain", frame=name, size=[w, h], pixels_state="plain buffers (qa_display_device)", kernels_ms=round(k_ms, 4), bytes_per_pixel=BYTES["plain"],
                  kernel_GBps=round(bpp * n / (k_ms * 1e-3) / 1e9, 1), share_of_hbm_peak_8TBps=round(bpp * n / (k_ms * 1e-3) / HBM_PEAK, 4))
        prog.close()
        fb.close()
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=("all",))
    ap.add_argument("--frames", default="C2,C5")
    ap.add_argument("--spp", type=int, default=8, help="the frame's spp; the mid-frame preview is taken at half of it")
    a = ap.parse_args()
    if a.one:
        return measure(a)
    cost.run_children(__file__, [["all"]], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
