// qa_progressive.hip — progressive frames (qa_progressive_*): a resident image refined in sample passes, each a launch of the frame's
// integrator (LaunchSetup / LaunchFrame, qa_frame.hip) between the small kernels below
#include <algorithm>

#include "qa_seed.h"
#include "qa_ctx.h"

namespace qa {
// ---- progressive frames (qa_progressive_*): the pixel state slab is RenderParams::pix_state's layout, 8 words per pixel at its output
// index q (row-major in the region): [0] RNG state, [1] samples taken | bit 31 finished, [2..4] running mean, [5..7] running variance
// qa_progressive_begin: every pixel's fresh state (what qa_integrate's section A sets up for a pixel's first sample), nothing rendered
__global__ __launch_bounds__(256) void qa_prog_init(uint32_t *state, float *rgb, float *depth, uint32_t *ns, int x0, int y0, uint32_t rw, uint32_t npix,
                                                    uint32_t width, uint32_t seed)
{
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= npix) return;
  const uint32_t px = (uint32_t) x0 + q % rw, py = (uint32_t) y0 + q / rw;
  uint4 *st = reinterpret_cast<uint4 *>(state) + 2 * (size_t) q;
  st[0] = make_uint4(qa_pixel_seed(seed, py * width + px), 0u, 0u, 0u);
  st[1] = make_uint4(0u, 0u, 0u, 0u);
  rgb[3 * (size_t) q] = 0.f; rgb[3 * (size_t) q + 1] = 0.f; rgb[3 * (size_t) q + 2] = 0.f;
  depth[q] = QA_BIGFLOAT;
  ns[q] = 0u;
}
// after a pass to `target` samples: the tiles whose pass is complete are at the target now.  tile_progress is indexed by the work item's
// place in the pass's tile order (qa_integrate, section A: 2 once the item is complete); every word is 1 again for the next pass (its
// work items are all "chunk 1": the wait for chunk 0 ends at once)
__global__ __launch_bounds__(256) void qa_prog_levels(uint32_t *progress, const uint32_t *order, uint32_t *level, uint32_t tiles, uint32_t target)
{
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= tiles) return;
  if (progress[p] >= 2u) {
    const uint32_t t = order ? order[p] : p;
    if (level[t] < target) level[t] = target;
  }
  progress[p] = 1u;
}
// a pass to a target some tiles already reached (the same target again after a stop): only the tiles below it are handed out, so that
// no pixel takes a sample beyond the target.  They go, in launch order, to the END of list[tiles], and the pass's work counter starts
// so that its items are the last min(count, limit) of them.  One wave walks the order (a rare path; the order decides the schedule only)
__global__ __launch_bounds__(64) void qa_prog_select(const uint32_t *order, const uint32_t *level, uint32_t tiles, uint32_t target, uint32_t limit,
                                                     uint32_t *list, unsigned int *work)
{
  const uint32_t lane = threadIdx.x;
  uint32_t k = 0;   // tiles selected so far
  for (uint32_t b = 0; b < tiles; b += 64) {
    const bool valid = b + lane < tiles;
    const uint32_t p = valid ? tiles - 1u - (b + lane) : 0u;   // (backwards from the order's end)
    const uint32_t t = valid ? (order ? order[p] : p) : 0u;
    const bool need = valid && level[t] < target;
    const unsigned long long m = __ballot(need);
    if (need) list[tiles - 1u - (k + (uint32_t) __popcll(m & ((1ull << lane) - 1ull)))] = t;
    k += (uint32_t) __popcll(m);
  }
  if (lane == 0) *work = (2u * tiles - ((limit && limit < k) ? limit : k)) * 64u;
}
// the preview: finished pixels' final mean and sample count, the running mean and the samples so far of the others (rgb 0, ns 0 where
// nothing was taken yet); depth is sample 0's hit distance (1e30 before it)
__global__ __launch_bounds__(256) void qa_prog_resolve(const uint32_t *state, const float *rgb, const float *depth, const uint32_t *ns, uint32_t npix,
                                                       float *outRgb, float *outDepth, uint32_t *outNs)
{
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= npix) return;
  const uint4 a = reinterpret_cast<const uint4 *>(state)[2 * (size_t) q];
  const uint32_t mz = state[8 * (size_t) q + 4];
  if (a.y & 0x80000000u) {
    outRgb[3 * (size_t) q] = rgb[3 * (size_t) q]; outRgb[3 * (size_t) q + 1] = rgb[3 * (size_t) q + 1]; outRgb[3 * (size_t) q + 2] = rgb[3 * (size_t) q + 2];
    outNs[q] = ns[q];
  } else {
    outRgb[3 * (size_t) q] = __uint_as_float(a.z); outRgb[3 * (size_t) q + 1] = __uint_as_float(a.w); outRgb[3 * (size_t) q + 2] = __uint_as_float(mz);
    outNs[q] = a.y;
  }
  outDepth[q] = depth[q];
}
// qa_progressive_status: out[0] finished pixels, out[1] tiles below `target`, out[2] the lowest tile level (zeroed / set to ~0 before)
__global__ __launch_bounds__(256) void qa_prog_status(const uint32_t *state, uint32_t npix, const uint32_t *level, uint32_t tiles, uint32_t target,
                                                      unsigned long long *out)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool fin = i < npix && (state[8 * (size_t) i + 1] & 0x80000000u);
  const bool behind = i < tiles && level[i] < target;
  const unsigned long long mf = __ballot(fin), mb = __ballot(behind);
  if (__lane_id() == 0) {
    if (mf) atomicAdd(&out[0], (unsigned long long) __popcll(mf));
    if (mb) atomicAdd(&out[1], (unsigned long long) __popcll(mb));
  }
  if (i < tiles) atomicMin(&out[2], (unsigned long long) level[i]);
}
}  // namespace qa

// What begin and restart share: every pixel's fresh state, no tile at any level, nothing in hand (on the context's stream)
static int ProgReset(qa_ctx *c)
{
  qa_ctx::Progressive &f = c->prog;
  const FrameArgs &a = f.args;
  hipLaunchKernelGGL(qa::qa_prog_init, dim3((unsigned) ((f.npix + 255) / 256)), dim3(256), 0, c->stream, f.dState, a.rgb, a.depth, a.ns, a.x0, a.y0,
                     (uint32_t) (a.x1 - a.x0), (uint32_t) f.npix, (uint32_t) c->ds.cam.width, a.seed);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(f.dLevel, 0, f.tiles * sizeof(uint32_t), c->stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) f.dProgress, 1, f.tiles, c->stream));
  HIP_TRY(f.done.Record(c->stream));
  f.target = f.top = 0;
  f.stale = false;
  return QA_OK;
}

extern "C" {

int qa_progressive_begin(qa_ctx *c, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce, uint32_t seed, uint32_t flags)
{
  if (int rc = Enter(c)) return rc;
  const FrameArgs a = {x0, y0, x1, y1, 0, 1, spp_min, spp_max, max_bounce, seed, flags, nullptr, nullptr, nullptr, nullptr};
  if (int rc = CheckFrame(c, a)) return rc;
  if (flags & ~QA_RENDER_STATS) return Fail(QA_EINVAL, "unknown flags");
  const unsigned tiles = (unsigned) ((x1 - x0 + 7) / 8) * (unsigned) ((y1 - y0 + 7) / 8);
  // a pass's work counter runs from tiles * 64 to 2 * tiles * 64 (plus 64 per exiting wave) in 32 bits
  if ((unsigned long long) tiles * 64ull * 2ull >= 0xF0000000ull) return Fail(QA_EINVAL, "region too large for a progressive frame");
  EndProgressive(c, nullptr);
  qa_ctx::Progressive &f = c->prog;
  f.ended.clear();
  f.args = a;
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  hipError_t e = hipSuccess;
  if ((e = hipMalloc((void **) &f.dState, npix * 8 * sizeof(uint32_t))) != hipSuccess || (e = hipMalloc((void **) &f.dLevel, tiles * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc((void **) &f.dProgress, tiles * sizeof(uint32_t))) != hipSuccess || (e = hipMalloc((void **) &f.args.rgb, npix * 3 * sizeof(float))) != hipSuccess ||
      (e = hipMalloc((void **) &f.args.depth, npix * sizeof(float))) != hipSuccess || (e = hipMalloc((void **) &f.args.ns, npix * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc((void **) &f.dStatus, 3 * sizeof(unsigned long long))) != hipSuccess || (e = hipMalloc((void **) &f.dList, tiles * sizeof(uint32_t))) != hipSuccess) {
    EndProgressive(c, nullptr);
    return Fail(e == hipErrorOutOfMemory ? QA_ENOMEM : QA_EHIP, std::string("progressive frame slabs: ") + hipGetErrorString(e));
  }
  f.tiles = tiles;
  f.npix = npix;
  if (int rc = ProgReset(c)) return rc;
  f.active = true;
  return QA_OK;
}

int qa_progressive_restart(qa_ctx *c)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = CheckFrame(c, c->prog.args)) return rc;   // (the edited scene may refuse the frame: area lights, bounce > 7)
  HIP_TRY(c->prog.done.WaitOn(c->stream));   // the last pass, on whatever stream it ran
  return ProgReset(c);
}

// the frame's status on the context's stream (synchronises)
static int ProgStatus(qa_ctx *c, int *reached, uint64_t *finished, uint64_t *behind)
{
  qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.done.WaitOn(c->stream));
  HIP_TRY(hipMemsetAsync(f.dStatus, 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(hipMemsetAsync(f.dStatus + 2, 0xFF, sizeof(unsigned long long), c->stream));
  const size_t n = std::max(f.npix, (size_t) f.tiles);
  hipLaunchKernelGGL(qa::qa_prog_status, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, c->stream, f.dState, (uint32_t) f.npix, f.dLevel, f.tiles,
                     (uint32_t) f.target, f.dStatus);
  HIP_TRY(hipGetLastError());
  unsigned long long h[3];
  HIP_TRY(hipMemcpyAsync(h, f.dStatus, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (reached) *reached = (int) h[2];
  if (finished) *finished = h[0];
  if (behind) *behind = h[1];
  return QA_OK;
}

int qa_progressive_advance(qa_ctx *c, int spp_target, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (spp_target < 1) return Fail(QA_EINVAL, "bad spp target");
  qa_ctx::Progressive &f = c->prog;
  if (f.stale) return Fail(QA_EINVAL, "the scene was edited since this progressive frame began: qa_progressive_restart or qa_progressive_begin first");
  const int target = std::min(spp_target, f.args.sppMax);
  // Every unfinished pixel of a tile has exactly the tile's level in samples (a tile in hand always completes its pass).  Above every
  // earlier target, no pixel has the target yet; at or below the highest, some tiles may have it (a stop left others behind): the
  // pass then hands out the tiles below the target alone - or nothing happens when there are none (this asks the device)
  const bool reissue = target <= f.top;
  if (reissue) {
    int reached = 0;
    if ((rc = ProgStatus(c, &reached, nullptr, nullptr)) != QA_OK) return rc;
    if (reached >= target) return QA_OK;
  }
  hipStream_t s = StreamOf(c, hip_stream);
  if ((rc = EnsureHalton(c, f.args.sppMax)) != QA_OK) return rc;   // (a one-shot frame in between may have reallocated the table)
  HIP_TRY(f.done.WaitOn(s));   // the frame's setup / last pass, on whatever stream it ran
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  Launch L;
  FrameArgs a = f.args;
  a.stream = s;
  if ((rc = LaunchSetup(c, L, a, (a.y1 - a.y0 + 7) / 8, work, true)) != QA_OK) return rc;
  // every work item is "chunk 1" of its tile: the counter starts past chunk 0 (qa_integrate, section A), so every pixel resumes from its
  // state and ends its chunk on chunk_spp + 1 * chunk_tail = target samples.  progressive_tile_limit (tests): only the last n items are
  // left, as if stopped
  const uint32_t limit = c->optProgTileLimit;
  if (reissue) {
    hipLaunchKernelGGL(qa::qa_prog_select, dim3(1), dim3(64), 0, s, L.rp.tile_order, f.dLevel, f.tiles, (uint32_t) target, limit, f.dList, work);
    HIP_TRY(hipGetLastError());
    L.rp.tile_order = f.dList;
  } else {
    const unsigned take = (limit && limit < f.tiles) ? limit : f.tiles;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) work, (int) ((2u * f.tiles - take) * 64u), 1, s));
  }
  L.rp.chunk_spp = (uint32_t) target; L.rp.chunk_tail = 0; L.rp.num_chunks = 2;
  L.rp.tile_progress = f.dProgress; L.rp.pix_state = f.dState;
  if ((rc = LaunchFrame(c, L, false, s)) != QA_OK) return rc;
  hipLaunchKernelGGL(qa::qa_prog_levels, dim3((f.tiles + 255) / 256), dim3(256), 0, s, f.dProgress, L.rp.tile_order, f.dLevel, f.tiles, (uint32_t) target);
  HIP_TRY(hipGetLastError());
  HIP_TRY(f.done.Record(s));
  f.target = target;
  f.top = std::max(f.top, target);
  return QA_OK;
}

int qa_progressive_read_device(qa_ctx *c, float *d_rgb, float *d_depth, uint32_t *d_ns, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  if (!d_rgb || !d_depth || !d_ns) return Fail(QA_EINVAL, "null output buffer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  const qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.done.WaitOn(s));
  hipLaunchKernelGGL(qa::qa_prog_resolve, dim3((unsigned) ((f.npix + 255) / 256)), dim3(256), 0, s, f.dState, f.args.rgb, f.args.depth, f.args.ns, (uint32_t) f.npix,
                     d_rgb, d_depth, d_ns);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

int qa_progressive_read(qa_ctx *c, float *rgb, float *depth, uint32_t *ns)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!rgb || !depth || !ns) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.prevRgb.Reserve(f.npix * 3 * sizeof(float)));   // (the frame's size is fixed and EndProgressive frees them: they never grow)
  HIP_TRY(f.prevDepth.Reserve(f.npix * sizeof(float)));
  HIP_TRY(f.prevNs.Reserve(f.npix * sizeof(uint32_t)));
  if ((rc = qa_progressive_read_device(c, (float *) f.prevRgb.p, (float *) f.prevDepth.p, (uint32_t *) f.prevNs.p, nullptr)) != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, f.prevRgb.p, f.prevRgb.cap, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(depth, f.prevDepth.p, f.prevDepth.cap, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(ns, f.prevNs.p, f.prevNs.cap, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

int qa_progressive_status(qa_ctx *c, int *spp_reached, uint64_t *pixels_finished, uint64_t *tiles_behind)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return ProgStatus(c, spp_reached, pixels_finished, tiles_behind);
}

int qa_progressive_end(qa_ctx *c)
{
  if (int rc = Enter(c)) return rc;
  EndProgressive(c, nullptr);
  c->prog.ended.clear();
  return QA_OK;
}

}  // extern "C"
