// qa_progressive.hip — progressive frames (qa_progressive_*): a resident image refined in sample passes, each a launch of the frame's
// integrator (LaunchSetup / LaunchFrame, qa_frame.hip) between the small kernels below
#include <algorithm>

#include "qa_seed.h"
#include "qa_ctx.h"
#include "qa_prog_error_dev.h"

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
// ---- tile-selective and noisiest-first passes (qa_progressive_advance_tiles / _adaptive; qa_prog_error_dev.h is the specification)
// An exclusive scan of v over the workgroup's 1024 threads (16 waves; wsum: 16 words of LDS) and the workgroup's total
__device__ __forceinline__ uint32_t progBlockScan(uint32_t v, uint32_t *wsum, uint32_t &total)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();   // (the last scan's sums are read by now)
  if (lane == 63u) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (uint32_t w = 0; w < 16u; ++w) {
    const uint32_t x = wsum[w];
    if (w < wave) base += x;
    all += x;
  }
  total = all;
  return base + inc - v;
}
// qa_prog_select with the caller's choice: the tiles below the target whose mask byte is set go, in launch order, to the END of
// list[tiles], and the work counter starts so that the pass's items are the last min(count, limit) of them.  One workgroup walks the
// order backwards, 4096 places a turn (every pass of this kind runs it: 4 places per thread keep the two dependent loads in flight)
__global__ __launch_bounds__(1024) void qa_prog_select_mask(const uint32_t *order, const uint32_t *level, const uint8_t *mask, uint32_t tiles, uint32_t target,
                                                            uint32_t limit, uint32_t *list, unsigned int *work)
{
  __shared__ uint32_t wsum[16];
  uint32_t k = 0;   // tiles selected so far
  for (uint32_t b = 0; b < tiles; b += 4096u) {
    uint32_t t[4];
    bool need[4];
    uint32_t n = 0;
    for (uint32_t i = 0; i < 4u; ++i) {
      const uint32_t j = b + threadIdx.x * 4u + i;   // (the j-th place from the order's end)
      const bool valid = j < tiles;
      const uint32_t p = valid ? tiles - 1u - j : 0u;
      t[i] = valid ? (order ? order[p] : p) : 0u;
      need[i] = valid && mask[t[i]] != 0 && level[t[i]] < target;
      n += need[i] ? 1u : 0u;
    }
    uint32_t total;
    uint32_t at = k + progBlockScan(n, wsum, total);
    for (uint32_t i = 0; i < 4u; ++i)
      if (need[i]) list[tiles - 1u - at++] = t[i];
    k += total;
  }
  if (threadIdx.x == 0) *work = (2u * tiles - ((limit && limit < k) ? limit : k)) * 64u;
}
// The error map: one wave per tile, lane = slot; the sum by halving runs in the specification's order
__global__ __launch_bounds__(256) void qa_prog_tile_error(const uint32_t *state, uint32_t rw, uint32_t rh, uint32_t tilesX, uint32_t tiles, float *error)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (t >= tiles) return;   // (whole waves)
  const uint32_t x = (t % tilesX) * 8u + (lane & 7u), y = (t / tilesX) * 8u + (lane >> 3);
  const bool inside = x < rw && y < rh;
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
  if (inside) {
    const uint4 *st = reinterpret_cast<const uint4 *>(state) + 2 * ((size_t) y * rw + x);
    a = st[0];
    b = st[1];
  }
  float s = progSlotValue(inside, a.y, b.y, b.z, b.w);
  for (int half = 32; half >= 1; half >>= 1) s = s + __shfl_down(s, half);   // (lane l < half: a[l] + a[l + half]; the others are not read)
  if (lane == 0) error[t] = s * 0.015625f;
}
// Adds the wave's lanes that are `on` to their bins, one LDS atomic per distinct bin (the top byte of an error is the same few values
// for a whole frame: 64 lanes on one address would queue up)
__device__ __forceinline__ void progWaveCount(uint32_t *hist, bool on, uint32_t bin)
{
  unsigned long long left = __ballot(on);
  while (left) {
    const int first = __ffsll((long long) left) - 1;
    const uint32_t b = __shfl(bin, first);
    const unsigned long long same = __ballot(on && bin == b);
    if ((int) (threadIdx.x & 63u) == first) atomicAdd(&hist[b], (uint32_t) __popcll(same));
    left &= ~same;
  }
}
// The noisiest-first choice as a mask: one workgroup finds the cut by four rounds of an 8-bit radix select with its bins in LDS and
// marks the tiles in index order (ties: the first by index).  The first sweep reads the maps, writes every tile's key (0: no
// candidate) and counts the top byte; the others read the keys alone, four a lane.  keys and mask hold tiles rounded up to 4
// entries.  info: qa_progressive_adaptive_info's words
__global__ __launch_bounds__(1024) void qa_prog_adaptive_mask(const float *error, const uint32_t *level, uint32_t tiles, uint32_t target, uint32_t maxTiles,
                                                              float minError, uint32_t *keys, uint8_t *mask, unsigned long long *info)
{
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t sCand, sTop, sPrefix, sRemaining;
  const uint32_t padded = (tiles + 3u) & ~3u;
  if (threadIdx.x < 256u) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) sTop = 0;
  __syncthreads();
  uint32_t top = 0;
  for (uint32_t b = 0; b < padded; b += 4096u) {
    uint32_t key[4];
    for (uint32_t i = 0; i < 4u; ++i) {
      const uint32_t t = b + i * 1024u + threadIdx.x;
      const bool in = t < tiles;
      const float e = in ? error[t] : 0.f;
      const uint32_t lv = in ? level[t] : 0xFFFFFFFFu;
      key[i] = progCandidate(e, lv, target, minError) ? progBits(e) : 0u;
      if (t < padded) keys[t] = key[i];
    }
    for (uint32_t i = 0; i < 4u; ++i) {
      progWaveCount(hist, key[i] != 0u, key[i] >> 24);
      if (key[i] < QA_PROG_INF_BITS && key[i] > top) top = key[i];
    }
  }
  if (top) atomicMax(&sTop, top);
  __syncthreads();   // (the keys are the whole workgroup's from here on)
  if (threadIdx.x == 0) {
    uint32_t n = 0;
    for (int i = 0; i < 256; ++i) n += hist[i];
    uint32_t p = 0, r = progTake(n, maxTiles);
    sCand = n;
    if (r) progRadixPick(hist, 24u, p, r);
    sPrefix = p; sRemaining = r;
  }
  __syncthreads();
  const uint32_t candidates = sCand, take = progTake(candidates, maxTiles);
  const uint4 *keys4 = reinterpret_cast<const uint4 *>(keys);
  if (take) {
    for (uint32_t shift = 16u;; shift -= 8u) {
      if (threadIdx.x < 256u) hist[threadIdx.x] = 0;
      __syncthreads();
      const uint32_t prefix = sPrefix;
      for (uint32_t b = 0; b < padded; b += 4096u) {
        const uint32_t t = b + threadIdx.x * 4u;
        if (t < padded) {
          const uint4 k = keys4[t >> 2];
          const uint32_t key[4] = {k.x, k.y, k.z, k.w};
          for (uint32_t i = 0; i < 4u; ++i)
            if (key[i] && progRadixMatch(key[i], prefix, shift)) atomicAdd(&hist[(key[i] >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t p = prefix, r = sRemaining;
        progRadixPick(hist, shift, p, r);
        sPrefix = p; sRemaining = r;
      }
      __syncthreads();
      if (shift == 0u) break;
    }
  }
  const uint32_t cut = sPrefix, ties = sRemaining;
  uint32_t rank = 0;   // candidates with the cut key at lower indices than this turn's
  for (uint32_t b = 0; b < padded; b += 4096u) {
    const uint32_t t = b + threadIdx.x * 4u;
    uint4 k = make_uint4(0u, 0u, 0u, 0u);
    if (take && t < padded) k = keys4[t >> 2];
    const uint32_t key[4] = {k.x, k.y, k.z, k.w};
    uint32_t n = 0;
    for (uint32_t i = 0; i < 4u; ++i) n += (key[i] && key[i] == cut) ? 1u : 0u;
    uint32_t total;
    uint32_t before = rank + progBlockScan(n, wsum, total);
    uint32_t bytes = 0;
    for (uint32_t i = 0; i < 4u; ++i) {
      if (key[i] && progAdmit(key[i], cut, ties, before)) bytes |= 1u << (8u * i);
      if (key[i] && key[i] == cut) ++before;
    }
    if (t < padded) reinterpret_cast<uint32_t *>(mask)[t >> 2] = bytes;
    rank += total;
  }
  if (threadIdx.x == 0) { info[0] = take; info[1] = candidates; info[2] = take ? cut : 0u; info[3] = sTop; }
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

// What every pass begins with: a frame, a target, pixels of the scene as it stands.  -> min(spp_target, spp_max)
static int ProgPassCheck(qa_ctx *c, int spp_target, int *target)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (spp_target < 1) return Fail(QA_EINVAL, "bad spp target");
  if (c->prog.stale) return Fail(QA_EINVAL, "the scene was edited since this progressive frame began: qa_progressive_restart or qa_progressive_begin first");
  *target = std::min(spp_target, c->prog.args.sppMax);
  return QA_OK;
}

// One pass to `target` on s.  mask null: every tile (reissue: every tile below the target, qa_prog_select); a device mask: its tiles
// below the target (qa_prog_select_mask), whatever the targets before
static int ProgPass(qa_ctx *c, int target, hipStream_t s, bool reissue, const uint8_t *mask)
{
  int rc = QA_OK;
  qa_ctx::Progressive &f = c->prog;
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
  if (mask) {
    hipLaunchKernelGGL(qa::qa_prog_select_mask, dim3(1), dim3(1024), 0, s, L.rp.tile_order, f.dLevel, mask, f.tiles, (uint32_t) target, limit, f.dList, work);
    HIP_TRY(hipGetLastError());
    L.rp.tile_order = f.dList;
  } else if (reissue) {
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

int qa_progressive_advance(qa_ctx *c, int spp_target, void *hip_stream)
{
  int target = 0;
  int rc = ProgPassCheck(c, spp_target, &target);
  if (rc != QA_OK) return rc;
  qa_ctx::Progressive &f = c->prog;
  // Every unfinished pixel of a tile has exactly the tile's level in samples (a tile in hand always completes its pass).  Above every
  // earlier target, no pixel has the target yet; at or below the highest, some tiles may have it (a stop or a selective pass left
  // others behind): the pass then hands out the tiles below the target alone - or nothing happens when there are none (this asks
  // the device)
  const bool reissue = target <= f.top;
  if (reissue) {
    int reached = 0;
    if ((rc = ProgStatus(c, &reached, nullptr, nullptr)) != QA_OK) return rc;
    if (reached >= target) return QA_OK;
  }
  return ProgPass(c, target, StreamOf(c, hip_stream), reissue, nullptr);
}

// The slabs of the selective passes, on first use
static int ProgTileSlabs(qa_ctx *c)
{
  qa_ctx::Progressive &f = c->prog;
  if (f.dInfo) return QA_OK;
  const size_t padded = ((size_t) f.tiles + 3) & ~(size_t) 3;   // (qa_prog_adaptive_mask works on four tiles a lane)
  hipError_t e = hipSuccess;
  if ((!f.dError && (e = hipMalloc((void **) &f.dError, f.tiles * sizeof(float))) != hipSuccess) ||
      (!f.dMask && (e = hipMalloc((void **) &f.dMask, padded)) != hipSuccess) ||
      (!f.dKeys && (e = hipMalloc((void **) &f.dKeys, padded * sizeof(uint32_t))) != hipSuccess) ||
      (!f.hMask && (e = hipHostMalloc((void **) &f.hMask, f.tiles, hipHostMallocDefault)) != hipSuccess) ||
      (!f.maskCopied && (e = hipEventCreateWithFlags(&f.maskCopied, hipEventDisableTiming)) != hipSuccess))
    return Fail(e == hipErrorOutOfMemory ? QA_ENOMEM : QA_EHIP, std::string("progressive tile slabs: ") + hipGetErrorString(e));
  unsigned long long *info = nullptr;
  HIP_TRY(hipMalloc((void **) &info, 4 * sizeof(unsigned long long)));
  if (hipError_t z = hipMemsetAsync(info, 0, 4 * sizeof(unsigned long long), c->stream); z != hipSuccess) {
    (void) hipFree(info);
    return Fail(QA_EHIP, std::string("progressive tile slabs: ") + hipGetErrorString(z));
  }
  f.dInfo = info;
  HIP_TRY(hipStreamSynchronize(c->stream));   // (the first use may be on another stream: the zeros are there before it)
  return QA_OK;
}

static int ProgNeedsVariance(qa_ctx *c)
{
  if (c->prog.args.sppMin >= c->prog.args.sppMax)
    return Fail(QA_EUNSUPPORTED, "this progressive frame keeps no variance (spp_min == spp_max): begin it with spp_min < spp_max for an error estimate");
  return QA_OK;
}

// the error map of the frame as the stream's earlier work leaves it -> d_error
static int ProgErrorMap(qa_ctx *c, float *d_error, hipStream_t s)
{
  const qa_ctx::Progressive &f = c->prog;
  const uint32_t rw = (uint32_t) (f.args.x1 - f.args.x0), rh = (uint32_t) (f.args.y1 - f.args.y0);
  hipLaunchKernelGGL(qa::qa_prog_tile_error, dim3((f.tiles + 3) / 4), dim3(256), 0, s, f.dState, rw, rh, (rw + 7u) / 8u, f.tiles, d_error);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

int qa_progressive_tile_count(qa_ctx *c, int *tiles_x, int *tiles_y)
{
  if (int rc = ProgActive(c)) return rc;
  const FrameArgs &a = c->prog.args;
  if (tiles_x) *tiles_x = (a.x1 - a.x0 + 7) / 8;
  if (tiles_y) *tiles_y = (a.y1 - a.y0 + 7) / 8;
  return QA_OK;
}

int qa_progressive_advance_tiles_device(qa_ctx *c, int spp_target, const uint8_t *d_tile_mask, void *hip_stream)
{
  int target = 0;
  if (int rc = ProgPassCheck(c, spp_target, &target)) return rc;
  if (!d_tile_mask) return Fail(QA_EINVAL, "null tile mask");
  return ProgPass(c, target, StreamOf(c, hip_stream), false, d_tile_mask);
}

int qa_progressive_advance_tiles(qa_ctx *c, int spp_target, const uint8_t *tile_mask, void *hip_stream)
{
  int target = 0;
  if (int rc = ProgPassCheck(c, spp_target, &target)) return rc;
  if (!tile_mask) return Fail(QA_EINVAL, "null tile mask");
  if (int rc = ProgTileSlabs(c)) return rc;
  qa_ctx::Progressive &f = c->prog;
  hipStream_t s = StreamOf(c, hip_stream);
  // the pinned bytes are one per frame: the last call's copy has left them (it usually has long ago), and the last pass has read dMask
  HIP_TRY(hipEventSynchronize(f.maskCopied));
  std::copy(tile_mask, tile_mask + f.tiles, f.hMask);
  HIP_TRY(f.done.WaitOn(s));
  HIP_TRY(hipMemcpyAsync(f.dMask, f.hMask, f.tiles, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(f.maskCopied, s));
  return ProgPass(c, target, s, false, f.dMask);
}

int qa_progressive_advance_adaptive(qa_ctx *c, int spp_target, uint32_t max_tiles, float min_error, void *hip_stream)
{
  int target = 0;
  if (int rc = ProgPassCheck(c, spp_target, &target)) return rc;
  if (int rc = ProgNeedsVariance(c)) return rc;
  if (!(min_error >= 0.f)) return Fail(QA_EINVAL, "min_error must not be negative or a NaN");
  if (int rc = ProgTileSlabs(c)) return rc;
  qa_ctx::Progressive &f = c->prog;
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(f.done.WaitOn(s));
  if (int rc = ProgErrorMap(c, f.dError, s)) return rc;
  hipLaunchKernelGGL(qa::qa_prog_adaptive_mask, dim3(1), dim3(1024), 0, s, f.dError, f.dLevel, f.tiles, (uint32_t) target, max_tiles, min_error, f.dKeys, f.dMask, f.dInfo);
  HIP_TRY(hipGetLastError());
  return ProgPass(c, target, s, false, f.dMask);
}

int qa_progressive_adaptive_info(qa_ctx *c, uint64_t out[4])
{
  if (int rc = ProgActive(c)) return rc;
  if (!out) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!f.dInfo) return QA_OK;   // (no adaptive pass yet)
  unsigned long long h[4];
  HIP_TRY(f.done.WaitOn(c->stream));
  HIP_TRY(hipMemcpyAsync(h, f.dInfo, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < 4; ++i) out[i] = h[i];
  return QA_OK;
}

int qa_progressive_tile_levels_device(qa_ctx *c, uint32_t *d_levels, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  if (!d_levels) return Fail(QA_EINVAL, "null output buffer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(c->prog.done.WaitOn(s));
  HIP_TRY(hipMemcpyAsync(d_levels, c->prog.dLevel, c->prog.tiles * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  return QA_OK;
}

int qa_progressive_tile_levels(qa_ctx *c, uint32_t *levels)
{
  if (int rc = ProgActive(c)) return rc;
  if (!levels) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->prog.done.WaitOn(c->stream));
  HIP_TRY(hipMemcpyAsync(levels, c->prog.dLevel, c->prog.tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

int qa_progressive_tile_error_device(qa_ctx *c, float *d_error, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  if (!d_error) return Fail(QA_EINVAL, "null output buffer");
  if (int rc = ProgNeedsVariance(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(c->prog.done.WaitOn(s));
  return ProgErrorMap(c, d_error, s);
}

int qa_progressive_tile_error(qa_ctx *c, float *error)
{
  if (int rc = ProgActive(c)) return rc;
  if (!error) return Fail(QA_EINVAL, "null argument");
  if (int rc = ProgNeedsVariance(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = ProgTileSlabs(c)) return rc;
  qa_ctx::Progressive &f = c->prog;
  // (dError is the adaptive pass's too: behind the last pass, on the context's stream, nothing else touches it)
  HIP_TRY(f.done.WaitOn(c->stream));
  if (int rc = ProgErrorMap(c, f.dError, c->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(error, f.dError, f.tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

int qa_progressive_state(qa_ctx *c, uint32_t *state)
{
  if (int rc = ProgActive(c)) return rc;
  if (!state) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->prog.done.WaitOn(c->stream));
  HIP_TRY(hipMemcpyAsync(state, c->prog.dState, c->prog.npix * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

int qa_test_tile_error_host(const uint32_t *state, int width, int height, float *error)
{
  if (!state || !error || width < 1 || height < 1) return Fail(QA_EINVAL, "bad argument");
  const uint32_t rw = (uint32_t) width, rh = (uint32_t) height, tx = (rw + 7u) / 8u, ty = (rh + 7u) / 8u;
  for (uint32_t t = 0; t < tx * ty; ++t) {
    float a[64];
    for (uint32_t l = 0; l < 64u; ++l) {
      const uint32_t x = (t % tx) * 8u + (l & 7u), y = (t / tx) * 8u + (l >> 3);
      const bool inside = x < rw && y < rh;
      const uint32_t *st = state + (inside ? 8 * ((size_t) y * rw + x) : 0);
      a[l] = progSlotValue(inside, st[1], st[5], st[6], st[7]);
    }
    error[t] = progTileSum(a);
  }
  return QA_OK;
}

int qa_test_tile_select_host(const float *error, const uint32_t *levels, uint32_t tiles, uint32_t target, uint32_t max_tiles, float min_error, uint8_t *mask,
                             uint64_t info[4])
{
  if (!error || !levels || !mask || !tiles) return Fail(QA_EINVAL, "bad argument");
  if (!(min_error >= 0.f)) return Fail(QA_EINVAL, "min_error must not be negative or a NaN");
  uint64_t mine[4];
  progSelectHost(error, levels, tiles, target, max_tiles, min_error, mask, info ? info : mine);
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
