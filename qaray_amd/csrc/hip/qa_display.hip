// qa_display.hip — the FrameBuffer's 8-bit products computed on the device (qa_display_*, qa_progressive_display*): a statistics
// kernel and an encode kernel over qa_display_dev.h, reading either plain rgb / depth / sample-count buffers or the progressive
// frame's own slabs (the preview qa_prog_resolve would write is formed in registers and never stored).
//
// Both kernels are memory-bound.  Bytes per pixel, P = products wanted (colour 3, count 1, z image 1, count image 1, mask 1: at most 7):
//   statistics  plain: depth 4 + ns 4 = 8 read                  progressive: + the 32-byte state line (one word of it used) = 40 read
//   encode      plain: rgb 12 + depth 4 + ns 4 = 20 read, P written
//               progressive: state 32 + depth 4 + ns 4 (+ rgb 12 of a finished pixel) = 40 .. 52 read, P written
// tools/gpu_display_cost.py puts these beside the measured times.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "qa_ctx.h"
#include "qa_display_dev.h"

namespace qa {

// state = null: the plain buffers.  Else the progressive frame: 8 words per pixel ([1] samples taken | bit 31 finished, [2..4] the
// running mean), rgb / ns hold the finished pixels' outputs and depth sample 0's hit distance (qa_progressive.hip, qa_prog_resolve)
struct DisplaySrc {
  const float *rgb, *depth;
  const uint32_t *ns, *state;
};
struct DisplayOut {
  uint8_t *color, *count, *zimg, *countimg, *mask;
  qa_display_stats *stats;
};

template <bool PROG>
__device__ __forceinline__ uint32_t displaySamples(const DisplaySrc &s, size_t q, uint32_t nsOut)
{
  if (!PROG) return nsOut;
  const uint32_t w = s.state[8 * q + 1];
  return (w & 0x80000000u) ? nsOut : w;
}
template <bool PROG>
__device__ __forceinline__ DisplayPixel displayLoad(const DisplaySrc &s, size_t q, float z, uint32_t nsOut)
{
  DisplayPixel p;
  p.z = z;
  if (PROG) {
    const uint4 a = reinterpret_cast<const uint4 *>(s.state)[2 * q];
    if (!(a.y & 0x80000000u)) {
      p.r = __uint_as_float(a.z); p.g = __uint_as_float(a.w); p.b = __uint_as_float(s.state[8 * q + 4]);
      p.ns = a.y;
      return p;
    }
  }
  p.r = s.rgb[3 * q]; p.g = s.rgb[3 * q + 1]; p.b = s.rgb[3 * q + 2];
  p.ns = nsOut;
  return p;
}

// block[0..3]: zmin and zmax as keys (displayKey), smin, smax; set to the initial values before every launch.  `groups` runs of four
// pixels are read with 16-byte loads, the pixels from 4 * groups on one by one (the tail, or everything when a buffer is not aligned)
template <bool PROG>
__global__ __launch_bounds__(256) void qa_display_reduce(DisplaySrc src, uint32_t npix, uint32_t groups, int sppMax, uint32_t *block)
{
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, total = gridDim.x * 256u;
  DisplayAcc acc = displayAccInit();
  for (uint32_t g = tid; g < groups; g += total) {
    const float4 d = reinterpret_cast<const float4 *>(src.depth)[g];
    const uint4 n = reinterpret_cast<const uint4 *>(src.ns)[g];
    const float z[4] = {d.x, d.y, d.z, d.w};
    const uint32_t m[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      DisplayPixel p;
      p.z = z[k];
      p.ns = displaySamples<PROG>(src, 4 * (size_t) g + k, m[k]);
      displayAccPixel(acc, displayDepth(p), displayCount(p, sppMax));
    }
  }
  for (uint32_t q = 4u * groups + tid; q < npix; q += total) {
    DisplayPixel p;
    p.z = src.depth[q];
    p.ns = displaySamples<PROG>(src, q, src.ns[q]);
    displayAccPixel(acc, displayDepth(p), displayCount(p, sppMax));
  }
  // inside the wave, then the workgroup's four waves through LDS, then one set of atomics per workgroup
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    DisplayAcc o;
    o.zmin = __shfl_xor(acc.zmin, off); o.zmax = __shfl_xor(acc.zmax, off);
    o.smin = __shfl_xor(acc.smin, off); o.smax = __shfl_xor(acc.smax, off);
    displayAccMerge(acc, o);
  }
  __shared__ DisplayAcc part[4];
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) displayAccMerge(acc, part[w]);
    atomicMin(&block[0], displayKey(acc.zmin));
    atomicMax(&block[1], displayKey(acc.zmax));
    atomicMin(&block[2], acc.smin);
    atomicMax(&block[3], acc.smax);
  }
}

// Every lane takes four consecutive pixels: their 12 colour bytes leave as three dwords, the one-byte images as one dword each.
// The pixels from 4 * groups on are written byte by byte.
template <bool PROG>
__global__ __launch_bounds__(256) void qa_display_encode(DisplaySrc src, uint32_t npix, uint32_t groups, int sppMax, int useSRGB, const uint32_t *block,
                                                         DisplayOut out)
{
  DisplayAcc st;
  st.zmin = displayUnkey(block[0]); st.zmax = displayUnkey(block[1]); st.smin = block[2]; st.smax = block[3];
  displayStatsEnd(st);
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, total = gridDim.x * 256u;
  if (tid == 0 && out.stats) {
    out.stats->zmin = st.zmin; out.stats->zmax = st.zmax; out.stats->smin = st.smin; out.stats->smax = st.smax;
  }
  const bool srgb = useSRGB != 0;
  for (uint32_t g = tid; g < groups; g += total) {
    const float4 d = reinterpret_cast<const float4 *>(src.depth)[g];
    const uint4 n = reinterpret_cast<const uint4 *>(src.ns)[g];
    const float z[4] = {d.x, d.y, d.z, d.w};
    const uint32_t m[4] = {n.x, n.y, n.z, n.w};
    DisplayPixel p[4];
    if (PROG) {
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = displayLoad<true>(src, 4 * (size_t) g + k, z[k], m[k]);
    } else {
      const float4 *c = reinterpret_cast<const float4 *>(src.rgb) + 3 * (size_t) g;
      const float4 c0 = c[0], c1 = c[1], c2 = c[2];
      const float v[12] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { p[k].r = v[3 * k]; p[k].g = v[3 * k + 1]; p[k].b = v[3 * k + 2]; p[k].z = z[k]; p[k].ns = m[k]; }
    }
    DisplayBytes b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = displayEncode(p[k], st, sppMax, srgb);
    if (out.color) {
      uint32_t *w = reinterpret_cast<uint32_t *>(out.color) + 3 * (size_t) g;
      w[0] = b[0].r | (uint32_t) b[0].g << 8 | (uint32_t) b[0].b << 16 | (uint32_t) b[1].r << 24;
      w[1] = b[1].g | (uint32_t) b[1].b << 8 | (uint32_t) b[2].r << 16 | (uint32_t) b[2].g << 24;
      w[2] = b[2].b | (uint32_t) b[3].r << 8 | (uint32_t) b[3].g << 16 | (uint32_t) b[3].b << 24;
    }
    if (out.count) reinterpret_cast<uint32_t *>(out.count)[g] = b[0].count | (uint32_t) b[1].count << 8 | (uint32_t) b[2].count << 16 | (uint32_t) b[3].count << 24;
    if (out.zimg) reinterpret_cast<uint32_t *>(out.zimg)[g] = b[0].z | (uint32_t) b[1].z << 8 | (uint32_t) b[2].z << 16 | (uint32_t) b[3].z << 24;
    if (out.countimg)
      reinterpret_cast<uint32_t *>(out.countimg)[g] = b[0].countImg | (uint32_t) b[1].countImg << 8 | (uint32_t) b[2].countImg << 16 | (uint32_t) b[3].countImg << 24;
    if (out.mask) reinterpret_cast<uint32_t *>(out.mask)[g] = b[0].mask | (uint32_t) b[1].mask << 8 | (uint32_t) b[2].mask << 16 | (uint32_t) b[3].mask << 24;
  }
  for (uint32_t q = 4u * groups + tid; q < npix; q += total) {
    const DisplayBytes b = displayEncode(displayLoad<PROG>(src, q, src.depth[q], src.ns[q]), st, sppMax, srgb);
    if (out.color) { out.color[3 * (size_t) q] = b.r; out.color[3 * (size_t) q + 1] = b.g; out.color[3 * (size_t) q + 2] = b.b; }
    if (out.count) out.count[q] = b.count;
    if (out.zimg) out.zimg[q] = b.z;
    if (out.countimg) out.countimg[q] = b.countImg;
    if (out.mask) out.mask[q] = b.mask;
  }
}

}  // namespace qa

static bool Aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The two kernels on s.  The context's statistics block (made on first use: 4 working words, then their initial values) is one per
// context, so a call on another stream than the last one waits for it
static int Display(qa_ctx *c, const DisplaySrc &src, uint64_t npix, int spp_max, int use_srgb, const DisplayOut &out, hipStream_t s)
{
  if (npix == 0) return Fail(QA_EINVAL, "no pixels");
  if (npix > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");   // (32-bit pixel indices in the kernels' grid-stride loops)
  if (spp_max < 1) return Fail(QA_EINVAL, "bad spp_max");
  if (!src.rgb || !src.depth || !src.ns) return Fail(QA_EINVAL, "null source buffer");
  if (!c->dDisplay) {
    HIP_TRY(hipMalloc((void **) &c->dDisplay, 8 * sizeof(uint32_t)));
    const DisplayAcc a = displayAccInit();
    const uint32_t init[8] = {0, 0, 0, 0, displayKey(a.zmin), displayKey(a.zmax), a.smin, a.smax};
    HIP_TRY(hipMemcpy(c->dDisplay, init, sizeof(init), hipMemcpyHostToDevice));
  }
  HIP_TRY(c->lastDisplay.WaitOn(s));
  HIP_TRY(hipMemcpyAsync(c->dDisplay, c->dDisplay + 4, 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  // the 16-byte loads and the dword stores want aligned buffers; otherwise every pixel takes the one-by-one path
  const bool vec = Aligned(src.rgb, 16) && Aligned(src.depth, 16) && Aligned(src.ns, 16) && Aligned(out.color, 4) && Aligned(out.count, 4) &&
                   Aligned(out.zimg, 4) && Aligned(out.countimg, 4) && Aligned(out.mask, 4);
  const uint32_t n = (uint32_t) npix, groups = vec ? n / 4u : 0u;
  const uint32_t items = groups + (n - 4u * groups);
  const uint32_t cap = (uint32_t) c->numCUs * 8u;
  const uint32_t blocks = std::max(1u, std::min((items + 255u) / 256u, cap));
  const bool prog = src.state != nullptr;
  hipLaunchKernelGGL(prog ? qa::qa_display_reduce<true> : qa::qa_display_reduce<false>, dim3(blocks), dim3(256), 0, s, src, n, groups, spp_max, c->dDisplay);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(prog ? qa::qa_display_encode<true> : qa::qa_display_encode<false>, dim3(blocks), dim3(256), 0, s, src, n, groups, spp_max, use_srgb,
                     c->dDisplay, out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(c->lastDisplay.Record(s));
  return QA_OK;
}

extern "C" {

int qa_display_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, uint64_t npix, int spp_max, int use_srgb,
                      uint8_t *d_color, uint8_t *d_count, uint8_t *d_zimg, uint8_t *d_countimg, uint8_t *d_mask, qa_display_stats *d_stats,
                      void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  const DisplaySrc src = {d_rgb, d_depth, d_ns, nullptr};
  const DisplayOut out = {d_color, d_count, d_zimg, d_countimg, d_mask, d_stats};
  return Display(c, src, npix, spp_max, use_srgb, out, StreamOf(c, hip_stream));
}

int qa_progressive_display_device(qa_ctx *c, int use_srgb, uint8_t *d_color, uint8_t *d_count, uint8_t *d_zimg, uint8_t *d_countimg,
                                  uint8_t *d_mask, qa_display_stats *d_stats, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  const qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.done.WaitOn(s));
  const DisplaySrc src = {f.args.rgb, f.args.depth, f.args.ns, f.dState};
  const DisplayOut out = {d_color, d_count, d_zimg, d_countimg, d_mask, d_stats};
  return Display(c, src, f.npix, f.args.sppMax, use_srgb, out, s);
}

int qa_progressive_display(qa_ctx *c, int use_srgb, uint8_t *color, uint8_t *count, uint8_t *zimg, uint8_t *countimg, uint8_t *mask,
                           qa_display_stats *stats)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  // the products' staging belongs to the context and only grows: [colour | count | z image | count image | mask | statistics]
  const size_t n = c->prog.npix, slot = (n + 15) & ~(size_t) 15, need = 3 * slot + 4 * slot + 16;
  HIP_TRY(c->displayStage.Reserve(need, false, c->stream));
  uint8_t *d = static_cast<uint8_t *>(c->displayStage.p);
  uint8_t *dv[5] = {color ? d : nullptr, count ? d + 3 * slot : nullptr, zimg ? d + 4 * slot : nullptr, countimg ? d + 5 * slot : nullptr,
                    mask ? d + 6 * slot : nullptr};
  qa_display_stats *ds = stats ? reinterpret_cast<qa_display_stats *>(d + 7 * slot) : nullptr;
  if ((rc = qa_progressive_display_device(c, use_srgb, dv[0], dv[1], dv[2], dv[3], dv[4], ds, nullptr)) != QA_OK) return rc;
  uint8_t *hv[5] = {color, count, zimg, countimg, mask};
  for (int k = 0; k < 5; ++k)
    if (hv[k]) HIP_TRY(hipMemcpyAsync(hv[k], dv[k], (k == 0 ? 3 : 1) * n, hipMemcpyDeviceToHost, c->stream));
  if (stats) HIP_TRY(hipMemcpyAsync(stats, ds, sizeof(qa_display_stats), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

// the same source on the CPU, pixel after pixel (no GPU, no context)
int qa_test_display_host(const float *rgb, const float *depth, const uint32_t *ns, uint64_t npix, int spp_max, int use_srgb, uint8_t *color,
                         uint8_t *count, uint8_t *zimg, uint8_t *countimg, uint8_t *mask, qa_display_stats *stats)
{
  if (!rgb || !depth || !ns || npix == 0 || spp_max < 1) return QA_EINVAL;
  DisplayAcc st = displayAccInit();
  DisplayPixel p;
  for (uint64_t q = 0; q < npix; ++q) {
    p.z = depth[q]; p.ns = ns[q];
    displayAccPixel(st, displayDepth(p), displayCount(p, spp_max));
  }
  displayStatsEnd(st);
  if (stats) { stats->zmin = st.zmin; stats->zmax = st.zmax; stats->smin = st.smin; stats->smax = st.smax; }
  for (uint64_t q = 0; q < npix; ++q) {
    p.r = rgb[3 * q]; p.g = rgb[3 * q + 1]; p.b = rgb[3 * q + 2]; p.z = depth[q]; p.ns = ns[q];
    const DisplayBytes b = displayEncode(p, st, spp_max, use_srgb != 0);
    if (color) { color[3 * q] = b.r; color[3 * q + 1] = b.g; color[3 * q + 2] = b.b; }
    if (count) count[q] = b.count;
    if (zimg) zimg[q] = b.z;
    if (countimg) countimg[q] = b.countImg;
    if (mask) mask[q] = b.mask;
  }
  return QA_OK;
}

}  // extern "C"
