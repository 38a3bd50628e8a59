// qa_denoise.hip — the edge-avoiding a-trous filter of qa_denoise_dev.h on the device (qa_denoise_device, qa_progressive_denoise*,
// the guided form qa_denoise_guided_*, the variance form qa_denoise_variance_device) and the same source on the host (qa_test_denoise_host, qa_test_denoise_guided_host, qa_test_denoise_variance_host).  A guide kernel (pass 0) fills the context's working planes - colour and
// variance (16 bytes per pixel, two of them: the iterations go from one to the other), depth and slope (8 bytes) - from plain
// buffers or from the progressive frame's slabs; one kernel per iteration follows, the last of which writes the caller's rgb.
//
// Per pixel and iteration 16 + 8 bytes are read and 16 written once (12 by the last): 40 bytes of algorithmic traffic; the 24 other
// taps are re-reads of neighbours' entries.  Steps 1 and 2 stage a 16x16 tile and its halo of 2s (20x20 / 24x24 entries, 9.4 / 13.5 KB)
// in LDS, where the tile's taps overlap almost wholly; from step 4 on a lane's taps are 4+ pixels apart, the halo would be 32x32
// entries and more for 256 pixels, and the taps are loaded directly (16 + 8 bytes each; neighbouring lanes share the lines).
// tools/gpu_denoise_cost.py puts the traffic beside the measured times.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "qa_ctx.h"
#include "qa_denoise_dev.h"

namespace qa {

static_assert(sizeof(DenoiseColor) == 16 && sizeof(DenoiseGuide) == 8, "the planes are read with 16- and 8-byte loads");
#define QA_DENOISE_TILE 16

// state = null: the plain buffers.  Else the progressive frame's slabs, resolved as qa_prog_resolve does (qa_progressive.hip): the
// running mean and samples so far of an unfinished pixel, the outputs of a finished one
struct DenoiseSrc {
  const float *rgb, *depth;
  const uint32_t *ns, *state;
  int W;
  __device__ __forceinline__ DenoisePixel operator()(int x, int y) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    DenoisePixel p;
    p.z = depth[q];
    if (state) {
      const uint4 a = reinterpret_cast<const uint4 *>(state)[2 * q];
      if (!(a.y & 0x80000000u)) {
        p.r = __uint_as_float(a.z); p.g = __uint_as_float(a.w); p.b = __uint_as_float(state[8 * q + 4]);
        p.ns = a.y;
        return p;
      }
    }
    p.r = rgb[3 * q]; p.g = rgb[3 * q + 1]; p.b = rgb[3 * q + 2];
    p.ns = ns[q];
    return p;
  }
};

__global__ __launch_bounds__(256) void qa_denoise_guide(DenoiseSrc src, int W, int H, DenoiseColor *color, DenoiseGuide *guide)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  DenoiseColor c;
  DenoiseGuide g;
  denoiseGuide(src, x, y, W, H, c, g);
  const size_t q = (size_t) y * (size_t) W + (size_t) x;
  color[q] = c;
  guide[q] = g;
}

// Pass 0 of the variance form: qa_denoise_guide with the caller's variance plane, 4 more bytes per window pixel
struct DenoiseVarianceSrc {
  const float *variance;
  int W;
  __host__ __device__ __forceinline__ float operator()(int x, int y) const { return variance[(size_t) y * (size_t) W + (size_t) x]; }
};

__global__ __launch_bounds__(256) void qa_denoise_guide_variance(DenoiseSrc src, DenoiseVarianceSrc vsrc, float varianceScale, int W, int H,
                                                                 DenoiseColor *color, DenoiseGuide *guide)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  DenoiseColor c;
  DenoiseGuide g;
  denoiseGuideVariance(src, vsrc, varianceScale, x, y, W, H, c, g);
  const size_t q = (size_t) y * (size_t) W + (size_t) x;
  color[q] = c;
  guide[q] = g;
}

// the planes in global memory / a window of them in LDS whose entry (0, 0) is pixel (ox, oy)
struct DenoiseTapGlobal {
  const DenoiseColor *color;
  const DenoiseGuide *guide;
  int W;
  __device__ __forceinline__ void operator()(int x, int y, DenoiseColor &c, DenoiseGuide &g) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    c = color[q];
    g = guide[q];
  }
};
struct DenoiseTapLds {
  const DenoiseColor *color;
  const DenoiseGuide *guide;
  int ox, oy, pitch;
  __device__ __forceinline__ void operator()(int x, int y, DenoiseColor &c, DenoiseGuide &g) const
  {
    const int i = (y - oy) * pitch + (x - ox);
    c = color[i];
    g = guide[i];
  }
};

__device__ __forceinline__ void denoiseStore(const DenoiseColor &o, size_t q, DenoiseColor *outColor, float *outRgb)
{
  if (outRgb) { outRgb[3 * q] = o.r; outRgb[3 * q + 1] = o.g; outRgb[3 * q + 2] = o.b; }
  else outColor[q] = o;
}

// One iteration at step S = 1 or 2 over a 16x16 tile staged with its halo of 2 S.  Entries outside the image are not loaded and
// never read (denoiseIterate skips those taps).  outRgb != null: the last iteration, which writes the caller's frame
template <int S>
__global__ __launch_bounds__(256) void qa_denoise_iterate_lds(const DenoiseColor *color, const DenoiseGuide *guide, int W, int H, float sigmaColor,
                                                              float sigmaDepth, DenoiseColor *outColor, float *outRgb)
{
  constexpr int SIDE = QA_DENOISE_TILE + 4 * S;
  __shared__ DenoiseColor tc[SIDE * SIDE];
  __shared__ DenoiseGuide tg[SIDE * SIDE];
  const int ox = (int) (blockIdx.x * QA_DENOISE_TILE) - 2 * S, oy = (int) (blockIdx.y * QA_DENOISE_TILE) - 2 * S;
  for (int i = (int) threadIdx.x; i < SIDE * SIDE; i += 256) {
    const int gx = ox + i % SIDE, gy = oy + i / SIDE;
    if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
      const size_t q = (size_t) gy * (size_t) W + (size_t) gx;
      tc[i] = color[q];
      tg[i] = guide[q];
    }
  }
  __syncthreads();
  const int x = ox + 2 * S + (int) (threadIdx.x & 15u), y = oy + 2 * S + (int) (threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const DenoiseTapLds tap = {tc, tg, ox, oy, SIDE};
  denoiseStore(denoiseIterate(tap, x, y, W, H, S, sigmaColor, sigmaDepth), (size_t) y * (size_t) W + (size_t) x, outColor, outRgb);
}

// One iteration at any step, the taps loaded directly
__global__ __launch_bounds__(256) void qa_denoise_iterate_direct(const DenoiseColor *color, const DenoiseGuide *guide, int W, int H, int s, float sigmaColor,
                                                                 float sigmaDepth, DenoiseColor *outColor, float *outRgb)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  const DenoiseTapGlobal tap = {color, guide, W};
  denoiseStore(denoiseIterate(tap, x, y, W, H, s, sigmaColor, sigmaDepth), (size_t) y * (size_t) W + (size_t) x, outColor, outRgb);
}

// ---- the guided form: an aux plane (normal, albedo, valid / reliable bits: 32 bytes per pixel) beside the unguided planes; one kernel
// fills it, and the iterations load every tap directly (a tap reads 16 + 8 bytes and, where the centre is reliable, 32 more)
static_assert(sizeof(DenoiseAux) == 32, "the aux plane is read with two 16-byte loads");
struct DenoiseGuideSrc {
  const float *normal, *albedo;
  int W;
  __device__ __forceinline__ void operator()(int x, int y, float *n, float *a) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    if (normal) { n[0] = normal[3 * q]; n[1] = normal[3 * q + 1]; n[2] = normal[3 * q + 2]; }
    if (albedo) { a[0] = albedo[3 * q]; a[1] = albedo[3 * q + 1]; a[2] = albedo[3 * q + 2]; }
  }
};
struct DenoiseAuxGlobal {
  const DenoiseAux *aux;
  int W;
  __device__ __forceinline__ DenoiseAux operator()(int x, int y) const { return aux[(size_t) y * (size_t) W + (size_t) x]; }
};

__global__ __launch_bounds__(256) void qa_denoise_guided_aux(DenoiseSrc src, DenoiseGuideSrc gsrc, int W, int H, uint32_t flags, DenoiseAux *aux)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  aux[(size_t) y * (size_t) W + (size_t) x] = denoiseAux(src, gsrc, x, y, W, H, flags);
}

__global__ __launch_bounds__(256) void qa_denoise_guided_iterate(const DenoiseColor *color, const DenoiseGuide *guide, const DenoiseAux *aux, int W, int H,
                                                                 int s, float sigmaColor, float sigmaDepth, float sigmaNormal, DenoiseColor *outColor,
                                                                 float *outRgb)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  const DenoiseTapGlobal tap = {color, guide, W};
  const DenoiseAuxGlobal at = {aux, W};
  denoiseStore(denoiseIterateGuided(tap, at, x, y, W, H, s, sigmaColor, sigmaDepth, sigmaNormal), (size_t) y * (size_t) W + (size_t) x, outColor, outRgb);
}

}  // namespace qa

static int CheckParams(const qa_denoise_params *p, int width, int height)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  if (width < 1 || height < 1) return Fail(QA_EINVAL, "bad frame size");
  if ((uint64_t) width * (uint64_t) height > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");
  if (p->iterations < 0 || p->iterations > QA_DENOISE_MAX_ITERATIONS) return Fail(QA_EINVAL, "iterations outside 0 .. 6");
  if (!std::isfinite(p->sigma_color) || !(p->sigma_color > 0.f) || !std::isfinite(p->sigma_depth) || !(p->sigma_depth > 0.f))
    return Fail(QA_EINVAL, "a sigma that is not finite and positive");
  if (p->flags != 0u) return Fail(QA_EINVAL, "unknown flags");
  return QA_OK;
}

// Pass 0 on s: the variance form's kernel when the caller brought a variance plane, else qa_denoise_guide
static int LaunchPass0(const DenoiseSrc &src, const float *variance, float varianceScale, int W, int H, DenoiseColor *color, DenoiseGuide *guide, dim3 grid,
                       hipStream_t s)
{
  if (variance) {
    const DenoiseVarianceSrc vsrc = {variance, W};
    hipLaunchKernelGGL(qa::qa_denoise_guide_variance, grid, dim3(256), 0, s, src, vsrc, varianceScale, W, H, color, guide);
  } else {
    hipLaunchKernelGGL(qa::qa_denoise_guide, grid, dim3(256), 0, s, src, W, H, color, guide);
  }
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// The guide kernel and the iterations on s.  The working planes (40 bytes per pixel: [colour A | colour B | guide]) are one per
// context and only grow; a call on another stream than the last one waits for it
static int Denoise(qa_ctx *c, const DenoiseSrc &src, int W, int H, const qa_denoise_params &p, float *out, hipStream_t s, const float *variance = nullptr,
                   float varianceScale = 1.f)
{
  const size_t n = (size_t) W * (size_t) H;
  if (p.iterations == 0) {   // the input's bits (a progressive frame still has to be resolved: its callers never get here)
    if (out != src.rgb) HIP_TRY(hipMemcpyAsync(out, src.rgb, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return QA_OK;
  }
  HIP_TRY(c->denoisePlanes.Reserve(n * 40, true));   // (the old planes may be in use on a stream of the caller's)
  HIP_TRY(c->lastDenoise.WaitOn(s));
  DenoiseColor *plane[2] = {static_cast<DenoiseColor *>(c->denoisePlanes.p), static_cast<DenoiseColor *>(c->denoisePlanes.p) + n};
  DenoiseGuide *guide = reinterpret_cast<DenoiseGuide *>(plane[1] + n);
  const dim3 grid((unsigned) ((W + QA_DENOISE_TILE - 1) / QA_DENOISE_TILE), (unsigned) ((H + QA_DENOISE_TILE - 1) / QA_DENOISE_TILE)), block(256);
  if (int rc = LaunchPass0(src, variance, varianceScale, W, H, plane[0], guide, grid, s)) return rc;
  for (int i = 0; i < p.iterations; ++i) {
    const DenoiseColor *from = plane[i & 1];
    DenoiseColor *to = plane[(i + 1) & 1];
    float *rgb = (i == p.iterations - 1) ? out : nullptr;
    if (i == 0) hipLaunchKernelGGL(qa::qa_denoise_iterate_lds<1>, grid, block, 0, s, from, guide, W, H, p.sigma_color, p.sigma_depth, to, rgb);
    else if (i == 1) hipLaunchKernelGGL(qa::qa_denoise_iterate_lds<2>, grid, block, 0, s, from, guide, W, H, p.sigma_color, p.sigma_depth, to, rgb);
    else hipLaunchKernelGGL(qa::qa_denoise_iterate_direct, grid, block, 0, s, from, guide, W, H, 1 << i, p.sigma_color, p.sigma_depth, to, rgb);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(c->lastDenoise.Record(s));
  return QA_OK;
}

// Every form on the CPU, pixel after pixel, after the entry's checks: pass 0 (the variance form's with a variance plane), the aux
// plane when p.flags names a guide, and the iterations of the form that p.flags selects
static int DenoiseOnHost(const float *rgb, const float *depth, const uint32_t *ns, const float *normal, const float *albedo, const float *variance,
                         float varianceScale, int W, int H, const qa_denoise_guided_params &p, float *out_rgb)
{
  const size_t n = (size_t) W * (size_t) H;
  if (p.iterations == 0) {
    if (out_rgb != rgb) memcpy(out_rgb, rgb, n * 3 * sizeof(float));
    return QA_OK;
  }
  const bool guided = (p.flags & (QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO)) != 0u;
  std::vector<DenoiseColor> plane[2] = {std::vector<DenoiseColor>(n), std::vector<DenoiseColor>(n)};
  std::vector<DenoiseGuide> guide(n);
  std::vector<DenoiseAux> aux(guided ? n : 0);
  const auto src = [=](int x, int y) {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    DenoisePixel px;
    px.r = rgb[3 * q]; px.g = rgb[3 * q + 1]; px.b = rgb[3 * q + 2]; px.z = depth[q]; px.ns = ns[q];
    return px;
  };
  const auto gsrc = [=](int x, int y, float *nn, float *aa) {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    if (normal) { nn[0] = normal[3 * q]; nn[1] = normal[3 * q + 1]; nn[2] = normal[3 * q + 2]; }
    if (albedo) { aa[0] = albedo[3 * q]; aa[1] = albedo[3 * q + 1]; aa[2] = albedo[3 * q + 2]; }
  };
  const DenoiseVarianceSrc vsrc = {variance, W};
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t q = (size_t) y * W + x;
      if (variance) denoiseGuideVariance(src, vsrc, varianceScale, x, y, W, H, plane[0][q], guide[q]);
      else denoiseGuide(src, x, y, W, H, plane[0][q], guide[q]);
      if (guided) aux[q] = denoiseAux(src, gsrc, x, y, W, H, p.flags);
    }
  for (int i = 0; i < p.iterations; ++i) {
    const DenoiseColor *from = plane[i & 1].data();
    const DenoiseGuide *gd = guide.data();
    const DenoiseAux *ad = aux.data();
    const auto tap = [=](int x, int y, DenoiseColor &cc, DenoiseGuide &g) {
      const size_t q = (size_t) y * (size_t) W + (size_t) x;
      cc = from[q];
      g = gd[q];
    };
    const auto at = [=](int x, int y) { return ad[(size_t) y * (size_t) W + (size_t) x]; };
    std::vector<DenoiseColor> &to = plane[(i + 1) & 1];
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        to[(size_t) y * W + x] = guided ? denoiseIterateGuided(tap, at, x, y, W, H, 1 << i, p.sigma_color, p.sigma_depth, p.sigma_normal)
                                        : denoiseIterate(tap, x, y, W, H, 1 << i, p.sigma_color, p.sigma_depth);
  }
  const std::vector<DenoiseColor> &last = plane[p.iterations & 1];
  for (size_t q = 0; q < n; ++q) { out_rgb[3 * q] = last[q].r; out_rgb[3 * q + 1] = last[q].g; out_rgb[3 * q + 2] = last[q].b; }
  return QA_OK;
}

extern "C" {

int qa_denoise_params_default(qa_denoise_params *p)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->iterations = QA_DENOISE_DEFAULT_ITERATIONS;
  p->sigma_color = QA_DENOISE_DEFAULT_SIGMA_COLOR;
  p->sigma_depth = QA_DENOISE_DEFAULT_SIGMA_DEPTH;
  p->flags = 0u;
  return QA_OK;
}

int qa_denoise_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, int width, int height, const qa_denoise_params *p,
                      float *d_out_rgb, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (!d_rgb || !d_depth || !d_ns || !d_out_rgb) return Fail(QA_EINVAL, "null buffer");
  if (int rc = CheckParams(p, width, height)) return rc;
  const DenoiseSrc src = {d_rgb, d_depth, d_ns, nullptr, width};
  return Denoise(c, src, width, height, *p, d_out_rgb, StreamOf(c, hip_stream));
}

int qa_progressive_denoise_device(qa_ctx *c, const qa_denoise_params *p, float *d_rgb, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!d_rgb) return Fail(QA_EINVAL, "null buffer");
  const qa_ctx::Progressive &f = c->prog;
  const int W = f.args.x1 - f.args.x0, H = f.args.y1 - f.args.y0;
  if ((rc = CheckParams(p, W, H)) != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(f.done.WaitOn(s));
  if (p->iterations == 0) {   // the preview itself; depth and sample counts go to the frame's preview buffers
    qa_ctx::Progressive &g = c->prog;
    HIP_TRY(g.prevDepth.Reserve(f.npix * sizeof(float)));
    HIP_TRY(g.prevNs.Reserve(f.npix * sizeof(uint32_t)));
    return qa_progressive_read_device(c, d_rgb, (float *) g.prevDepth.p, (uint32_t *) g.prevNs.p, hip_stream);
  }
  const DenoiseSrc src = {f.args.rgb, f.args.depth, f.args.ns, f.dState, W};
  return Denoise(c, src, W, H, *p, d_rgb, s);
}

int qa_progressive_denoise(qa_ctx *c, const qa_denoise_params *p, float *rgb)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!rgb) return Fail(QA_EINVAL, "null buffer");
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.prevRgb.Reserve(f.npix * 3 * sizeof(float)));   // (the preview's buffer: the frame's size is fixed, it never grows)
  if ((rc = qa_progressive_denoise_device(c, p, (float *) f.prevRgb.p, nullptr)) != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, f.prevRgb.p, f.npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

// the same source on the CPU, pixel after pixel (no GPU, no context)
int qa_test_denoise_host(const float *rgb, const float *depth, const uint32_t *ns, int width, int height, const qa_denoise_params *p, float *out_rgb)
{
  if (!rgb || !depth || !ns || !out_rgb) return Fail(QA_EINVAL, "null buffer");
  if (int rc = CheckParams(p, width, height)) return rc;
  const qa_denoise_guided_params g = {p->iterations, p->sigma_color, p->sigma_depth, QA_DENOISE_DEFAULT_SIGMA_NORMAL, 0u};
  return DenoiseOnHost(rgb, depth, ns, nullptr, nullptr, nullptr, 1.f, width, height, g, out_rgb);
}

}  // extern "C"

static int CheckGuidedParams(const qa_denoise_guided_params *p, int width, int height, const void *normal, const void *albedo, bool planes)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  const qa_denoise_params u = {p->iterations, p->sigma_color, p->sigma_depth, 0u};
  if (int rc = CheckParams(&u, width, height)) return rc;
  if (!std::isfinite(p->sigma_normal) || !(p->sigma_normal > 0.f)) return Fail(QA_EINVAL, "a sigma that is not finite and positive");
  if (p->flags & ~(QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO)) return Fail(QA_EINVAL, "unknown flags");
  if (planes && ((normal != nullptr) != ((p->flags & QA_DENOISE_GUIDE_NORMAL) != 0u) || (albedo != nullptr) != ((p->flags & QA_DENOISE_GUIDE_ALBEDO) != 0u)))
    return Fail(QA_EINVAL, "a guide plane that disagrees with its flag");
  return QA_OK;
}

// The guided form on s (iterations >= 1, flags != 0).  Working planes [colour A | colour B | guide | aux | own normal | own albedo]:
// 40 + 32 bytes per pixel, and 24 more when the planes are the context's own (a progressive frame's, computed here: prog = true).
// Every entry is written before it is read, as in Denoise
static int DenoiseGuided(qa_ctx *c, const DenoiseSrc &src, const float *normal, const float *albedo, bool prog, int W, int H,
                         const qa_denoise_guided_params &p, float *out, hipStream_t s, void *hip_stream, const float *variance = nullptr,
                         float varianceScale = 1.f)
{
  const size_t n = (size_t) W * (size_t) H;
  HIP_TRY(c->denoisePlanes.Reserve(n * (prog ? 96 : 72), true));
  HIP_TRY(c->lastDenoise.WaitOn(s));
  DenoiseColor *plane[2] = {static_cast<DenoiseColor *>(c->denoisePlanes.p), static_cast<DenoiseColor *>(c->denoisePlanes.p) + n};
  DenoiseGuide *guide = reinterpret_cast<DenoiseGuide *>(plane[1] + n);
  DenoiseAux *aux = reinterpret_cast<DenoiseAux *>(guide + n);
  if (prog) {
    float *own = reinterpret_cast<float *>(aux + n);
    float *dN = (p.flags & QA_DENOISE_GUIDE_NORMAL) ? own : nullptr, *dA = (p.flags & QA_DENOISE_GUIDE_ALBEDO) ? own + 3 * n : nullptr;
    if (int rc = qa_progressive_gbuffer_device(c, dN, dA, nullptr, nullptr, hip_stream)) return rc;
    normal = dN; albedo = dA;
  }
  const dim3 grid((unsigned) ((W + QA_DENOISE_TILE - 1) / QA_DENOISE_TILE), (unsigned) ((H + QA_DENOISE_TILE - 1) / QA_DENOISE_TILE)), block(256);
  if (int rc = LaunchPass0(src, variance, varianceScale, W, H, plane[0], guide, grid, s)) return rc;
  const DenoiseGuideSrc gsrc = {normal, albedo, W};
  hipLaunchKernelGGL(qa::qa_denoise_guided_aux, grid, block, 0, s, src, gsrc, W, H, p.flags, aux);
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < p.iterations; ++i) {
    float *rgb = (i == p.iterations - 1) ? out : nullptr;
    hipLaunchKernelGGL(qa::qa_denoise_guided_iterate, grid, block, 0, s, plane[i & 1], guide, aux, W, H, 1 << i, p.sigma_color, p.sigma_depth, p.sigma_normal,
                       plane[(i + 1) & 1], rgb);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(c->lastDenoise.Record(s));
  return QA_OK;
}

extern "C" {

int qa_denoise_guided_params_default(qa_denoise_guided_params *p)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->iterations = QA_DENOISE_DEFAULT_ITERATIONS;
  p->sigma_color = QA_DENOISE_DEFAULT_SIGMA_COLOR;
  p->sigma_depth = QA_DENOISE_DEFAULT_SIGMA_DEPTH;
  p->sigma_normal = QA_DENOISE_DEFAULT_SIGMA_NORMAL;
  p->flags = QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO;
  return QA_OK;
}

int qa_denoise_guided_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, const float *d_normal, const float *d_albedo,
                             int width, int height, const qa_denoise_guided_params *p, float *d_out_rgb, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (!d_rgb || !d_depth || !d_ns || !d_out_rgb) return Fail(QA_EINVAL, "null buffer");
  if (int rc = CheckGuidedParams(p, width, height, d_normal, d_albedo, true)) return rc;
  const qa_denoise_params u = {p->iterations, p->sigma_color, p->sigma_depth, 0u};
  if (p->flags == 0u || p->iterations == 0) return qa_denoise_device(c, d_rgb, d_depth, d_ns, width, height, &u, d_out_rgb, hip_stream);
  const DenoiseSrc src = {d_rgb, d_depth, d_ns, nullptr, width};
  return DenoiseGuided(c, src, d_normal, d_albedo, false, width, height, *p, d_out_rgb, StreamOf(c, hip_stream), hip_stream);
}

int qa_progressive_denoise_guided_device(qa_ctx *c, const qa_denoise_guided_params *p, float *d_rgb, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!d_rgb) return Fail(QA_EINVAL, "null buffer");
  const qa_ctx::Progressive &f = c->prog;
  const int W = f.args.x1 - f.args.x0, H = f.args.y1 - f.args.y0;
  if ((rc = CheckGuidedParams(p, W, H, nullptr, nullptr, false)) != QA_OK) return rc;
  const qa_denoise_params u = {p->iterations, p->sigma_color, p->sigma_depth, 0u};
  if (p->flags == 0u || p->iterations == 0) return qa_progressive_denoise_device(c, &u, d_rgb, hip_stream);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(f.done.WaitOn(s));
  const DenoiseSrc src = {f.args.rgb, f.args.depth, f.args.ns, f.dState, W};
  return DenoiseGuided(c, src, nullptr, nullptr, true, W, H, *p, d_rgb, s, hip_stream);
}

int qa_progressive_denoise_guided(qa_ctx *c, const qa_denoise_guided_params *p, float *rgb)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!rgb) return Fail(QA_EINVAL, "null buffer");
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.prevRgb.Reserve(f.npix * 3 * sizeof(float)));
  if ((rc = qa_progressive_denoise_guided_device(c, p, (float *) f.prevRgb.p, nullptr)) != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, f.prevRgb.p, f.npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

// the guided form on the CPU, pixel after pixel (no GPU, no context); normal / albedo null where the flag is clear
int qa_test_denoise_guided_host(const float *rgb, const float *depth, const uint32_t *ns, const float *normal, const float *albedo, int width, int height,
                                const qa_denoise_guided_params *p, float *out_rgb)
{
  if (!rgb || !depth || !ns || !out_rgb) return Fail(QA_EINVAL, "null buffer");
  if (int rc = CheckGuidedParams(p, width, height, normal, albedo, true)) return rc;
  return DenoiseOnHost(rgb, depth, ns, normal, albedo, nullptr, 1.f, width, height, *p, out_rgb);
}

// ---- the variance form: pass 0 takes the caller's variance plane; everything after it is the form that the guide flags select

static int CheckVarianceParams(const qa_denoise_variance_params *p, int width, int height, const void *normal, const void *albedo, const void *variance,
                               qa_denoise_guided_params *guided)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  if (p->flags & ~(QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO | QA_DENOISE_GUIDE_VARIANCE)) return Fail(QA_EINVAL, "unknown flags");
  *guided = {p->iterations, p->sigma_color, p->sigma_depth, p->sigma_normal, p->flags & (QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO)};
  if (int rc = CheckGuidedParams(guided, width, height, normal, albedo, true)) return rc;
  if (!std::isfinite(p->variance_scale) || !(p->variance_scale > 0.f)) return Fail(QA_EINVAL, "a variance_scale that is not finite and positive");
  if ((variance != nullptr) != ((p->flags & QA_DENOISE_GUIDE_VARIANCE) != 0u)) return Fail(QA_EINVAL, "a variance plane that disagrees with its flag");
  return QA_OK;
}

int qa_denoise_variance_params_default(qa_denoise_variance_params *p)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->iterations = QA_DENOISE_DEFAULT_ITERATIONS;
  p->sigma_color = QA_DENOISE_DEFAULT_SIGMA_COLOR;
  p->sigma_depth = QA_DENOISE_DEFAULT_SIGMA_DEPTH;
  p->sigma_normal = QA_DENOISE_DEFAULT_SIGMA_NORMAL;
  p->variance_scale = QA_DENOISE_DEFAULT_VARIANCE_SCALE;
  p->flags = QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO | QA_DENOISE_GUIDE_VARIANCE;
  return QA_OK;
}

int qa_denoise_variance_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, const float *d_normal, const float *d_albedo,
                               const float *d_variance, int width, int height, const qa_denoise_variance_params *p, float *d_out_rgb, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (!d_rgb || !d_depth || !d_ns || !d_out_rgb) return Fail(QA_EINVAL, "null buffer");
  qa_denoise_guided_params g;
  if (int rc = CheckVarianceParams(p, width, height, d_normal, d_albedo, d_variance, &g)) return rc;
  if (!d_variance || p->iterations == 0) return qa_denoise_guided_device(c, d_rgb, d_depth, d_ns, d_normal, d_albedo, width, height, &g, d_out_rgb, hip_stream);
  const DenoiseSrc src = {d_rgb, d_depth, d_ns, nullptr, width};
  if (g.flags == 0u) {
    const qa_denoise_params u = {p->iterations, p->sigma_color, p->sigma_depth, 0u};
    return Denoise(c, src, width, height, u, d_out_rgb, StreamOf(c, hip_stream), d_variance, p->variance_scale);
  }
  return DenoiseGuided(c, src, d_normal, d_albedo, false, width, height, g, d_out_rgb, StreamOf(c, hip_stream), hip_stream, d_variance, p->variance_scale);
}

// the variance form on the CPU, pixel after pixel (no GPU, no context); a plane is null where its flag is clear
int qa_test_denoise_variance_host(const float *rgb, const float *depth, const uint32_t *ns, const float *normal, const float *albedo, const float *variance,
                                  int width, int height, const qa_denoise_variance_params *p, float *out_rgb)
{
  if (!rgb || !depth || !ns || !out_rgb) return Fail(QA_EINVAL, "null buffer");
  qa_denoise_guided_params g;
  if (int rc = CheckVarianceParams(p, width, height, normal, albedo, variance, &g)) return rc;
  return DenoiseOnHost(rgb, depth, ns, normal, albedo, variance, p->variance_scale, width, height, g, out_rgb);
}

}  // extern "C"
