// qa_denoise.hip — the edge-avoiding a-trous filter of qa_denoise_dev.h on the device (qa_denoise_device, qa_progressive_denoise*,
// the guided form qa_denoise_guided_*, the variance form qa_denoise_variance_device) and the same source on the host
// (qa_test_denoise_host, qa_test_denoise_guided_host, qa_test_denoise_variance_host).  Every entry fills one DenoiseCall through
// CheckDenoise and hands it to LaunchDenoise (DenoiseOnHost for the host forms).  The kernels:
//   qa_denoise_pass0<VARIANCE>       pass 0: fills the context's working planes - colour and variance (16 bytes per pixel, two of them:
//                                    the iterations go from one to the other), depth and slope (8 bytes) - from plain buffers or from
//                                    the progressive frame's slabs; <true> reads the caller's variance plane as well
//   qa_denoise_guided_aux            the guided form's aux plane (normal, albedo, valid / reliable bits: 32 bytes per pixel)
//   qa_denoise_iterate_lds<1>, <2>   one iteration at step 1 / 2 of the forms without guides
//   qa_denoise_iterate_direct<GUIDED> one iteration at any step: <false> from step 4 on, <true> every iteration of the guided form
// The last iteration writes the caller's rgb.
//
// Per pixel and iteration 16 + 8 bytes are read and 16 written once (12 by the last): 40 bytes of algorithmic traffic; the 24 other
// taps are re-reads of neighbours' entries.  Steps 1 and 2 stage a 16x16 tile and its halo of 2s (20x20 / 24x24 entries, 9.4 / 13.5 KB)
// in LDS, where the tile's taps overlap almost wholly; from step 4 on a lane's taps are 4+ pixels apart, the halo would be 32x32
// entries and more for 256 pixels, and the taps are loaded directly (16 + 8 bytes each; neighbouring lanes share the lines).  The
// guided iterations load every tap directly (a tap reads 16 + 8 bytes and, where the centre is reliable, 32 more).
// tools/gpu_denoise_cost.py puts the traffic beside the measured times.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "qa_ctx.h"
#include "qa_denoise_dev.h"

namespace qa {

static_assert(sizeof(DenoiseColor) == 16 && sizeof(DenoiseGuide) == 8, "the planes are read with 16- and 8-byte loads");
static_assert(sizeof(DenoiseAux) == 32, "the aux plane is read with two 16-byte loads");
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
// the caller's variance plane (4 more bytes per window pixel of pass 0) and the guide planes; a guide that is not given is null
struct DenoiseVarianceSrc {
  const float *variance;
  int W;
  __host__ __device__ __forceinline__ float operator()(int x, int y) const { return variance[(size_t) y * (size_t) W + (size_t) x]; }
};
struct DenoiseGuideSrc {
  const float *normal, *albedo;
  int W;
  __host__ __device__ __forceinline__ void operator()(int x, int y, float *n, float *a) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    if (normal) { n[0] = normal[3 * q]; n[1] = normal[3 * q + 1]; n[2] = normal[3 * q + 2]; }
    if (albedo) { a[0] = albedo[3 * q]; a[1] = albedo[3 * q + 1]; a[2] = albedo[3 * q + 2]; }
  }
};

// the planes in global memory / a window of them in LDS whose entry (0, 0) is pixel (ox, oy)
struct DenoiseTapGlobal {
  const DenoiseColor *color;
  const DenoiseGuide *guide;
  int W;
  __host__ __device__ __forceinline__ void operator()(int x, int y, DenoiseColor &c, DenoiseGuide &g) const
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
struct DenoiseAuxGlobal {
  const DenoiseAux *aux;
  int W;
  __host__ __device__ __forceinline__ DenoiseAux operator()(int x, int y) const { return aux[(size_t) y * (size_t) W + (size_t) x]; }
};

// Pass 0.  VARIANCE: the variance form's, with the caller's plane (vsrc and varianceScale are not read otherwise)
template <bool VARIANCE>
__global__ __launch_bounds__(256) void qa_denoise_pass0(DenoiseSrc src, DenoiseVarianceSrc vsrc, float varianceScale, int W, int H, DenoiseColor *color,
                                                        DenoiseGuide *guide)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  DenoiseColor c;
  DenoiseGuide g;
  if constexpr (VARIANCE) denoiseGuideVariance(src, vsrc, varianceScale, x, y, W, H, c, g);
  else denoiseGuide(src, x, y, W, H, c, g);
  const size_t q = (size_t) y * (size_t) W + (size_t) x;
  color[q] = c;
  guide[q] = g;
}

__global__ __launch_bounds__(256) void qa_denoise_guided_aux(DenoiseSrc src, DenoiseGuideSrc gsrc, int W, int H, uint32_t flags, DenoiseAux *aux)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  aux[(size_t) y * (size_t) W + (size_t) x] = denoiseAux(src, gsrc, x, y, W, H, flags);
}

__device__ __forceinline__ void denoiseStore(const DenoiseColor &o, size_t q, DenoiseColor *outColor, float *outRgb)
{
  if (outRgb) { outRgb[3 * q] = o.r; outRgb[3 * q + 1] = o.g; outRgb[3 * q + 2] = o.b; }
  else outColor[q] = o;
}

// One iteration without guides at step S = 1 or 2 over a 16x16 tile staged with its halo of 2 S.  Entries outside the image are not
// loaded and never read (denoiseIterate skips those taps).  outRgb != null: the last iteration, which writes the caller's frame
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
  denoiseStore(denoiseIterate<false>(tap, DenoiseNoAux{}, x, y, W, H, S, sigmaColor, sigmaDepth, 0.f), (size_t) y * (size_t) W + (size_t) x, outColor, outRgb);
}

// One iteration at any step, the taps loaded directly.  GUIDED: with the aux plane (aux and sigmaNormal are not read otherwise)
template <bool GUIDED>
__global__ __launch_bounds__(256) void qa_denoise_iterate_direct(const DenoiseColor *color, const DenoiseGuide *guide, const DenoiseAux *aux, int W, int H,
                                                                 int s, float sigmaColor, float sigmaDepth, float sigmaNormal, DenoiseColor *outColor,
                                                                 float *outRgb)
{
  const int x = (int) (blockIdx.x * QA_DENOISE_TILE + (threadIdx.x & 15u)), y = (int) (blockIdx.y * QA_DENOISE_TILE + (threadIdx.x >> 4));
  if (x >= W || y >= H) return;
  const DenoiseTapGlobal tap = {color, guide, W};
  const DenoiseAuxGlobal at = {aux, W};
  denoiseStore(denoiseIterate<GUIDED>(tap, at, x, y, W, H, s, sigmaColor, sigmaDepth, sigmaNormal), (size_t) y * (size_t) W + (size_t) x, outColor, outRgb);
}

}  // namespace qa

// Everything a call needs, whichever entry it came through.  The entry fills the planes, the size and out; CheckDenoise the rest
struct DenoiseCall {
  DenoiseSrc src;
  const float *normal, *albedo, *variance;   // null where the flag is clear
  int W, H;
  float *out;
  bool ownGuides;   // a progressive frame: the guide planes are the context's own, computed by the launch
  int iterations;
  float sigmaColor, sigmaDepth, sigmaNormal, varianceScale;
  uint32_t flags;   // QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO: the guided form where one is set
};

// The refusals of every entry, in one order, and k's parameters from p: any of the three parameter structs, whose type says which
// flags the form knows (a parameter that a struct does not have is never read by the forms it can select)
template <class P>
static int CheckDenoise(DenoiseCall &k, const P *p)
{
  constexpr bool HAS_NORMAL = !std::is_same_v<P, qa_denoise_params>, HAS_VARIANCE = std::is_same_v<P, qa_denoise_variance_params>;
  constexpr uint32_t GUIDES = QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO;
  constexpr uint32_t KNOWN = HAS_VARIANCE ? (GUIDES | QA_DENOISE_GUIDE_VARIANCE) : HAS_NORMAL ? GUIDES : 0u;
  const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
  if (!k.src.rgb || !k.src.depth || !k.src.ns || !k.out) return Fail(QA_EINVAL, "null buffer");
  if (!p) return Fail(QA_EINVAL, "null parameters");
  if (p->flags & ~KNOWN) return Fail(QA_EINVAL, "unknown flags");
  if (k.W < 1 || k.H < 1) return Fail(QA_EINVAL, "bad frame size");
  if ((uint64_t) k.W * (uint64_t) k.H > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");
  if (p->iterations < 0 || p->iterations > QA_DENOISE_MAX_ITERATIONS) return Fail(QA_EINVAL, "iterations outside 0 .. 6");
  if (!positive(p->sigma_color) || !positive(p->sigma_depth)) return Fail(QA_EINVAL, "a sigma that is not finite and positive");
  k.iterations = p->iterations; k.sigmaColor = p->sigma_color; k.sigmaDepth = p->sigma_depth;
  k.sigmaNormal = QA_DENOISE_DEFAULT_SIGMA_NORMAL; k.varianceScale = 1.f;
  k.flags = p->flags & GUIDES;
  if constexpr (HAS_NORMAL) {
    if (!positive(p->sigma_normal)) return Fail(QA_EINVAL, "a sigma that is not finite and positive");
    k.sigmaNormal = p->sigma_normal;
  }
  if constexpr (HAS_VARIANCE) {
    if (!positive(p->variance_scale)) return Fail(QA_EINVAL, "a variance_scale that is not finite and positive");
    k.varianceScale = p->variance_scale;
  }
  if (!k.ownGuides && ((k.normal != nullptr) != ((p->flags & QA_DENOISE_GUIDE_NORMAL) != 0u) || (k.albedo != nullptr) != ((p->flags & QA_DENOISE_GUIDE_ALBEDO) != 0u)))
    return Fail(QA_EINVAL, "a guide plane that disagrees with its flag");
  if ((k.variance != nullptr) != ((p->flags & QA_DENOISE_GUIDE_VARIANCE) != 0u)) return Fail(QA_EINVAL, "a variance plane that disagrees with its flag");
  return QA_OK;
}

// Pass 0 and the iterations of a checked call on s.  The working planes are one per context and only grow: [colour A | colour B |
// guide], 40 bytes per pixel; the guided form adds [aux], 32 bytes, and [own normal | own albedo], 24 more, when the guide planes are
// the context's own (a progressive frame's, computed here).  Every entry is written before it is read; a call on another stream than
// the last one waits for it
static int LaunchDenoise(qa_ctx *c, const DenoiseCall &k, hipStream_t s, void *hip_stream)
{
  const int W = k.W, H = k.H;
  const size_t n = (size_t) W * (size_t) H;
  if (k.iterations == 0) {   // the input's bits (a progressive frame still has to be resolved: its callers never get here)
    if (k.out != k.src.rgb) HIP_TRY(hipMemcpyAsync(k.out, k.src.rgb, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return QA_OK;
  }
  const bool guided = k.flags != 0u;
  HIP_TRY(c->denoisePlanes.Reserve(n * (!guided ? 40 : k.ownGuides ? 96 : 72), true));   // (the old planes may be in use on a stream of the caller's)
  HIP_TRY(c->lastDenoise.WaitOn(s));
  DenoiseColor *plane[2] = {static_cast<DenoiseColor *>(c->denoisePlanes.p), static_cast<DenoiseColor *>(c->denoisePlanes.p) + n};
  DenoiseGuide *guide = reinterpret_cast<DenoiseGuide *>(plane[1] + n);
  DenoiseAux *aux = reinterpret_cast<DenoiseAux *>(guide + n);   // (past the planes' end, and not used, without guides)
  const float *normal = k.normal, *albedo = k.albedo;
  if (guided && k.ownGuides) {
    float *own = reinterpret_cast<float *>(aux + n);
    float *dN = (k.flags & QA_DENOISE_GUIDE_NORMAL) ? own : nullptr, *dA = (k.flags & QA_DENOISE_GUIDE_ALBEDO) ? own + 3 * n : nullptr;
    if (int rc = qa_progressive_gbuffer_device(c, dN, dA, nullptr, nullptr, hip_stream)) return rc;
    normal = dN; albedo = dA;
  }
  const dim3 grid((unsigned) ((W + QA_DENOISE_TILE - 1) / QA_DENOISE_TILE), (unsigned) ((H + QA_DENOISE_TILE - 1) / QA_DENOISE_TILE)), block(256);
  const DenoiseVarianceSrc vsrc = {k.variance, W};
  if (k.variance) hipLaunchKernelGGL(qa::qa_denoise_pass0<true>, grid, block, 0, s, k.src, vsrc, k.varianceScale, W, H, plane[0], guide);
  else hipLaunchKernelGGL(qa::qa_denoise_pass0<false>, grid, block, 0, s, k.src, vsrc, k.varianceScale, W, H, plane[0], guide);
  HIP_TRY(hipGetLastError());
  if (guided) {
    const DenoiseGuideSrc gsrc = {normal, albedo, W};
    hipLaunchKernelGGL(qa::qa_denoise_guided_aux, grid, block, 0, s, k.src, gsrc, W, H, k.flags, aux);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < k.iterations; ++i) {
    const DenoiseColor *from = plane[i & 1];
    DenoiseColor *to = plane[(i + 1) & 1];
    float *rgb = (i == k.iterations - 1) ? k.out : nullptr;
    if (guided)
      hipLaunchKernelGGL(qa::qa_denoise_iterate_direct<true>, grid, block, 0, s, from, guide, aux, W, H, 1 << i, k.sigmaColor, k.sigmaDepth, k.sigmaNormal, to, rgb);
    else if (i == 0) hipLaunchKernelGGL(qa::qa_denoise_iterate_lds<1>, grid, block, 0, s, from, guide, W, H, k.sigmaColor, k.sigmaDepth, to, rgb);
    else if (i == 1) hipLaunchKernelGGL(qa::qa_denoise_iterate_lds<2>, grid, block, 0, s, from, guide, W, H, k.sigmaColor, k.sigmaDepth, to, rgb);
    else
      hipLaunchKernelGGL(qa::qa_denoise_iterate_direct<false>, grid, block, 0, s, from, guide, nullptr, W, H, 1 << i, k.sigmaColor, k.sigmaDepth, 0.f, to, rgb);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(c->lastDenoise.Record(s));
  return QA_OK;
}

// A call on plain device buffers: qa_denoise_device and its guided and variance forms
template <class P>
static int DenoiseDevice(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, const float *d_normal, const float *d_albedo,
                         const float *d_variance, int width, int height, const P *p, float *d_out_rgb, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  DenoiseCall k = {{d_rgb, d_depth, d_ns, nullptr, width}, d_normal, d_albedo, d_variance, width, height, d_out_rgb, false};
  if (int rc = CheckDenoise(k, p)) return rc;
  return LaunchDenoise(c, k, StreamOf(c, hip_stream), hip_stream);
}

// A call on the progressive frame, after ProgActive: filtered straight from its slabs into d_rgb, guided by its own first-hit planes
template <class P>
static int DenoiseProgressive(qa_ctx *c, const P *p, float *d_rgb, void *hip_stream)
{
  qa_ctx::Progressive &f = c->prog;
  const int W = f.args.x1 - f.args.x0, H = f.args.y1 - f.args.y0;
  DenoiseCall k = {{f.args.rgb, f.args.depth, f.args.ns, f.dState, W}, nullptr, nullptr, nullptr, W, H, d_rgb, true};
  if (int rc = CheckDenoise(k, p)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(f.done.WaitOn(s));
  if (k.iterations == 0) {   // the preview itself; depth and sample counts go to the frame's preview buffers
    HIP_TRY(f.prevDepth.Reserve(f.npix * sizeof(float)));
    HIP_TRY(f.prevNs.Reserve(f.npix * sizeof(uint32_t)));
    return qa_progressive_read_device(c, d_rgb, (float *) f.prevDepth.p, (uint32_t *) f.prevNs.p, hip_stream);
  }
  return LaunchDenoise(c, k, s, hip_stream);
}

// The same into host memory, through the preview's buffer (the frame's size is fixed: it never grows); synchronises
template <class P>
static int DenoiseProgressiveToHost(qa_ctx *c, const P *p, float *rgb)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!rgb) return Fail(QA_EINVAL, "null buffer");
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  HIP_TRY(f.prevRgb.Reserve(f.npix * 3 * sizeof(float)));
  if ((rc = DenoiseProgressive(c, p, (float *) f.prevRgb.p, nullptr)) != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, f.prevRgb.p, f.npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

// Every form on the CPU, pixel after pixel (no GPU, no context), after the checks: pass 0 (the variance form's with a variance plane),
// the aux plane when a guide is named, and the iterations of the form that the guide flags select
template <class P>
static int DenoiseOnHost(const float *rgb, const float *depth, const uint32_t *ns, const float *normal, const float *albedo, const float *variance, int W,
                         int H, const P *p, float *out_rgb)
{
  DenoiseCall k = {{rgb, depth, ns, nullptr, W}, normal, albedo, variance, W, H, out_rgb, false};
  if (int rc = CheckDenoise(k, p)) return rc;
  const size_t n = (size_t) W * (size_t) H;
  if (k.iterations == 0) {
    if (out_rgb != rgb) memcpy(out_rgb, rgb, n * 3 * sizeof(float));
    return QA_OK;
  }
  const bool guided = k.flags != 0u;
  std::vector<DenoiseColor> plane[2] = {std::vector<DenoiseColor>(n), std::vector<DenoiseColor>(n)};
  std::vector<DenoiseGuide> guide(n);
  std::vector<DenoiseAux> aux(guided ? n : 0);
  const auto src = [=](int x, int y) {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    DenoisePixel px;
    px.r = rgb[3 * q]; px.g = rgb[3 * q + 1]; px.b = rgb[3 * q + 2]; px.z = depth[q]; px.ns = ns[q];
    return px;
  };
  const DenoiseGuideSrc gsrc = {normal, albedo, W};
  const DenoiseVarianceSrc vsrc = {variance, W};
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t q = (size_t) y * W + x;
      if (variance) denoiseGuideVariance(src, vsrc, k.varianceScale, x, y, W, H, plane[0][q], guide[q]);
      else denoiseGuide(src, x, y, W, H, plane[0][q], guide[q]);
      if (guided) aux[q] = denoiseAux(src, gsrc, x, y, W, H, k.flags);
    }
  for (int i = 0; i < k.iterations; ++i) {
    const DenoiseTapGlobal tap = {plane[i & 1].data(), guide.data(), W};
    const DenoiseAuxGlobal at = {aux.data(), W};
    std::vector<DenoiseColor> &to = plane[(i + 1) & 1];
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        to[(size_t) y * W + x] = guided ? denoiseIterate<true>(tap, at, x, y, W, H, 1 << i, k.sigmaColor, k.sigmaDepth, k.sigmaNormal)
                                        : denoiseIterate<false>(tap, DenoiseNoAux{}, x, y, W, H, 1 << i, k.sigmaColor, k.sigmaDepth, 0.f);
  }
  const std::vector<DenoiseColor> &last = plane[k.iterations & 1];
  for (size_t q = 0; q < n; ++q) { out_rgb[3 * q] = last[q].r; out_rgb[3 * q + 1] = last[q].g; out_rgb[3 * q + 2] = last[q].b; }
  return QA_OK;
}

// The defaults of the three parameter structs: every flag the form knows, and the parameters it has
template <class P>
static int DenoiseDefaults(P *p, uint32_t flags)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->iterations = QA_DENOISE_DEFAULT_ITERATIONS;
  p->sigma_color = QA_DENOISE_DEFAULT_SIGMA_COLOR;
  p->sigma_depth = QA_DENOISE_DEFAULT_SIGMA_DEPTH;
  if constexpr (!std::is_same_v<P, qa_denoise_params>) p->sigma_normal = QA_DENOISE_DEFAULT_SIGMA_NORMAL;
  if constexpr (std::is_same_v<P, qa_denoise_variance_params>) p->variance_scale = QA_DENOISE_DEFAULT_VARIANCE_SCALE;
  p->flags = flags;
  return QA_OK;
}

extern "C" {

int qa_denoise_params_default(qa_denoise_params *p) { return DenoiseDefaults(p, 0u); }
int qa_denoise_guided_params_default(qa_denoise_guided_params *p) { return DenoiseDefaults(p, QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO); }
int qa_denoise_variance_params_default(qa_denoise_variance_params *p)
{
  return DenoiseDefaults(p, QA_DENOISE_GUIDE_NORMAL | QA_DENOISE_GUIDE_ALBEDO | QA_DENOISE_GUIDE_VARIANCE);
}

int qa_denoise_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, int width, int height, const qa_denoise_params *p,
                      float *d_out_rgb, void *hip_stream)
{
  return DenoiseDevice(c, d_rgb, d_depth, d_ns, nullptr, nullptr, nullptr, width, height, p, d_out_rgb, hip_stream);
}

int qa_denoise_guided_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, const float *d_normal, const float *d_albedo,
                             int width, int height, const qa_denoise_guided_params *p, float *d_out_rgb, void *hip_stream)
{
  return DenoiseDevice(c, d_rgb, d_depth, d_ns, d_normal, d_albedo, nullptr, width, height, p, d_out_rgb, hip_stream);
}

int qa_denoise_variance_device(qa_ctx *c, const float *d_rgb, const float *d_depth, const uint32_t *d_ns, const float *d_normal, const float *d_albedo,
                               const float *d_variance, int width, int height, const qa_denoise_variance_params *p, float *d_out_rgb, void *hip_stream)
{
  return DenoiseDevice(c, d_rgb, d_depth, d_ns, d_normal, d_albedo, d_variance, width, height, p, d_out_rgb, hip_stream);
}

int qa_progressive_denoise_device(qa_ctx *c, const qa_denoise_params *p, float *d_rgb, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  return DenoiseProgressive(c, p, d_rgb, hip_stream);
}

int qa_progressive_denoise_guided_device(qa_ctx *c, const qa_denoise_guided_params *p, float *d_rgb, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  return DenoiseProgressive(c, p, d_rgb, hip_stream);
}

int qa_progressive_denoise(qa_ctx *c, const qa_denoise_params *p, float *rgb) { return DenoiseProgressiveToHost(c, p, rgb); }
int qa_progressive_denoise_guided(qa_ctx *c, const qa_denoise_guided_params *p, float *rgb) { return DenoiseProgressiveToHost(c, p, rgb); }

// a plane is null where its flag is clear
int qa_test_denoise_host(const float *rgb, const float *depth, const uint32_t *ns, int width, int height, const qa_denoise_params *p, float *out_rgb)
{
  return DenoiseOnHost(rgb, depth, ns, nullptr, nullptr, nullptr, width, height, p, out_rgb);
}

int qa_test_denoise_guided_host(const float *rgb, const float *depth, const uint32_t *ns, const float *normal, const float *albedo, int width, int height,
                                const qa_denoise_guided_params *p, float *out_rgb)
{
  return DenoiseOnHost(rgb, depth, ns, normal, albedo, nullptr, width, height, p, out_rgb);
}

int qa_test_denoise_variance_host(const float *rgb, const float *depth, const uint32_t *ns, const float *normal, const float *albedo, const float *variance,
                                  int width, int height, const qa_denoise_variance_params *p, float *out_rgb)
{
  return DenoiseOnHost(rgb, depth, ns, normal, albedo, variance, width, height, p, out_rgb);
}

}  // extern "C"
