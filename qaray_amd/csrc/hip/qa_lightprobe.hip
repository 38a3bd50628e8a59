// qa_lightprobe.hip — light probes (qa_probe_*): what a camera at a point in free space would see in every direction of a cube map,
// traced by qa_radiance_rays_device, projected onto the spherical harmonics of order 2 on the device, and the per-shading-point
// evaluation a viewer calls every frame.  The opening comment of qa_lightprobe_dev.h is the specification of all arithmetic; this
// unit holds the kernels around it, the entries of the C ABI and the host hooks that run the same source on the CPU.
//
// No integrator is compiled here: the rays of a chunk of probes are written into a scratch buffer of the context's (origins,
// directions, stream ids, rgb, t: 44 bytes per ray, only grows), handed to qa_radiance_rays_device - its checks, its ordering behind
// frames and edits, its counters - and reduced, one wave per probe, before the next chunk is written; all on the call's stream.
// The scratch is one per context: a call waits for lastFrame before it writes it and records lastFrame behind its last reduction,
// so that a probe call on another stream, which waits for that fence as every batch does, finds it free.
//
// What a probe holds: emitters, the environment, and the surfaces around it under their own direct and bounced light.  It does not
// hold the direct term of point, spot and directional lights at P itself - no ray can meet them; a shader adds them analytically.
//
// Visibility (qa_probevis_*, specified in qa_probevis_dev.h): the same batch with one more kernel per chunk, which pools the chunk's t
// from the scratch into two distance moments per direction cell, and a grid shading that weighs the probes of a cell by them.
#include "qa_lightprobe_dev.h"
#include "qa_probevis_dev.h"
#include "qa_raybatch.h"
#include "qa_stage.h"

namespace qa {

struct ProbeGen {
  const float *points;      // [n][3], the chunk's first probe at [first]
  const uint32_t *stream;   // [n] or null
  uint64_t first, count;    // the chunk's probes
  uint32_t m, K, seed, jitter;
  float *o, *d;             // [count * K][3]
  uint32_t *ray_stream;     // [count * K]
};

// One thread per ray of the chunk
__global__ __launch_bounds__(256) void qa_probe_rays(const ProbeGen g)
{
  const uint64_t r = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (r >= g.count * g.K) return;
  const uint64_t q = g.first + r / g.K;
  const uint32_t k = (uint32_t) (r % g.K);
  const uint32_t S = g.stream ? g.stream[q] : (uint32_t) q;
  const ProbeDir pd = probeRecord(g.m, g.seed, S, k, g.jitter != 0);
  for (int e = 0; e < 3; ++e) {
    g.o[3 * r + e] = g.points[3 * q + e];
    g.d[3 * r + e] = pd.d[e];
  }
  g.ray_stream[r] = probeRayStream(S, g.K, k);
}

struct ProbeReduce {
  const float *points;
  const uint32_t *stream;
  uint64_t first, count;
  uint32_t m, K, seed, jitter;
  const float *rgb, *t;     // the chunk's rays
  float *cube;              // the chunk's part of the cube output when rgb is that, else null
  float *sh;                // outputs of the whole batch, indexed by probe
  uint32_t *hits;
  float *tmin;
};

// One wave per probe, four probes per workgroup
__global__ __launch_bounds__(256) void qa_probe_project(const ProbeReduce g)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t local = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (local >= g.count) return;
  const uint64_t q = g.first + local;
  if (probeVoid(g.points[3 * q], g.points[3 * q + 1], g.points[3 * q + 2])) {
    if (g.sh && lane < 27) g.sh[27 * q + lane] = 0.f;
    if (lane == 0) {
      if (g.hits) g.hits[q] = 0u;
      if (g.tmin) g.tmin[q] = QA_AO_MAX_T;
    }
    if (g.cube)
      for (uint64_t i = lane; i < 3ull * g.K; i += 64) g.cube[local * 3 * g.K + i] = 0.f;
    return;
  }
  const uint32_t S = g.stream ? g.stream[q] : (uint32_t) q;
  ProbeAcc acc;
  probeAccInit(acc);
  for (uint32_t k = lane; k < g.K; k += QA_PROBE_LANES) {
    const ProbeDir pd = probeRecord(g.m, g.seed, S, k, g.jitter != 0);
    const uint64_t r = local * g.K + k;
    const float rgb[3] = {g.rgb[3 * r], g.rgb[3 * r + 1], g.rgb[3 * r + 2]};
    probeAccAdd(acc, pd.d, pd.w, rgb, g.t[r]);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    ProbeAcc other;
    for (int i = 0; i < 28; ++i) other.a[i] = __shfl_xor(acc.a[i], off, 64);
    other.hits = (uint32_t) __shfl_xor((int) acc.hits, off, 64);
    other.tmin = __shfl_xor(acc.tmin, off, 64);
    probeAccFold(acc, other);
  }
  float sh[27];
  probeAccFinish(acc, sh);
  // (every lane holds the same 27 values: lane i writes the i-th, picked by a chain of selects - a branch per lane here became a
  // switch tree of a dozen masked stores)
  float mine = sh[0];
  for (int i = 1; i < 27; ++i) mine = (lane == (uint32_t) i) ? sh[i] : mine;
  if (g.sh && lane < 27) g.sh[27 * q + lane] = mine;
  if (lane == 0) {
    if (g.hits) g.hits[q] = acc.hits;
    if (g.tmin) g.tmin[q] = acc.tmin;
  }
}

// One thread per shading point
__global__ __launch_bounds__(256) void qa_probe_shade(uint64_t n, const float *sh, int64_t probes, const float *normals, const int32_t *index, float *rgb)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t q = probeIndex(index ? (int64_t) index[i] : (int64_t) i, probes);
  float out[3];
  probeShade(sh + 27 * q, normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], out);
  rgb[3 * i] = out[0]; rgb[3 * i + 1] = out[1]; rgb[3 * i + 2] = out[2];
}

__global__ __launch_bounds__(256) void qa_probe_grid_shade(uint64_t n, const ProbeGrid grid, const float *sh, const float *points, const float *normals, float *rgb)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float P[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]}, N[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  float out[3];
  probeGridShade(grid, sh, P, N, out);
  rgb[3 * i] = out[0]; rgb[3 * i + 1] = out[1]; rgb[3 * i + 2] = out[2];
}

// ---- visibility (qa_probevis_*; the opening comment of qa_probevis_dev.h is the specification)

struct ProbeVisPool {
  const float *points;
  uint64_t first, count;    // the chunk's probes
  uint32_t m, K, d;
  float dmax;
  const float *t;           // the chunk's rays
  float *moments;           // output of the whole batch [n][6][d][d][2]
};

// One thread per cell of the chunk's probes: the chunk's t is read before the next chunk's rays overwrite it
__global__ __launch_bounds__(256) void qa_probevis_moments(const ProbeVisPool g)
{
  const uint32_t cells = 6u * g.d * g.d;
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= g.count * cells) return;
  const uint64_t local = i / cells, q = g.first + local;
  const uint32_t cell = (uint32_t) (i % cells);
  float out[2] = {0.f, 0.f};
  if (!probeVoid(g.points[3 * q], g.points[3 * q + 1], g.points[3 * q + 2])) probeVisMoments(g.m, g.d, g.dmax, g.t + local * g.K, cell, out);
  g.moments[2 * (q * cells + cell)] = out[0];
  g.moments[2 * (q * cells + cell) + 1] = out[1];
}

// One thread per shading point
__global__ __launch_bounds__(256) void qa_probevis_grid_shade(uint64_t n, const ProbeGrid grid, const float *sh, const float *moments, int d, float normal_bias,
                                                              const float *points, const float *normals, float *rgb)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float P[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]}, N[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  float out[3];
  probeVisGridShade(grid, sh, moments, d, normal_bias, P, N, out);
  rgb[3 * i] = out[0]; rgb[3 * i + 1] = out[1]; rgb[3 * i + 2] = out[2];
}

}  // namespace qa

#define QA_PROBE_FLAGS (QA_PROBE_JITTER | QA_RADIANCE_PHOTON_MAPS)
#define QA_PROBE_CHUNK_RAYS (1ull << 20)
static_assert(!(QA_PROBE_JITTER & (QA_RADIANCE_PER_SAMPLE | QA_RADIANCE_MISS_ENVIRONMENT | QA_RADIANCE_PHOTON_MAPS)), "the probe's own bit beside the radiance bits");

// the probes a chunk takes
static uint64_t ChunkProbes(const qa_probe_params *p, uint64_t n, uint64_t K)
{
  const uint64_t rays = p->chunk_rays ? p->chunk_rays : QA_PROBE_CHUNK_RAYS;
  return std::min<uint64_t>(n, std::max<uint64_t>(1, rays / K));
}
static qa_radiance_params RadianceOf(const qa_probe_params *p)
{
  return {p->spp, p->max_bounce, p->seed, QA_RADIANCE_MISS_ENVIRONMENT | (p->flags & QA_RADIANCE_PHOTON_MAPS)};
}

// What the device and the host forms refuse alike.  QA_OK with n == 0: nothing to do
static int ProbeChecks(qa_ctx *c, uint64_t n, bool points, const qa_probe_params *p, bool sh)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 probes");
  if (!points) return Fail(QA_EINVAL, "null point array");
  if (!sh) return Fail(QA_EINVAL, "null sh output");
  if (!p) return Fail(QA_EINVAL, "null params");
  if (p->m < 1 || p->m > QA_PROBE_MAX_M) return Fail(QA_EINVAL, "m must be 1 .. 128");
  if (p->flags & ~QA_PROBE_FLAGS) return Fail(QA_EINVAL, "unknown flag bits");
  // the chunks are batches of the radiance query: its rules for their size, spp, max_bounce, area lights and photon maps, its codes
  const uint64_t K = 6ull * p->m * p->m;
  const qa_radiance_params rp = RadianceOf(p);
  return RayBatchChecks(c, ChunkProbes(p, n, K) * K, true, false, false, false, &rp, true, QA_RADIANCE_MISS_ENVIRONMENT | QA_RADIANCE_PHOTON_MAPS, true);
}

// The batch, chunk after chunk on stream s (behind ProbeChecks; every array is the device's)
static int ProbeBatch(qa_ctx *c, uint64_t n, const float *points, const uint32_t *stream, const qa_probe_params *p, float *sh, float *cube,
                      uint32_t *hits, float *tmin, hipStream_t s, const qa_probevis_params *vis = nullptr, float *moments = nullptr)
{
  const uint64_t K = 6ull * p->m * p->m, per = ChunkProbes(p, n, K), rays = per * K;
  const qa_radiance_params rp = RadianceOf(p);
  // the scratch of the largest chunk so far: [origins 3 | dirs 3 | rgb 3 | t 1 | stream 1] floats per ray
  HIP_TRY(c->probeScratch.Reserve((size_t) rays * 11 * sizeof(float), true));
  float *dO = (float *) c->probeScratch.p, *dD = dO + 3 * rays, *dRgb = dD + 3 * rays, *dT = dRgb + 3 * rays;
  uint32_t *dS = (uint32_t *) (dT + rays);
  HIP_TRY(c->lastFrame.WaitOn(s));   // (an earlier probe call on another stream may still read the scratch)
  for (uint64_t first = 0; first < n; first += per) {
    const uint64_t count = std::min(per, n - first), nr = count * K;
    float *rgb = cube ? cube + first * K * 3 : dRgb;
    const ProbeGen gen = {points, stream, first, count, (uint32_t) p->m, (uint32_t) K, p->seed, p->flags & QA_PROBE_JITTER, dO, dD, dS};
    hipLaunchKernelGGL(qa_probe_rays, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, s, gen);
    HIP_TRY(hipGetLastError());
    if (int rc = qa_radiance_rays_device(c, nr, dO, dD, nullptr, nullptr, nullptr, dS, &rp, rgb, dT, nullptr, s)) return rc;
    const ProbeReduce red = {points, stream, first, count, (uint32_t) p->m, (uint32_t) K, p->seed, p->flags & QA_PROBE_JITTER, rgb, dT, cube ? rgb : nullptr, sh, hits, tmin};
    hipLaunchKernelGGL(qa_probe_project, dim3((unsigned) ((count + 3) / 4)), dim3(256), 0, s, red);
    HIP_TRY(hipGetLastError());
    if (moments) {
      const ProbeVisPool pool = {points, first, count, (uint32_t) p->m, (uint32_t) K, (uint32_t) vis->d, vis->dmax, dT, moments};
      hipLaunchKernelGGL(qa_probevis_moments, dim3((unsigned) ((count * 6 * vis->d * vis->d + 255) / 256)), dim3(256), 0, s, pool);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(c->lastFrame.Record(s));
  return QA_OK;
}

// qa_probevis_sh*: what qa_probe_sh* refuses, in its order and with its codes (sh is optional here), then the moments' own rules
static int ProbeVisChecks(qa_ctx *c, uint64_t n, bool points, const qa_probe_params *p, const qa_probevis_params *v, bool moments)
{
  if (int rc = ProbeChecks(c, n, points, p, true)) return rc;
  if (n == 0) return QA_OK;
  if (!v) return Fail(QA_EINVAL, "null visibility params");
  if (!moments) return Fail(QA_EINVAL, "null moments output");
  if (v->d < 1 || v->d > p->m || p->m % v->d) return Fail(QA_EINVAL, "d must be 1 .. m and divide m");
  if (!(v->dmax > 0.f) || !std::isfinite(v->dmax)) return Fail(QA_EINVAL, "dmax must be positive and finite");
  if (!std::isfinite(v->normal_bias)) return Fail(QA_EINVAL, "normal_bias must be finite");
  return QA_OK;
}

// What both host forms do behind their checks (n > 0): stage, run the batch on the context's stream, copy back.  vis and moments are
// null for the plain call
static int ProbeHost(qa_ctx *c, uint64_t n, const float *points, const uint32_t *stream_ids, const qa_probe_params *params, const qa_probevis_params *vis,
                     float *sh, float *cube, uint32_t *hits, float *tmin, float *moments)
{
  const uint64_t K = 6ull * params->m * params->m, cells = vis ? 12ull * vis->d * vis->d : 0;
  QueryStage st(c);
  const auto dP = st.In(points, 3 * n);
  const auto dStream = st.In(stream_ids, n);
  const auto dSh = st.Out(sh, 27 * n), dCube = st.Out(cube, 3 * K * n);
  const auto dHits = st.Out(hits, n);
  const auto dTmin = st.Out(tmin, n), dMoments = st.Out(moments, cells * n);
  if (int rc = st.Begin()) return rc;
  if (int rc = ProbeBatch(c, n, st(dP), st(dStream), params, st(dSh), st(dCube), st(dHits), st(dTmin), c->stream, vis, st(dMoments))) return rc;
  if (int rc = st.End()) return rc;
  return DrainEvents(c);   // the chunks are complete: fold their event pairs into the kernel time
}

extern "C" {

int qa_probe_params_default(qa_probe_params *params)
{
  if (!params) return Fail(QA_EINVAL, "null argument");
  params->m = 16;
  params->spp = 1;
  params->max_bounce = 5;
  params->seed = 0x51A7A7u;
  params->flags = 0;
  params->chunk_rays = 0;
  return QA_OK;
}

int qa_probe_sh_device(qa_ctx *c, uint64_t n, const float *d_points, const uint32_t *d_stream, const qa_probe_params *params, float *d_sh,
                       float *d_cube, uint32_t *d_hits, float *d_tmin, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = ProbeChecks(c, n, d_points != nullptr, params, d_sh != nullptr)) return rc;
  if (n == 0) return QA_OK;
  return ProbeBatch(c, n, d_points, d_stream, params, d_sh, d_cube, d_hits, d_tmin, StreamOf(c, stream), nullptr, nullptr);
}

int qa_probe_sh(qa_ctx *c, uint64_t n, const float *points, const uint32_t *stream_ids, const qa_probe_params *params, float *sh, float *cube,
                uint32_t *hits, float *tmin)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = ProbeChecks(c, n, points != nullptr, params, sh != nullptr)) return rc;
  if (n == 0) return QA_OK;
  return ProbeHost(c, n, points, stream_ids, params, nullptr, sh, cube, hits, tmin, nullptr);
}

int qa_probe_shade_device(qa_ctx *c, uint64_t n, const float *d_sh, uint64_t probes, const float *d_normals, const int32_t *d_index,
                          float *d_rgb, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 shading points");
  if (!d_sh || !d_normals || !d_rgb) return Fail(QA_EINVAL, "null array");
  if (probes < 1 || probes > QA_MAX_RAYS) return Fail(QA_EINVAL, "bad probe count");
  if (!d_index && probes < n) return Fail(QA_EINVAL, "fewer probes than shading points and no index");
  hipLaunchKernelGGL(qa_probe_shade, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, StreamOf(c, stream), n, d_sh, (int64_t) probes, d_normals, d_index, d_rgb);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

int qa_probe_grid_shade_device(qa_ctx *c, uint64_t n, const float *d_sh, const float *origin, const float *spacing, const int32_t *counts,
                               const float *d_points, const float *d_normals, float *d_rgb, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (!GridOk(origin, spacing, counts)) return Fail(QA_EINVAL, "bad grid: finite origin, spacing > 0, counts >= 1, at most 2^31 - 1 probes");
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 shading points");
  if (!d_sh || !d_points || !d_normals || !d_rgb) return Fail(QA_EINVAL, "null array");
  hipLaunchKernelGGL(qa_probe_grid_shade, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, StreamOf(c, stream), n, GridOf(origin, spacing, counts), d_sh,
                     d_points, d_normals, d_rgb);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// ---- visibility: the moments beside the coefficients, and the shading that uses them

int qa_probevis_params_default(qa_probevis_params *params)
{
  if (!params) return Fail(QA_EINVAL, "null argument");
  params->d = 8;
  params->dmax = 0.f;   // (refused as it stands: the caller says how far a probe looks)
  params->normal_bias = 0.f;
  return QA_OK;
}

int qa_probevis_sh_device(qa_ctx *c, uint64_t n, const float *d_points, const uint32_t *d_stream, const qa_probe_params *params,
                          const qa_probevis_params *vis, float *d_sh, float *d_cube, uint32_t *d_hits, float *d_tmin, float *d_moments, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = ProbeVisChecks(c, n, d_points != nullptr, params, vis, d_moments != nullptr)) return rc;
  if (n == 0) return QA_OK;
  return ProbeBatch(c, n, d_points, d_stream, params, d_sh, d_cube, d_hits, d_tmin, StreamOf(c, stream), vis, d_moments);
}

int qa_probevis_sh(qa_ctx *c, uint64_t n, const float *points, const uint32_t *stream_ids, const qa_probe_params *params,
                   const qa_probevis_params *vis, float *sh, float *cube, uint32_t *hits, float *tmin, float *moments)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = ProbeVisChecks(c, n, points != nullptr, params, vis, moments != nullptr)) return rc;
  if (n == 0) return QA_OK;
  return ProbeHost(c, n, points, stream_ids, params, vis, sh, cube, hits, tmin, moments);
}

int qa_probevis_grid_shade_device(qa_ctx *c, uint64_t n, const float *d_sh, const float *d_moments, int d, const float *origin, const float *spacing,
                                  const int32_t *counts, const float *d_points, const float *d_normals, const qa_probevis_params *params,
                                  float *d_rgb, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (!GridOk(origin, spacing, counts)) return Fail(QA_EINVAL, "bad grid: finite origin, spacing > 0, counts >= 1, at most 2^31 - 1 probes");
  if (!params || !std::isfinite(params->normal_bias)) return Fail(QA_EINVAL, "null params or a normal_bias that is not finite");
  if (d < 1 || d > QA_PROBE_MAX_M) return Fail(QA_EINVAL, "d must be 1 .. 128");
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 shading points");
  if (!d_sh || !d_moments || !d_points || !d_normals || !d_rgb) return Fail(QA_EINVAL, "null array");
  hipLaunchKernelGGL(qa_probevis_grid_shade, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, StreamOf(c, stream), n, GridOf(origin, spacing, counts), d_sh,
                     d_moments, d, params->normal_bias, d_points, d_normals, d_rgb);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// ---- the same source on the CPU (no GPU and no context needed)

int qa_test_probevis_moments_host(int m, int d, float dmax, const float *t, float *out)
{
  if (m < 1 || m > QA_PROBE_MAX_M || d < 1 || d > m || m % d || !(dmax > 0.f) || !std::isfinite(dmax) || !t || !out) return QA_EINVAL;
  for (uint32_t cell = 0; cell < 6u * (uint32_t) d * (uint32_t) d; ++cell) probeVisMoments((uint32_t) m, (uint32_t) d, dmax, t, cell, out + 2 * cell);
  return QA_OK;
}

int qa_test_probevis_grid_shade_host(uint64_t n, const float *sh, const float *moments, int d, const float *origin, const float *spacing, const int32_t *counts,
                                     const float *points, const float *normals, const qa_probevis_params *params, float *rgb)
{
  if (!GridOk(origin, spacing, counts) || !params || !std::isfinite(params->normal_bias) || d < 1 || d > QA_PROBE_MAX_M) return QA_EINVAL;
  if (n == 0) return QA_OK;
  if (!sh || !moments || !points || !normals || !rgb) return QA_EINVAL;
  const ProbeGrid g = GridOf(origin, spacing, counts);
  for (uint64_t i = 0; i < n; ++i) probeVisGridShade(g, sh, moments, d, params->normal_bias, points + 3 * i, normals + 3 * i, rgb + 3 * i);
  return QA_OK;
}

// the n probes with stream ids stream [n]: d [n][K][3], w [n][K], ray_stream [n][K] (each may be null, not all)
int qa_test_probe_directions_host(int m, uint32_t seed, uint32_t flags, const uint32_t *stream, uint64_t n, float *d, float *w, uint32_t *ray_stream)
{
  if (m < 1 || m > QA_PROBE_MAX_M || (flags & ~QA_PROBE_JITTER)) return QA_EINVAL;
  if (n && (!stream || (!d && !w && !ray_stream))) return QA_EINVAL;
  const uint32_t K = 6u * (uint32_t) m * (uint32_t) m;
  for (uint64_t q = 0; q < n; ++q)
    for (uint32_t k = 0; k < K; ++k) {
      const ProbeDir pd = probeRecord((uint32_t) m, seed, stream[q], k, (flags & QA_PROBE_JITTER) != 0);
      const uint64_t r = q * K + k;
      if (d) { d[3 * r] = pd.d[0]; d[3 * r + 1] = pd.d[1]; d[3 * r + 2] = pd.d[2]; }
      if (w) w[r] = pd.w;
      if (ray_stream) ray_stream[r] = probeRayStream(stream[q], K, k);
    }
  return QA_OK;
}

// one probe's projection as the wave does it: K rays d [K][3], w [K], rgb [K][3], t [K] -> sh [27], hits [1], tmin [1] (the last two may be null)
int qa_test_probe_project_host(uint64_t K, const float *d, const float *w, const float *rgb, const float *t, float *sh, uint32_t *hits, float *tmin)
{
  if (!sh || (K && (!d || !w || !rgb || !t))) return QA_EINVAL;
  ProbeAcc lanes[QA_PROBE_LANES], next[QA_PROBE_LANES];
  for (uint32_t l = 0; l < QA_PROBE_LANES; ++l) {
    probeAccInit(lanes[l]);
    for (uint64_t k = l; k < K; k += QA_PROBE_LANES) probeAccAdd(lanes[l], d + 3 * k, w[k], rgb + 3 * k, t[k]);
  }
  for (uint32_t off = 32; off >= 1; off >>= 1) {
    for (uint32_t l = 0; l < QA_PROBE_LANES; ++l) { next[l] = lanes[l]; probeAccFold(next[l], lanes[l ^ off]); }
    memcpy(lanes, next, sizeof(lanes));
  }
  probeAccFinish(lanes[0], sh);
  if (hits) *hits = lanes[0].hits;
  if (tmin) *tmin = lanes[0].tmin;
  return QA_OK;
}

int qa_test_probe_shade_host(uint64_t n, const float *sh, uint64_t probes, const float *normals, const int32_t *index, float *rgb)
{
  if (n == 0) return QA_OK;
  if (!sh || !normals || !rgb || probes < 1 || probes > QA_MAX_RAYS || (!index && probes < n)) return QA_EINVAL;
  for (uint64_t i = 0; i < n; ++i) {
    const int64_t q = probeIndex(index ? (int64_t) index[i] : (int64_t) i, (int64_t) probes);
    probeShade(sh + 27 * q, normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], rgb + 3 * i);
  }
  return QA_OK;
}

int qa_test_probe_grid_shade_host(uint64_t n, const float *sh, const float *origin, const float *spacing, const int32_t *counts, const float *points,
                                  const float *normals, float *rgb)
{
  if (!GridOk(origin, spacing, counts)) return QA_EINVAL;
  if (n == 0) return QA_OK;
  if (!sh || !points || !normals || !rgb) return QA_EINVAL;
  const ProbeGrid g = GridOf(origin, spacing, counts);
  for (uint64_t i = 0; i < n; ++i) probeGridShade(g, sh, points + 3 * i, normals + 3 * i, rgb + 3 * i);
  return QA_OK;
}

}  // extern "C"
