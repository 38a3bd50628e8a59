// qa_reflprobe.hip — reflection probes (qa_reflprobe_*): a probe's cube map prefiltered into a chain of Phong-convolved levels, and the
// glossy lookup a viewer makes in it every frame, at one probe per shading point or blended over a grid's cell.  The opening comment
// of qa_reflprobe_dev.h is the specification of all arithmetic; this unit holds the kernels around it, the entries of the C ABI and
// the host hooks that run the same source on the CPU.
//
// No ray is traced and no scene is read here: the calls read and write arrays of the caller's and order nothing.
//
// The prefilter is the dense one: every filtered texel of a probe meets every source texel (m = 16, L = 5: 510 x 1536 pairs).  Output
// texels are the only parallel dimension - the sum is sequential by specification - so a thread owns one output texel and walks the
// source records in ascending k.  A record (d, w, rgb) is the same for all lanes of a wave in the same turn: the workgroup stages the
// records in LDS, (d, w) computed once per piece by probeDirection and rgb read from the cube, and every lane reads the same address,
// a conflict-free broadcast.
#include "qa_reflprobe_dev.h"
#include "qa_raybatch.h"

namespace qa {

#define QA_REFL_THREADS 512   // m = 16, L = 5: 510 filtered texels, one workgroup per probe
#define QA_REFL_PIECE 1536    // source records staged at a time: a whole m = 16 cube, 48 KB of LDS with rgb padded to 16 bytes

struct ReflPrefilter {
  const float *cube;   // [n][K][3]
  float *chain;        // [n][T][3]
  uint64_t n;
  uint32_t m, lg, L, K, T;
  uint32_t F;          // filtered texels per probe, T - K
  uint32_t lanes;      // the lanes a probe takes in a workgroup: a multiple of 64, QA_REFL_THREADS when a probe fills it
  uint32_t share;      // probes per workgroup, QA_REFL_THREADS / lanes: > 1 only when the whole cube is one piece
};

// Level 0: the cube, bit for bit.  One thread per float, grid-stride
__global__ __launch_bounds__(256) void qa_reflprobe_copy(const float *cube, float *chain, uint64_t n, uint64_t perCube, uint64_t perChain)
{
  const uint64_t total = n * perCube, stride = (uint64_t) gridDim.x * 256;
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < total; i += stride) chain[(i / perCube) * perChain + i % perCube] = cube[i];
}

// a staged piece's records, ascending, folded into one output texel
__device__ __forceinline__ void reflWalk(ReflAcc &acc, const float o[3], uint32_t squarings, const float4 *dir, const float4 *rgb, uint32_t len)
{
  // (the next record is read while this one is folded in: without the read ahead every pair waits for its own LDS read)
  float4 d = dir[0], c = rgb[0];
  for (uint32_t i = 0; i < len; ++i) {
    const uint32_t next = (i + 1 < len) ? i + 1 : i;
    const float4 dn = dir[next], cn = rgb[next];
    reflAccAdd(acc, o, squarings, d.x, d.y, d.z, d.w, c.x, c.y, c.z);
    d = dn;
    c = cn;
  }
}

// Levels 1 .. L - 1.  blockIdx.x: a group of `share` probes; blockIdx.y: a run of QA_REFL_THREADS filtered texels of the probe
// (more than one only when share == 1).  The lanes of a probe are whole waves; its filtered texels are numbered level after level,
// so a wave holds texels of one level except where a level ends inside it
__global__ __launch_bounds__(QA_REFL_THREADS) void qa_reflprobe_prefilter(const ReflPrefilter g)
{
  __shared__ float4 sDir[QA_REFL_PIECE];   // d.x, d.y, d.z, w of the piece's records: every probe's
  __shared__ float4 sRgb[QA_REFL_PIECE];   // [slot][record] rgb (and a pad) of the workgroup's probes
  const uint32_t slot = threadIdx.x / g.lanes;
  const uint64_t probe = (uint64_t) blockIdx.x * g.share + slot;
  const uint32_t texel = blockIdx.y * QA_REFL_THREADS + threadIdx.x % g.lanes;
  const bool live = slot < g.share && probe < g.n && texel < g.F;
  // (an idle lane walks with the probe's last texel and stores nothing: the squaring count stays the wave's)
  uint32_t j = texel < g.F ? texel : g.F - 1u;
  uint32_t l = 1, off = g.K;
  for (; l + 1 < g.L; ++l) {
    const uint32_t count = 6u * (g.m >> l) * (g.m >> l);
    if (j < count) break;
    j -= count;
    off += count;
  }
  const ProbeDir o = probeDirection(g.m >> l, j, .5f, .5f);
  const uint32_t squarings = reflSquarings((int) g.lg, (int) l);
  const uint32_t first = (uint32_t) __builtin_amdgcn_readfirstlane((int) squarings);
  const bool uniform = __all(squarings == first);
  ReflAcc acc = {{0.f, 0.f, 0.f}, 0.f};
  for (uint32_t k0 = 0; k0 < g.K; k0 += QA_REFL_PIECE) {
    const uint32_t len = (g.K - k0 < QA_REFL_PIECE) ? g.K - k0 : QA_REFL_PIECE;
    if (k0) __syncthreads();   // (the piece before has been read)
    for (uint32_t i = threadIdx.x; i < len; i += QA_REFL_THREADS) {
      const ProbeDir d = probeDirection(g.m, k0 + i, .5f, .5f);
      sDir[i] = make_float4(d.d[0], d.d[1], d.d[2], d.w);
    }
    for (uint32_t e = threadIdx.x; e < g.share * len; e += QA_REFL_THREADS) {
      const uint64_t q = (uint64_t) blockIdx.x * g.share + e / len;
      float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < g.n) {
        const float *src = g.cube + 3 * (q * g.K + k0 + e % len);
        c = make_float4(src[0], src[1], src[2], 0.f);
      }
      sRgb[e] = c;
    }
    __syncthreads();
    const float4 *rgb = sRgb + (slot < g.share ? slot : 0u) * len;
    // the squaring counts there are (0, and the odd 2 (lg - l) - 1 up to 13 at m = 128) as constants, so that the pair loop of a
    // wave of one level carries no inner loop; a wave across a level's end counts per lane
    switch (uniform ? first : ~0u) {
      case 0u: reflWalk(acc, o.d, 0u, sDir, rgb, len); break;
      case 1u: reflWalk(acc, o.d, 1u, sDir, rgb, len); break;
      case 3u: reflWalk(acc, o.d, 3u, sDir, rgb, len); break;
      case 5u: reflWalk(acc, o.d, 5u, sDir, rgb, len); break;
      case 7u: reflWalk(acc, o.d, 7u, sDir, rgb, len); break;
      case 9u: reflWalk(acc, o.d, 9u, sDir, rgb, len); break;
      case 11u: reflWalk(acc, o.d, 11u, sDir, rgb, len); break;
      case 13u: reflWalk(acc, o.d, 13u, sDir, rgb, len); break;
      default: reflWalk(acc, o.d, squarings, sDir, rgb, len); break;
    }
  }
  if (live) {
    float *out = g.chain + 3 * (probe * g.T + off + j);
    out[0] = acc.a[0] / acc.W;
    out[1] = acc.a[1] / acc.W;
    out[2] = acc.a[2] / acc.W;
  }
}

// One thread per shading point
__global__ __launch_bounds__(256) void qa_reflprobe_shade(uint64_t n, const float *chain, int64_t probes, uint32_t m, int L, const float *dirs, const float *level,
                                                          const int32_t *index, float *rgb)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t q = probeIndex(index ? (int64_t) index[i] : (int64_t) i, probes);
  const float R[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
  float out[3];
  reflLookup(chain + (size_t) 3 * reflOffset(m, L) * (size_t) q, m, L, R, level[i], out);
  rgb[3 * i] = out[0]; rgb[3 * i + 1] = out[1]; rgb[3 * i + 2] = out[2];
}

__global__ __launch_bounds__(256) void qa_reflprobe_grid_shade(uint64_t n, const ProbeGrid grid, const float *chain, uint32_t m, int L, const float *points,
                                                               const float *dirs, const float *level, float *rgb)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float P[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]}, R[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
  float out[3];
  reflGridLookup(grid, chain, m, L, P, R, level[i], out);
  rgb[3 * i] = out[0]; rgb[3 * i + 1] = out[1]; rgb[3 * i + 2] = out[2];
}

}  // namespace qa

// m a power of two in 1 .. 128 and levels in 1 .. lg + 1 -> lg, else -1
static int ChainLog2(int m, int levels)
{
  const int lg = reflLog2(m);
  return (lg < 0 || levels < 1 || levels > lg + 1) ? -1 : lg;
}

// How the prefilter's workgroups take the probes' filtered texels (F > 0)
static ReflPrefilter PrefilterPlan(uint64_t n, const float *cube, int m, int lg, int levels, float *chain)
{
  ReflPrefilter g = {cube, chain, n, (uint32_t) m, (uint32_t) lg, (uint32_t) levels, 6u * m * m, reflOffset((uint32_t) m, levels), 0, 0, 0};
  g.F = g.T - g.K;
  g.lanes = std::min<uint32_t>(QA_REFL_THREADS, (g.F + 63u) / 64u * 64u);
  // several probes share a workgroup only where all their records fit its LDS at once (m <= 8)
  g.share = std::max<uint32_t>(1u, std::min<uint32_t>(QA_REFL_THREADS / g.lanes, QA_REFL_PIECE / g.K));
  return g;
}

extern "C" {

int qa_reflprobe_layout(int m, int levels, uint32_t *offset, uint32_t *res, uint32_t *squarings, uint64_t *texels)
{
  const int lg = ChainLog2(m, levels);
  if (lg < 0) return Fail(QA_EINVAL, "m must be a power of two in 1 .. 128 and levels 1 .. log2 m + 1");
  for (int l = 0; l < levels; ++l) {
    if (offset) offset[l] = reflOffset((uint32_t) m, l);
    if (res) res[l] = (uint32_t) m >> l;
    if (squarings) squarings[l] = l ? reflSquarings(lg, l) : 0u;
  }
  if (texels) *texels = reflOffset((uint32_t) m, levels);
  return QA_OK;
}

int qa_reflprobe_prefilter_device(qa_ctx *c, uint64_t n, const float *d_cube, int m, int levels, float *d_chain, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 probes");
  if (!d_cube || !d_chain) return Fail(QA_EINVAL, "null array");
  const int lg = ChainLog2(m, levels);
  if (lg < 0) return Fail(QA_EINVAL, "m must be a power of two in 1 .. 128 and levels 1 .. log2 m + 1");
  const hipStream_t s = StreamOf(c, stream);
  const uint64_t K = 6ull * m * m, T = reflOffset((uint32_t) m, levels);
  const uint64_t copyBlocks = std::min<uint64_t>((n * K * 3 + 255) / 256, 1u << 20);
  hipLaunchKernelGGL(qa_reflprobe_copy, dim3((unsigned) copyBlocks), dim3(256), 0, s, d_cube, d_chain, n, K * 3, T * 3);
  HIP_TRY(hipGetLastError());
  if (T == K) return QA_OK;   // (one level: the copy is all of it)
  const ReflPrefilter g = PrefilterPlan(n, d_cube, m, lg, levels, d_chain);
  const dim3 grid((unsigned) ((n + g.share - 1) / g.share), (g.F + g.lanes - 1) / g.lanes);
  hipLaunchKernelGGL(qa_reflprobe_prefilter, grid, dim3(QA_REFL_THREADS), 0, s, g);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

int qa_reflprobe_shade_device(qa_ctx *c, uint64_t n, const float *d_chain, uint64_t probes, int m, int levels, const float *d_dirs, const float *d_level,
                              const int32_t *d_index, float *d_rgb, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 shading points");
  if (!d_chain || !d_dirs || !d_level || !d_rgb) return Fail(QA_EINVAL, "null array");
  if (ChainLog2(m, levels) < 0) return Fail(QA_EINVAL, "m must be a power of two in 1 .. 128 and levels 1 .. log2 m + 1");
  if (probes < 1 || probes > QA_MAX_RAYS) return Fail(QA_EINVAL, "bad probe count");
  if (!d_index && probes < n) return Fail(QA_EINVAL, "fewer probes than shading points and no index");
  hipLaunchKernelGGL(qa_reflprobe_shade, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, StreamOf(c, stream), n, d_chain, (int64_t) probes, (uint32_t) m, levels,
                     d_dirs, d_level, d_index, d_rgb);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

int qa_reflprobe_grid_shade_device(qa_ctx *c, uint64_t n, const float *d_chain, int m, int levels, const float *origin, const float *spacing,
                                   const int32_t *counts, const float *d_points, const float *d_dirs, const float *d_level, float *d_rgb, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (!GridOk(origin, spacing, counts)) return Fail(QA_EINVAL, "bad grid: finite origin, spacing > 0, counts >= 1, at most 2^31 - 1 probes");
  if (ChainLog2(m, levels) < 0) return Fail(QA_EINVAL, "m must be a power of two in 1 .. 128 and levels 1 .. log2 m + 1");
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 shading points");
  if (!d_chain || !d_points || !d_dirs || !d_level || !d_rgb) return Fail(QA_EINVAL, "null array");
  hipLaunchKernelGGL(qa_reflprobe_grid_shade, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, StreamOf(c, stream), n, GridOf(origin, spacing, counts), d_chain,
                     (uint32_t) m, levels, d_points, d_dirs, d_level, d_rgb);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// ---- the same source on the CPU (no GPU and no context needed)

int qa_test_reflprobe_prefilter_host(uint64_t n, const float *cube, int m, int levels, float *chain)
{
  if (n == 0) return QA_OK;
  const int lg = ChainLog2(m, levels);
  if (n > QA_MAX_RAYS || !cube || !chain || lg < 0) return QA_EINVAL;
  const uint32_t K = 6u * m * m, T = reflOffset((uint32_t) m, levels);
  std::vector<ProbeDir> rec(K);
  for (uint32_t k = 0; k < K; ++k) rec[k] = probeDirection((uint32_t) m, k, .5f, .5f);
  for (uint64_t q = 0; q < n; ++q) {
    const float *src = cube + 3 * q * K;
    float *dst = chain + 3 * q * T;
    memcpy(dst, src, (size_t) 12 * K);
    for (int l = 1; l < levels; ++l) {
      const uint32_t off = reflOffset((uint32_t) m, l), count = 6u * (m >> l) * (m >> l);
      for (uint32_t k = 0; k < count; ++k) reflPrefilterTexel((uint32_t) m, lg, l, k, rec.data(), src, dst + 3 * (off + k));
    }
  }
  return QA_OK;
}

int qa_test_reflprobe_shade_host(uint64_t n, const float *chain, uint64_t probes, int m, int levels, const float *dirs, const float *level,
                                 const int32_t *index, float *rgb)
{
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS || !chain || !dirs || !level || !rgb || ChainLog2(m, levels) < 0 || probes < 1 || probes > QA_MAX_RAYS || (!index && probes < n))
    return QA_EINVAL;
  const size_t perProbe = (size_t) 3 * reflOffset((uint32_t) m, levels);
  for (uint64_t i = 0; i < n; ++i) {
    const int64_t q = probeIndex(index ? (int64_t) index[i] : (int64_t) i, (int64_t) probes);
    reflLookup(chain + perProbe * (size_t) q, (uint32_t) m, levels, dirs + 3 * i, level[i], rgb + 3 * i);
  }
  return QA_OK;
}

int qa_test_reflprobe_grid_shade_host(uint64_t n, const float *chain, int m, int levels, const float *origin, const float *spacing, const int32_t *counts,
                                      const float *points, const float *dirs, const float *level, float *rgb)
{
  if (!GridOk(origin, spacing, counts) || ChainLog2(m, levels) < 0) return QA_EINVAL;
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS || !chain || !points || !dirs || !level || !rgb) return QA_EINVAL;
  const ProbeGrid g = GridOf(origin, spacing, counts);
  for (uint64_t i = 0; i < n; ++i) reflGridLookup(g, chain, (uint32_t) m, levels, points + 3 * i, dirs + 3 * i, level[i], rgb + 3 * i);
  return QA_OK;
}

}  // extern "C"
