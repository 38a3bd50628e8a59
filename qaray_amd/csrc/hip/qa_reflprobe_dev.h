// qa_reflprobe_dev.h — reflection probes: a probe's cube map (qa_probe_sh_device's cube output, path-traced by the renderer's own
// integrator) convolved with Phong lobes of decreasing sharpness into a chain of ever smaller cube maps, and the lookup a glossy
// material makes in it - a direction and a level, blended between texels and between levels; the grid form blends the eight probes
// of a point's cell.  This comment is the specification; tests/reflprobe_util.py restates it in float32 numpy and
// tests/test_reflprobe_host.py holds the host build of the functions below to that restatement bit for bit.
//
// All arithmetic is fp32 in the order written, nothing is contracted, `/` and sqrtf are the correctly rounded ones, denormals are
// kept.  No trig, exp, log or pow is used.  probeDirection (DIRECTIONS there), probeGridAxis, probeLerp, probeIndex and probeVoid are
// qa_lightprobe_dev.h's: used from that header, not restated here.
//
// CHAIN.  The source is a cube [6][m][m][3] as qa_probe_sh_device writes it; m is a power of two, 1 <= m <= 128, lg = log2 m.  A
// chain has L levels, 1 <= L <= lg + 1.  Level l has r_l = m >> l texels per face edge and starts at texel off_l = 6 * sum_{j<l}
// r_j^2; T = off_L texels in all, and the layout of n probes' chains is [n][T][3] floats.
//   Level 0 is the cube, copied bit for bit: the mirror level.
//   Level l >= 1 is the cube convolved with the Phong lobe max(0, dot)^(2^s_l), s_l = max(0, 2 * (lg - l) - 1): the power is taken
//   by s_l squarings (m = 16: exponents 32, 8, 2, 1 at 8, 4, 2, 1 texels per face edge - halving the resolution doubles the lobe's
//   width, and a lobe of exponent r^2 / 2 is about one texel of an r x r face wide).
// Output texel k' (0 <= k' < 6 r_l^2) of level l has the direction o = probeDirection(r_l, k', .5f, .5f).d and four accumulators -
// acc[3] and W - all +0 at the start.  For the source records k = 0 .. 6 m^2 - 1, ascending, with (d, w) = probeDirection(m, k,
// .5f, .5f) and rgb_k the cube's texel k:
//   c = ((o.x * d.x) + (o.y * d.y)) + (o.z * d.z);   c = (c > 0.f) ? c : 0.f;   s_l times: c = c * c
//   if (c > 0.f) { q = c * w;  acc[ch] = acc[ch] + (q * rgb_k[ch]);  W = W + q; }
// and then out[ch] = acc[ch] / W.  The texel's own direction always contributes, so W > 0.  A void probe's zeros stay zeros; a NaN
// texel reaches exactly the outputs whose lobe covers it (c > 0 after the squarings: a lobe that underflowed to 0 does not).  The
// sum is sequential per output texel: output texels are the only parallel dimension, and nothing else about the mapping is fixed.
//
// LOOKUP of a direction R = (R0, R1, R2) (any length) at level lambda (a float) in one probe's chain.  If a component of R is not
// finite, R is (0, 0, 0), or lambda is NaN, the answer is (0, 0, 0).  Otherwise:
//   face: axis a = argmax |R_a|, the lowest a on ties; ma = |R_a|; f = 2 a + (R_a < 0 ? 1 : 0); s = +1.f for even f, -1.f for odd
//         (probeVisCell's rule);  u = R[(a + 1) % 3] / ma,  v = (s * R[(a + 2) % 3]) / ma
//   level: (l0, l1, fl) = probeGridAxis(lambda, 0.f, 1.f, L): lambda clamped to [0, L - 1], l0 = min((int) lambda, L - 2), ...
//   in level l with r = r_l, for t = u (columns) and t = v (rows):
//         g = ((t + 1.f) * 0.5f) * (float) r - 0.5f;   (i0, i1, ft) = probeGridAxis(g, 0.f, 1.f, r)
//         (the clamp holds the coordinate at the face's edge: nothing is filtered across face borders)
//   with texel (row b, column c) of face f at off_l + (f * r + b) * r + c and lerp(a, b, f) = ((1.f - f) * a) + (f * b), per channel:
//         x0 = lerp(tex(b0, c0), tex(b0, c1), fu);  x1 = lerp(tex(b1, c0), tex(b1, c1), fu);  level_l = lerp(x0, x1, fv)
//   rgb = lerp(level_l0, level_l1, fl)                       (with L = 1 both are level 0 and fl = 0)
// With an index array, lookup i reads probe min(max(index[i], 0), probes - 1), as qa_probe_shade_device clamps it.
//
// GRID LOOKUP.  The point's cell is probeGridAxis's per axis (GRID SHADING there).  The lookup above is made in each of the cell's
// eight probes, (i0 or i1 per axis), and the eight results (three floats each) are blended with the same lerp along x between the
// four (y, z) corners, then along y, then along z.  A point on a probe takes that probe's answer exactly (f = 0 or 1 and finite
// texels).  A point with a component that is not finite answers (0, 0, 0).  There is no parallax correction: every probe is asked
// for the same direction.
//
// Every function here is compiled for the host too: qa_test_reflprobe_*_host and the kernels of qa_reflprobe.hip run the same source.
#pragma once
#include "qa_lightprobe_dev.h"

namespace qa {

#define QA_REFLPROBE_MAX_LEVELS 8   // lg + 1 at m = 128

// log2 m for a power of two in 1 .. 128, else -1
__host__ __device__ __forceinline__ int reflLog2(int m)
{
  if (m < 1 || m > QA_PROBE_MAX_M || (m & (m - 1))) return -1;
  int lg = 0;
  while ((1 << lg) < m) ++lg;
  return lg;
}
// the squarings of level l >= 1 (level 0 is the copy)
__host__ __device__ __forceinline__ uint32_t reflSquarings(int lg, int l)
{
  const int s = 2 * (lg - l) - 1;
  return (uint32_t) (s > 0 ? s : 0);
}
// the first texel of level l (l = L: the chain's texels T)
__host__ __device__ __forceinline__ uint32_t reflOffset(uint32_t m, int l)
{
  uint32_t off = 0;
  for (int j = 0; j < l; ++j) off += 6u * (m >> j) * (m >> j);
  return off;
}

struct ReflAcc { float a[3], W; };

// the lobe's weight of source direction d seen from output direction o, before the texel's solid angle
__host__ __device__ __forceinline__ float reflLobe(const float o[3], float dx, float dy, float dz, uint32_t squarings)
{
  float c = ((o[0] * dx) + (o[1] * dy)) + (o[2] * dz);
  c = (c > 0.f) ? c : 0.f;
  for (uint32_t i = 0; i < squarings; ++i) c = c * c;
  return c;
}
// one source record folded into an output texel's accumulators
__host__ __device__ __forceinline__ void reflAccAdd(ReflAcc &acc, const float o[3], uint32_t squarings, float dx, float dy, float dz, float w,
                                                    float r, float g, float b)
{
  const float c = reflLobe(o, dx, dy, dz, squarings);
  if (c > 0.f) {
    const float q = c * w;
    acc.a[0] = acc.a[0] + (q * r);
    acc.a[1] = acc.a[1] + (q * g);
    acc.a[2] = acc.a[2] + (q * b);
    acc.W = acc.W + q;
  }
}

// output texel k of level l >= 1 of one probe from its cube [6 m^2][3] and the source records rec [6 m^2] (probeDirection(m, s, .5f,
// .5f), computed once: they are every probe's and every output texel's): the whole sum, record by record
__host__ __device__ __forceinline__ void reflPrefilterTexel(uint32_t m, int lg, int l, uint32_t k, const ProbeDir *rec, const float *cube, float out[3])
{
  const ProbeDir o = probeDirection(m >> l, k, .5f, .5f);
  const uint32_t squarings = reflSquarings(lg, l), K = 6u * m * m;
  ReflAcc acc = {{0.f, 0.f, 0.f}, 0.f};
  for (uint32_t s = 0; s < K; ++s)
    reflAccAdd(acc, o.d, squarings, rec[s].d[0], rec[s].d[1], rec[s].d[2], rec[s].w, cube[3 * s], cube[3 * s + 1], cube[3 * s + 2]);
  for (int ch = 0; ch < 3; ++ch) out[ch] = acc.a[ch] / acc.W;
}

// the face R points into and its two coordinates there (R finite and not zero)
__host__ __device__ __forceinline__ int reflFace(const float R[3], float &u, float &v)
{
  const float m0 = fabsf(R[0]), m1 = fabsf(R[1]), m2 = fabsf(R[2]);
  int a = 0;
  float ma = m0;
  if (m1 > ma) { a = 1; ma = m1; }
  if (m2 > ma) { a = 2; ma = m2; }
  const float va = a == 0 ? R[0] : a == 1 ? R[1] : R[2];
  const float vu = a == 0 ? R[1] : a == 1 ? R[2] : R[0];
  const float vw = a == 0 ? R[2] : a == 1 ? R[0] : R[1];
  const bool neg = va < 0.f;
  const float s = neg ? -1.f : 1.f;
  u = vu / ma;
  v = (s * vw) / ma;
  return 2 * a + (neg ? 1 : 0);
}

// the bilinear lookup in level l of one probe's chain [T][3]
__host__ __device__ __forceinline__ void reflLevelLookup(const float *chain, uint32_t m, int l, int face, float u, float v, float rgb[3])
{
  const int r = (int) (m >> l);
  const float fr = (float) r;
  int c0, c1, b0, b1;
  float fu, fv;
  probeGridAxis(((u + 1.f) * 0.5f) * fr - 0.5f, 0.f, 1.f, r, c0, c1, fu);
  probeGridAxis(((v + 1.f) * 0.5f) * fr - 0.5f, 0.f, 1.f, r, b0, b1, fv);
  const float *base = chain + 3 * ((size_t) reflOffset(m, l) + (size_t) face * r * r);
  const float *t00 = base + 3 * (b0 * r + c0), *t01 = base + 3 * (b0 * r + c1), *t10 = base + 3 * (b1 * r + c0), *t11 = base + 3 * (b1 * r + c1);
  for (int ch = 0; ch < 3; ++ch) {
    const float x0 = probeLerp(t00[ch], t01[ch], fu);
    const float x1 = probeLerp(t10[ch], t11[ch], fu);
    rgb[ch] = probeLerp(x0, x1, fv);
  }
}

// what no lookup answers: a direction that is not finite or zero, a level that is NaN
__host__ __device__ __forceinline__ bool reflVoid(const float R[3], float lambda)
{
  return probeVoid(R[0], R[1], R[2]) || (R[0] == 0.f && R[1] == 0.f && R[2] == 0.f) || lambda != lambda;
}

// where a lookup reads: the face, its two coordinates, the two levels and the weight of the second
struct ReflTap { int face, l0, l1; float u, v, fl; };
__host__ __device__ __forceinline__ ReflTap reflTap(const float R[3], float lambda, int L)
{
  ReflTap t;
  t.face = reflFace(R, t.u, t.v);
  probeGridAxis(lambda, 0.f, 1.f, L, t.l0, t.l1, t.fl);
  return t;
}
// the two levels of one probe's chain [T][3] at tap t, blended
__host__ __device__ __forceinline__ void reflFetch(const float *chain, uint32_t m, const ReflTap &t, float rgb[3])
{
  float lo[3], hi[3];
  reflLevelLookup(chain, m, t.l0, t.face, t.u, t.v, lo);
  reflLevelLookup(chain, m, t.l1, t.face, t.u, t.v, hi);
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = probeLerp(lo[ch], hi[ch], t.fl);
}

// the lookup of direction R at level lambda in one probe's chain [T][3] of L levels
__host__ __device__ __forceinline__ void reflLookup(const float *chain, uint32_t m, int L, const float R[3], float lambda, float rgb[3])
{
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (reflVoid(R, lambda)) return;
  reflFetch(chain, m, reflTap(R, lambda, L), rgb);
}

// the lookup at point P from the chains [probes][T][3] of grid G
__host__ __device__ __forceinline__ void reflGridLookup(const ProbeGrid &G, const float *chain, uint32_t m, int L, const float P[3], const float R[3],
                                                        float lambda, float rgb[3])
{
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (probeVoid(P[0], P[1], P[2]) || reflVoid(R, lambda)) return;
  int i0[3], i1[3];
  float f[3];
  for (int e = 0; e < 3; ++e) probeGridAxis(P[e], G.origin[e], G.spacing[e], G.counts[e], i0[e], i1[e], f[e]);
  const int64_t nx = G.counts[0], ny = G.counts[1];
  const size_t perProbe = (size_t) 3 * reflOffset(m, L);
  const ReflTap tap = reflTap(R, lambda, L);
  float corner[8][3];
  for (int j = 0; j < 8; ++j) {
    const int64_t probe = ((int64_t) ((j & 4) ? i1[2] : i0[2]) * ny + ((j & 2) ? i1[1] : i0[1])) * nx + ((j & 1) ? i1[0] : i0[0]);
    reflFetch(chain + perProbe * (size_t) probe, m, tap, corner[j]);
#if defined(__HIP_DEVICE_COMPILE__)
    // probe by probe, as probeVisGridShade: without the fence the scheduler gathers all eight probes' taps ahead of the blends
    __builtin_amdgcn_sched_barrier(0);
#endif
  }
  for (int ch = 0; ch < 3; ++ch) {
    const float x00 = probeLerp(corner[0][ch], corner[1][ch], f[0]);
    const float x01 = probeLerp(corner[2][ch], corner[3][ch], f[0]);
    const float x10 = probeLerp(corner[4][ch], corner[5][ch], f[0]);
    const float x11 = probeLerp(corner[6][ch], corner[7][ch], f[0]);
    const float y0 = probeLerp(x00, x01, f[1]);
    const float y1 = probeLerp(x10, x11, f[1]);
    rgb[ch] = probeLerp(y0, y1, f[2]);
  }
}

}  // namespace qa
