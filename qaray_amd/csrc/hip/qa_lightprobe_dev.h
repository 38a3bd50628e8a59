// qa_lightprobe_dev.h — light probes on the resident scene: the radiance arriving at a point in free space from the directions of a
// cube map, projected onto the real spherical harmonics of order 2, and the shading of a normal from those 27 coefficients.  This
// comment is the specification; tests/probe_util.py restates it in float32 numpy and tests/test_probe_host.py holds the host build
// of the functions below to that restatement bit for bit.
//
// All arithmetic is fp32 in the order written, nothing is contracted, `/` and sqrtf are the correctly rounded ones.  No trig, exp
// or pow is used.  Integers are uint32 and wrap unless said otherwise.  mix, key and kr are qa_ao_dev.h's (aoMix, aoKey, aoRayKey),
// and so is the word-to-float step aoSigned: they are used from that header, not restated here.
//
// DIRECTIONS.  A probe of resolution m (1 <= m <= 128) has K = 6 m^2 directions: the texels of a cube map of m x m texels per face.
// Record k = 0 .. K - 1:
//   f = k / m^2 (face), b = (k % m^2) / m (row), c = k % m (column)
//   step = 2.f / (float) m
//   u = ((float) c + j0) * step - 1.f           v = ((float) b + j1) * step - 1.f
//   l2 = (u * u + v * v) + 1.f                  i = 1.f / sqrtf(l2)
//   axis a = f / 2, sign s = +1.f for even f and -1.f for odd f (1 - 2 * (f % 2)); with d indexed 0 = x, 1 = y, 2 = z:
//   d[a] = s * i        d[(a + 1) % 3] = u * i        d[(a + 2) % 3] = s * (v * i)
//   weight (the texel's solid angle)  w = ((4.f / (float) (m * m)) * i) / l2
// The offsets: j0 = j1 = 0.5f (texel centres); with QA_PROBE_JITTER, for t = 0, 1
//   j_t = (aoSigned(mix(kr ^ (t + 1) * 0x9E3779B9)) + 1.f) * 0.5f        in [0, 1)
//   kr  = aoRayKey(aoKey(seed, S), k)            S: the probe's stream id (its index in the batch, or the caller's id)
//
// RAYS.  Ray (q, k) starts at the probe's position P_q, runs along d and draws from the random-number stream of pixel index
// (S_q * K + k) mod 2^32: it is one ray of qa_radiance_rays_device with QA_RADIANCE_MISS_ENVIRONMENT, spp samples, and everything
// that call says of a ray holds (qa_radiance.hip).  rgb is the mean of its samples, t the parameter of sample 0's first hit, 1e30
// on a miss.
//
// VOID PROBES.  A probe with a component of P that is not finite: its rays are void rays of the radiance query (not walked, nothing
// drawn), its 27 coefficients and its cube texels are +0, hits = 0, tmin = 1e30.
//
// THE BASIS.  The nine real spherical harmonics of order 2 as polynomials of d = (x, y, z), used as given (not normalised):
//   Y0 = 0.282095f
//   Y1 = 0.488603f * y              Y2 = 0.488603f * z              Y3 = 0.488603f * x
//   Y4 = 1.092548f * (x * y)        Y5 = 1.092548f * (y * z)        Y6 = 0.315392f * ((3.f * (z * z)) - 1.f)
//   Y7 = 1.092548f * (x * z)        Y8 = 0.546274f * ((x * x) - (y * y))
//
// PROJECTION, one wave of 64 lanes per probe.  Lane l holds 28 accumulators - acc[c][ch] for the nine functions and three colours,
// and W - all +0 at the start, a count of hits (0) and a least t (1e30).  For k = l, l + 64, l + 128, ... < K, ascending:
//   acc[c][ch] = acc[c][ch] + ((w_k * rgb_k[ch]) * Y_c(d_k))          W = W + w_k
//   hits += (t_k < 1e30) ? 1 : 0                                        tmin = (t_k < tmin) ? t_k : tmin
// Then for off = 32, 16, 8, 4, 2, 1 every lane l replaces each accumulator a by a + a_of_lane(l ^ off), all lanes at once (fp32
// addition commutes: every lane ends with the same bits); hits add and tmin takes (other < tmin) ? other : tmin likewise.
//   sh[c][ch] = acc[c][ch] * (12.566371f / W)
// The layout of a probe's coefficients is [9][3] floats, function-major.  Dividing by the measured W and not by the 4 pi the weights
// approximate makes a constant radiance project onto Y0 alone up to rounding.  hits and tmin are exact and independent of the order.
//
// SHADING a normal N = (x, y, z) (unit length assumed, used as given) from coefficients sh[9][3]: per channel ch
//   s = +0;  for c = 0 .. 8 ascending:  s = s + ((A_c * sh[c][ch]) * Y_c(N))
//   A_0 = 1.f,  A_1 = A_2 = A_3 = 2.f / 3.f (the fp32 quotient),  A_4 .. A_8 = 0.25f
//   rgb[ch] = (s > 0.f) ? s : 0.f                                       (a NaN sum shades to 0)
// These are the cosine lobe's band factors divided by pi: rgb is in the units of qa_irradiance_points, kd * rgb a diffuse colour.
// A normal with a component that is not finite shades to (0, 0, 0).  With an index array, shading point i reads probe
// min(max(index[i], 0), probes - 1): an index outside [0, probes) is clamped, not refused (it lives in device memory).
//
// GRID SHADING.  A regular grid of probes: origin[3], spacing[3] > 0, counts[3] >= 1, probe (iz * ny + iy) * nx + ix at
// origin + (ix, iy, iz) * spacing.  For a point p and each axis e with n = counts[e]:
//   g = (p[e] - origin[e]) / spacing[e];  g = (g < 0.f) ? 0.f : g;  g = (g > (float) (n - 1)) ? (float) (n - 1) : g
//   i0 = (n > 1) ? min((int) g, n - 2) : 0;  i1 = (n > 1) ? i0 + 1 : i0;  f = g - (float) i0
// Every one of the 27 coefficients is interpolated with lerp(a, b, f) = ((1.f - f) * a) + (f * b) along x between the probes
// (i0, i1) of the four (y, z) corners, then along y, then along z; the result is shaded as above.  A point on a probe takes that
// probe's coefficients exactly (f = 0 or 1 and finite coefficients).  A point or a normal with a component that is not finite
// shades to (0, 0, 0).
//
// Every function here is compiled for the host too: qa_test_probe_*_host and the kernels of qa_lightprobe.hip run the same source.
#pragma once
#include "qa_ao_dev.h"

namespace qa {

#define QA_PROBE_MAX_M 128
#define QA_PROBE_LANES 64
#define QA_PROBE_FOUR_PI 12.566371f

struct ProbeDir { float d[3]; float w; };

// the two offsets of record k of the probe with stream id S inside its texel
__host__ __device__ __forceinline__ void probeOffsets(uint32_t seed, uint32_t S, uint32_t k, bool jitter, float &j0, float &j1)
{
  j0 = j1 = 0.5f;
  if (!jitter) return;
  const uint32_t kr = aoRayKey(aoKey(seed, S), k);
  j0 = (aoSigned(aoMix(kr ^ 1u * QA_AO_GOLDEN)) + 1.f) * 0.5f;
  j1 = (aoSigned(aoMix(kr ^ 2u * QA_AO_GOLDEN)) + 1.f) * 0.5f;
}

// direction and weight of record k of a cube map of m x m texels per face
__host__ __device__ __forceinline__ ProbeDir probeDirection(uint32_t m, uint32_t k, float j0, float j1)
{
  const uint32_t m2 = m * m, f = k / m2, r = k % m2, b = r / m, c = r % m;
  const float step = 2.f / (float) m;
  const float u = ((float) c + j0) * step - 1.f;
  const float v = ((float) b + j1) * step - 1.f;
  const float l2 = (u * u + v * v) + 1.f;
  const float i = 1.f / sqrtf(l2);
  const uint32_t a = f / 2u;
  const float s = (f & 1u) ? -1.f : 1.f;
  ProbeDir o;
  o.d[a] = s * i;
  o.d[(a + 1u) % 3u] = u * i;
  o.d[(a + 2u) % 3u] = s * (v * i);
  o.w = ((4.f / (float) m2) * i) / l2;
  return o;
}
__host__ __device__ __forceinline__ ProbeDir probeRecord(uint32_t m, uint32_t seed, uint32_t S, uint32_t k, bool jitter)
{
  float j0, j1;
  probeOffsets(seed, S, k, jitter, j0, j1);
  return probeDirection(m, k, j0, j1);
}
// the random-number stream of ray (q, k)
__host__ __device__ __forceinline__ uint32_t probeRayStream(uint32_t S, uint32_t K, uint32_t k) { return S * K + k; }
__host__ __device__ __forceinline__ bool probeVoid(float x, float y, float z) { return !(isfinite(x) && isfinite(y) && isfinite(z)); }

// the nine basis functions at (x, y, z)
__host__ __device__ __forceinline__ void probeBasis(float x, float y, float z, float Y[9])
{
  Y[0] = 0.282095f;
  Y[1] = 0.488603f * y;
  Y[2] = 0.488603f * z;
  Y[3] = 0.488603f * x;
  Y[4] = 1.092548f * (x * y);
  Y[5] = 1.092548f * (y * z);
  Y[6] = 0.315392f * ((3.f * (z * z)) - 1.f);
  Y[7] = 1.092548f * (x * z);
  Y[8] = 0.546274f * ((x * x) - (y * y));
}

// what a lane of the projection carries
struct ProbeAcc {
  float a[28];   // [c * 3 + ch], then W
  uint32_t hits;
  float tmin;
};
__host__ __device__ __forceinline__ void probeAccInit(ProbeAcc &p)
{
  for (int i = 0; i < 28; ++i) p.a[i] = 0.f;
  p.hits = 0u;
  p.tmin = QA_AO_MAX_T;
}
__host__ __device__ __forceinline__ void probeAccAdd(ProbeAcc &p, const float d[3], float w, const float rgb[3], float t)
{
  float Y[9];
  probeBasis(d[0], d[1], d[2], Y);
  for (int c = 0; c < 9; ++c)
    for (int ch = 0; ch < 3; ++ch) p.a[c * 3 + ch] = p.a[c * 3 + ch] + ((w * rgb[ch]) * Y[c]);
  p.a[27] = p.a[27] + w;
  p.hits += (t < QA_AO_MAX_T) ? 1u : 0u;
  p.tmin = (t < p.tmin) ? t : p.tmin;
}
// one step of the butterfly: what lane l ^ off holds, folded in
__host__ __device__ __forceinline__ void probeAccFold(ProbeAcc &p, const ProbeAcc &other)
{
  for (int i = 0; i < 28; ++i) p.a[i] = p.a[i] + other.a[i];
  p.hits += other.hits;
  p.tmin = (other.tmin < p.tmin) ? other.tmin : p.tmin;
}
__host__ __device__ __forceinline__ void probeAccFinish(const ProbeAcc &p, float sh[27])
{
  const float scale = QA_PROBE_FOUR_PI / p.a[27];
  for (int i = 0; i < 27; ++i) sh[i] = p.a[i] * scale;
}

// the shading of normal (x, y, z) from 27 coefficients
__host__ __device__ __forceinline__ void probeShade(const float sh[27], float x, float y, float z, float rgb[3])
{
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (probeVoid(x, y, z)) return;
  float Y[9];
  probeBasis(x, y, z, Y);
  const float band1 = 2.f / 3.f;
  for (int ch = 0; ch < 3; ++ch) {
    float s = 0.f;
    for (int c = 0; c < 9; ++c) {
      const float A = c == 0 ? 1.f : c < 4 ? band1 : 0.25f;
      s = s + ((A * sh[c * 3 + ch]) * Y[c]);
    }
    rgb[ch] = (s > 0.f) ? s : 0.f;
  }
}
__host__ __device__ __forceinline__ int64_t probeIndex(int64_t index, int64_t probes)
{
  return index < 0 ? 0 : index > probes - 1 ? probes - 1 : index;
}

// one axis of the grid: the cell's two probes and the weight of the second
__host__ __device__ __forceinline__ void probeGridAxis(float p, float origin, float spacing, int n, int &i0, int &i1, float &f)
{
  float g = (p - origin) / spacing;
  g = (g < 0.f) ? 0.f : g;
  const float top = (float) (n - 1);
  g = (g > top) ? top : g;
  const int cell = (int) g;
  i0 = (n > 1) ? (cell < n - 2 ? cell : n - 2) : 0;
  i1 = (n > 1) ? i0 + 1 : i0;
  f = g - (float) i0;
}
__host__ __device__ __forceinline__ float probeLerp(float a, float b, float f) { return ((1.f - f) * a) + (f * b); }

struct ProbeGrid {
  float origin[3], spacing[3];
  int32_t counts[3];
};
// a grid as the entry points take it - three host arrays - checked (finite origin, spacing > 0, counts >= 1, at most 2^31 - 1
// probes) and packed: what the grid calls of qa_lightprobe.hip and qa_reflprobe.hip share
inline bool GridOk(const float *origin, const float *spacing, const int32_t *counts)
{
  if (!origin || !spacing || !counts) return false;
  uint64_t total = 1;
  for (int e = 0; e < 3; ++e) {
    if (!isfinite(origin[e]) || !isfinite(spacing[e]) || !(spacing[e] > 0.f) || counts[e] < 1) return false;
    total *= (uint64_t) counts[e];
    if (total > 0x7FFFFFFFull) return false;
  }
  return true;
}
inline ProbeGrid GridOf(const float *origin, const float *spacing, const int32_t *counts)
{
  ProbeGrid g;
  for (int e = 0; e < 3; ++e) { g.origin[e] = origin[e]; g.spacing[e] = spacing[e]; g.counts[e] = counts[e]; }
  return g;
}
// the shading of normal N at point P from the grid's coefficients sh [nz * ny * nx][27]
__host__ __device__ __forceinline__ void probeGridShade(const ProbeGrid &G, const float *sh, const float P[3], const float N[3], float rgb[3])
{
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (probeVoid(P[0], P[1], P[2]) || probeVoid(N[0], N[1], N[2])) return;
  int i0[3], i1[3];
  float f[3];
  for (int e = 0; e < 3; ++e) probeGridAxis(P[e], G.origin[e], G.spacing[e], G.counts[e], i0[e], i1[e], f[e]);
  const int64_t nx = G.counts[0], ny = G.counts[1];
  const float *corner[2][2][2];
  for (int z = 0; z < 2; ++z)
    for (int y = 0; y < 2; ++y)
      for (int x = 0; x < 2; ++x)
        corner[z][y][x] = sh + 27 * (((int64_t) (z ? i1[2] : i0[2]) * ny + (y ? i1[1] : i0[1])) * nx + (x ? i1[0] : i0[0]));
  float mixed[27];
  for (int i = 0; i < 27; ++i) {
    const float x00 = probeLerp(corner[0][0][0][i], corner[0][0][1][i], f[0]);
    const float x01 = probeLerp(corner[0][1][0][i], corner[0][1][1][i], f[0]);
    const float x10 = probeLerp(corner[1][0][0][i], corner[1][0][1][i], f[0]);
    const float x11 = probeLerp(corner[1][1][0][i], corner[1][1][1][i], f[0]);
    const float y0 = probeLerp(x00, x01, f[1]);
    const float y1 = probeLerp(x10, x11, f[1]);
    mixed[i] = probeLerp(y0, y1, f[2]);
  }
  probeShade(mixed, N[0], N[1], N[2], rgb);
}

}  // namespace qa
