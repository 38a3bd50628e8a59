// qa_probevis_dev.h — visibility between a shading point and the probes of its grid cell: the distances a probe's rays travelled,
// kept as two moments per direction cell, and a grid shading that weighs each of the cell's eight probes by whether it can see the
// point - the Chebyshev test of Majercik et al. 2019, "Dynamic Diffuse Global Illumination with Ray-Traced Irradiance Fields".  This
// comment is the specification; tests/probevis_util.py restates it in float32 numpy and tests/test_probevis_host.py holds the host
// build of the functions below to that restatement bit for bit.
//
// All arithmetic is fp32 in the order written, nothing is contracted, `/` and sqrtf are the correctly rounded ones.  The directions,
// the grid's axis function, probeShade, probeGridShade and probeVoid are qa_lightprobe_dev.h's: used from that header, not restated.
//
// MOMENTS.  A probe of resolution m (its K = 6 m^2 rays are DIRECTIONS' records, t_k their hit parameters - distances, the directions
// being unit vectors; 1e30 on a miss; with QA_PROBE_JITTER the texel's ray is the jittered one) gets a cube map of d x d cells per
// face, 1 <= d <= m and m % d == 0; r = m / d.  Cell (f, B, C) pools the r^2 texels (f, b, c) with b / r == B and c / r == C.  One
// thread owns one cell and visits its texels with b ascending, then c ascending (b outer); s = s2 = +0 at the start, per texel
//   x = (t < dmax) ? t : dmax                  (a miss, and a t that is NaN, become dmax; dmax > 0 and finite)
//   s = s + x                                  s2 = s2 + (x * x)
// and the cell stores  mean = s / (float) (r * r),  mean2 = s2 / (float) (r * r).  The layout is [n][6][d][d][2] floats (mean, then
// mean2).  A void probe stores +0 in both: in the shading below it ends up weighing only the floor.
//
// THE CELL A VECTOR POINTS INTO, the inverse of DIRECTIONS, for v = (v0, v1, v2) with a component that is not 0:
//   axis a = argmax |v_a|, the lowest a on ties;  m_a = |v_a|;  face f = 2 a + (v_a < 0 ? 1 : 0),  s = +1.f for even f, -1.f for odd
//   u = v[(a + 1) % 3] / m_a                   w = (s * v[(a + 2) % 3]) / m_a
//   gu = ((u + 1.f) * 0.5f) * (float) d        column = (gu < (float) d) ? (int) gu : d - 1        (so a NaN takes d - 1)
//   gw = ((w + 1.f) * 0.5f) * (float) d        row    = (gw < (float) d) ? (int) gw : d - 1
//   cell = (f * d + row) * d + column          (u and w lie in [-1, 1]: for finite v this is min((int) g, d - 1))
//
// VISIBILITY SHADING of the unit normal N at point P from the grid (origin, spacing, counts), its coefficients sh [probes][27] and
// its moments [probes][6][d][d][2], with the caller's normal_bias.  If P or N has a component that is not finite the result is
// (0, 0, 0).  i0, i1 and f of every axis e are probeGridAxis's.  The biased point is  b_e = P_e + (normal_bias * N_e).  For the eight
// corners j = cz * 4 + cy * 2 + cx, ascending, with c_e the corner's bit on axis e:
//   idx_e = c_e ? i1_e : i0_e                  w_e = c_e ? f_e : 1.f - f_e                tri = (w_x * w_y) * w_z
//   Q_e = origin_e + (float) idx_e * spacing_e v_e = b_e - Q_e
//   r2 = (v0 * v0 + v1 * v1) + v2 * v2         rr = sqrtf(r2)
//   if rr == 0:  vis = 1, wrap = 1
//   else, with (mean, mean2) of the cell v points into, of probe (idx_z * ny + idx_y) * nx + idx_x:
//     var = fabsf(mean2 - mean * mean)
//     dd = rr - mean                           cheb = (rr <= mean) ? 1.f : var / (var + dd * dd)
//     cheb = (cheb * cheb) * cheb              vis = (cheb > 0.05f) ? cheb : 0.05f          (a NaN takes the floor)
//     e_k = (-v_k) / rr                        h = (((e0 * N0 + e1 * N1) + e2 * N2) + 1.f) * 0.5f
//     wrap = h * h + 0.2f
//   w_j = (tri * wrap) * vis
// W = +0, then W = W + w_j for j ascending.  The two floors and sum(tri) = 1 make W > 0 for finite input; if W is nevertheless not
// a positive finite number (the biased point overflowed), the result is probeGridShade's.  Otherwise every one of the 27 coefficients
// starts at +0 and takes  c_i = c_i + ((w_j / W) * sh_j[i])  for j ascending, and the result is probeShade of them.
//
// Two consequences.  A point on a probe (normal_bias 0) has tri = 1 for one corner and 0 for the others: it takes that probe's
// coefficients exactly (x / x == 1, the other terms are 0 * finite) and so that probe's shading, bit for bit.  The sum runs probe by
// probe over 27 accumulators: the eight corner sets of probeGridShade are never held at once.
//
// The constants 0.05 and 0.2 and the cube are the paper's and part of this specification; d, dmax and normal_bias are the caller's.
// Limits: the nearest cell is used, nothing is filtered across cell or face borders; a probe inside geometry is still the caller's
// to move (hits and tmin show it); there is no view-direction bias.
//
// Every function here is compiled for the host too: qa_test_probevis_*_host and the kernels of qa_lightprobe.hip run the same source.
#pragma once
#include "qa_lightprobe_dev.h"

namespace qa {

#define QA_PROBEVIS_FLOOR 0.05f
#define QA_PROBEVIS_WRAP 0.2f

// the two moments of cell `cell` (of 6 d^2) of one probe from its K hit parameters t
__host__ __device__ __forceinline__ void probeVisMoments(uint32_t m, uint32_t d, float dmax, const float *t, uint32_t cell, float out[2])
{
  const uint32_t r = m / d, f = cell / (d * d), B = (cell % (d * d)) / d, C = cell % d;
  float s = 0.f, s2 = 0.f;
  for (uint32_t b = B * r; b < B * r + r; ++b)
    for (uint32_t c = C * r; c < C * r + r; ++c) {
      const float tk = t[(f * m + b) * m + c];
      const float x = (tk < dmax) ? tk : dmax;
      s = s + x;
      s2 = s2 + (x * x);
    }
  const float count = (float) (r * r);
  out[0] = s / count;
  out[1] = s2 / count;
}

// the cell of a cube map of d x d cells per face that v points into
__host__ __device__ __forceinline__ uint32_t probeVisCell(const float v[3], int d)
{
  const float m0 = fabsf(v[0]), m1 = fabsf(v[1]), m2 = fabsf(v[2]);
  int a = 0;
  float ma = m0;
  if (m1 > ma) { a = 1; ma = m1; }
  if (m2 > ma) { a = 2; ma = m2; }
  const float va = a == 0 ? v[0] : a == 1 ? v[1] : v[2];
  const float vu = a == 0 ? v[1] : a == 1 ? v[2] : v[0];
  const float vw = a == 0 ? v[2] : a == 1 ? v[0] : v[1];
  const bool neg = va < 0.f;
  const float s = neg ? -1.f : 1.f;
  const float u = vu / ma, w = (s * vw) / ma;
  const float fd = (float) d;
  const float gu = ((u + 1.f) * 0.5f) * fd, gw = ((w + 1.f) * 0.5f) * fd;
  const int column = (gu < fd) ? (int) gu : d - 1;
  const int row = (gw < fd) ? (int) gw : d - 1;
  return (uint32_t) (((2 * a + (neg ? 1 : 0)) * d + row) * d + column);
}

// the weight of one corner's probe beside its trilinear weight: wrap * vis is folded in by the caller in the order of the specification
__host__ __device__ __forceinline__ float probeVisWeight(float tri, const float v[3], const float N[3], const float *probeMoments, int d)
{
  const float r2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  const float rr = sqrtf(r2);
  float vis = 1.f, wrap = 1.f;
  if (!(rr == 0.f)) {
    const float *mo = probeMoments + 2 * (size_t) probeVisCell(v, d);
    const float mean = mo[0], mean2 = mo[1];
    const float var = fabsf(mean2 - mean * mean);
    const float dd = rr - mean;
    float cheb = (rr <= mean) ? 1.f : var / (var + dd * dd);
    cheb = (cheb * cheb) * cheb;
    vis = (cheb > QA_PROBEVIS_FLOOR) ? cheb : QA_PROBEVIS_FLOOR;
    const float e0 = (-v[0]) / rr, e1 = (-v[1]) / rr, e2 = (-v[2]) / rr;
    const float h = (((e0 * N[0] + e1 * N[1]) + e2 * N[2]) + 1.f) * 0.5f;
    wrap = h * h + QA_PROBEVIS_WRAP;
  }
  return (tri * wrap) * vis;
}

// the shading of normal N at point P from the grid's coefficients sh [probes][27] and moments [probes][6][d][d][2]
__host__ __device__ __forceinline__ void probeVisGridShade(const ProbeGrid &G, const float *sh, const float *moments, int d, float normal_bias,
                                                           const float P[3], const float N[3], float rgb[3])
{
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (probeVoid(P[0], P[1], P[2]) || probeVoid(N[0], N[1], N[2])) return;
  int i0[3], i1[3];
  float f[3], biased[3];
  for (int e = 0; e < 3; ++e) {
    probeGridAxis(P[e], G.origin[e], G.spacing[e], G.counts[e], i0[e], i1[e], f[e]);
    biased[e] = P[e] + (normal_bias * N[e]);
  }
  const int64_t nx = G.counts[0], ny = G.counts[1];
  const size_t perProbe = (size_t) 12 * d * d;
  float w[8], W = 0.f;
  int64_t probe[8];
  for (int j = 0; j < 8; ++j) {
    int idx[3];
    float we[3], v[3];
    for (int e = 0; e < 3; ++e) {
      const bool far = (j >> e) & 1;
      idx[e] = far ? i1[e] : i0[e];
      we[e] = far ? f[e] : 1.f - f[e];
      const float Q = G.origin[e] + (float) idx[e] * G.spacing[e];
      v[e] = biased[e] - Q;
    }
    probe[j] = ((int64_t) idx[2] * ny + idx[1]) * nx + idx[0];
    const float tri = (we[0] * we[1]) * we[2];
    w[j] = probeVisWeight(tri, v, N, moments + perProbe * (size_t) probe[j], d);
    W = W + w[j];
  }
  if (!(W > 0.f && isfinite(W))) {
    probeGridShade(G, sh, P, N, rgb);
    return;
  }
  float mixed[27];
  for (int i = 0; i < 27; ++i) mixed[i] = 0.f;
  for (int j = 0; j < 8; ++j) {
    const float k = w[j] / W;
    const float *c = sh + 27 * probe[j];
    for (int i = 0; i < 27; ++i) mixed[i] = mixed[i] + (k * c[i]);
#if defined(__HIP_DEVICE_COMPILE__)
    // probe by probe: without the fence the scheduler loads all eight coefficient sets ahead of the sums (260 registers)
    __builtin_amdgcn_sched_barrier(0);
#endif
  }
  probeShade(mixed, N[0], N[1], N[2], rgb);
}

}  // namespace qa
