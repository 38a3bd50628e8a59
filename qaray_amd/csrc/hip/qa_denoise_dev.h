// qa_denoise_dev.h — an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) for a frame of float results, guided by the
// frame's own colour and by sample 0's hit distance.  No reference counterpart: the reference shows its previews unfiltered.
// Every function here is compiled for the host too: qa_test_denoise_host and the kernels of qa_denoise.hip run the same source
// (tests/test_gpu_denoise.py: equal bit for bit); tests/denoise_util.py restates THIS COMMENT in float64 numpy.
//
// SPECIFICATION.  All arithmetic is fp32 in the order written, without contraction; / and sqrtf are correctly rounded; exp is qexpf.
//
// Input: W x H pixels, row-major: rgb[3], depth, ns.   Parameters: iterations 0 .. 6, sigma_color, sigma_depth (finite, > 0), flags 0.
// Defaults: iterations 5, sigma_color 4, sigma_depth 1  (chosen on the 4-spp box frame of tests/test_denoise_host.py: DESIGN 4g).
//
// Classes.   VOID: ns == 0, or a colour component or the depth is not finite.  (The depth is an addition to the rule for the
//                  colours: no frame of the renderer holds such a depth, and with it every weight below is a number.)
//            MISS: not void and depth == 1e30.       HIT: everything else.
// A void pixel weighs 0 as a neighbour and its output is its input's bits.  Two pixels of different classes weigh 0 for each other.
// iterations == 0: the output is the input's bits.
//
// luma(c) = 0.2126f * r + 0.7152f * g + 0.0722f * b, summed left to right (the reference's ColorLuma).
//
// Pass 0, per non-void pixel p -> colour c_p, var_p, slope_p:
//   members = the pixels of the 3x3 window around p that lie in the image, are not void and have p's class (p is one), visited
//             row-major; n = their number.
//   mean = (sum of luma over the members) / n;   var_p = n > 1 ? (sum of (luma - mean)^2 over the members) / n : 0
//             (the biased variance in its two-pass form: never negative, and 0 on a constant window whatever its level)
//   slope_p (hit pixels; 0 for a miss): per axis, the differences |z_p - z_n| to the two neighbours on that axis that lie in the
//             image and are hit pixels; the axis gives the SMALLER of the two, the one there is when there is only one, else 0.
//             slope_p = max(max(axis x, axis y), 1e-3f * |z_p|).
//             (On a slanted plane both differences of an axis agree and this is the largest over the 4-neighbours.  At a depth step
//             the largest would be the step itself, which would then weigh e^(-1 / sigma_depth) for the pixels on its edge; the
//             smaller one is the slope of the surface p lies on.)
//
// Iteration i = 0 .. iterations - 1, step s = 1 << i, per non-void pixel p, from the colours and variances of iteration i - 1
// (pass 0 for i = 0); slope, depth and class stay pass 0's:
//   l_p = luma(c_p);   den_l = sigma_color * sqrtf(var_p) + 1e-4f;   den_z = sigma_depth * slope_p * (float) s
//   the 25 taps q = p + s * (dx, dy), dx, dy in -2 .. 2, row-major in (dy, dx); a tap outside the image, a void tap and a tap of
//   the other class are skipped.  h = (1/16, 1/4, 3/8, 1/4, 1/16); k = max(|dx|, |dy|).
//     centre tap: w = 9/64
//     else        e = |l_p - luma(c_q)| / den_l;   hit pixels with z_p != z_q: e = e + |z_p - z_q| / (den_z * (float) k)
//                 w = (h[dx + 2] * h[dy + 2]) * qexpf(-e)         (one exponential for w_z * w_l)
//     sw += w;   sc += w * (c_q - c_p) per component;   sv += (w * w) * var_q
//   c'_p = c_p + sc / sw   (= sum(w c_q) / sum(w), written around the centre: a constant neighbourhood stays constant exactly)
//   var'_p = sv / (sw * sw)
// The output is the colour after the last iteration.  sw >= 9/64: no division by zero.
//
// GUIDED FORM (qa_denoise_guided_*; tests/denoise_guided_util.py restates this section).  Two more inputs per pixel, each optional
// (flags QA_DENOISE_GUIDE_NORMAL = 1, QA_DENOISE_GUIDE_ALBEDO = 2): normal[3] and albedo[3], the planes of qa_gbuffer_region*.  One more
// parameter, sigma_normal (finite, > 0; default 0.1).  With flags == 0 it is the filter above, bit for bit.  Classes, void rules,
// pass 0, the centre-form update and the variance recursion are unchanged; the colours are never divided or multiplied by a guide
// (DESIGN 4g has the measurements that ruled demodulation out), so iterations == 0 is the input's bits here too.  The guides add
// terms to the exponent e of a tap, in the one qexpf.
//   A guide is sample 0's: on a pixel whose footprint holds an edge (of geometry, of a texture) it describes one side only, while the
//   colour is the mean over both.  Such a pixel must not be tied to sample 0's side, so it is filtered as if it had no guides:
//   valid_n(p): the flag is set, p is a hit pixel, the normal's components are finite and not all 0.
//   valid_a(p): the flag is set and the albedo's components are finite.         (p not void, for both)
//   dn(p, q) = 1 - (n_p.x * n_q.x + n_p.y * n_q.y + n_p.z * n_q.z);  da(p, q) = max(max(|a_p.r - a_q.r|, |a_p.g - a_q.g|), |a_p.b - a_q.b|)
//   members = the pixels of the 3x3 window around p that lie in the image and are not void (p is one), of EITHER class.
//   reliable(p): no member has the other class; every member q with valid_n(p) and valid_n(q) has dn(p, q) <= 0.02f; every member q
//                with valid_a(p) and valid_a(q) has da(p, q) <= 0.3f.
//   (0.02: 11.5 degrees, what a curved surface turns between neighbouring pixels at preview sizes and no crease does; 0.3: a third of
//   the albedo range, the step of a painted edge and more than a filtered texture varies between neighbours.)
// A tap q of pixel p that is not skipped, after the depth term, in this order:
//   reliable(p) and valid_n(p) and valid_n(q) and dn(p, q) > 0:   e = e + dn(p, q) / sigma_normal
//   reliable(p) and valid_a(p) and valid_a(q):                    e = e + da(p, q) / 0.02f
// (It is the centre that is gated: an unreliable q still counts for a reliable p, at the distance its sample 0 gives it.)
//
// VARIANCE FORM (qa_denoise_variance_*; tests/denoise_variance_util.py restates this section).  One more input per pixel, optional
// (flag QA_DENOISE_GUIDE_VARIANCE = 4, beside the two guide flags): variance[1], an estimate of the variance of the pixel's luma
// that the caller brings - the out_variance plane of qa_reproject_moments_dev.h, which knows from the frames behind a pixel what no
// window of one frame can tell: texture detail on a converged surface from Monte-Carlo noise.  One more parameter, variance_scale
// (finite, > 0; default 4: DESIGN 4k has the sweep), which reconciles that estimate's scale with the sigma_color tuned on the spatial
// one.  With the flag clear it is the guided form, bit for bit, and so it is with a plane that holds -1 everywhere.  Only pass 0
// changes; the iterations, the variance recursion, the classes, the void rules and the guides' gating are unchanged.
//   trusted(q): q is not void and its variance t_q is finite and >= 0.    (A negative value, one that is not a number and an
//               infinite one all say "none".)
//   Pass 0 computes var_p as above.  For a trusted p it is then replaced:
//     members = the pixels of the 3x3 window around p that lie in the image, are not void, have p's class and are trusted (p is
//               one), visited row-major; w = (1, 2, 1) x (1, 2, 1): 4 for p, 2 for its edge neighbours, 1 for the corners.
//     sw += w;  st += w * t_q     (both from 0);          var_p = variance_scale * (st / sw)
//   (The 3x3 prefilter that SVGF applies to its variance: an estimate from a handful of 4-spp frames is itself noisy.  A trusted p
//   alone in its window takes variance_scale * t_p exactly.)  Every other pixel keeps the spatial estimate.
// What it does not do: the plane is of the luma only; it is read by pass 0 and never updated by anything but the recursion; the
// progressive variants have no such form (a viewer filters the accumulated plain buffers of hip.TemporalPreview).
#pragma once
#include "qa_device_math.h"

namespace qa {

#define QA_DENOISE_MISS 1.0e30f
#define QA_DENOISE_MAX_ITERATIONS 6
#define QA_DENOISE_DEFAULT_ITERATIONS 5
#define QA_DENOISE_DEFAULT_SIGMA_COLOR 4.0f
#define QA_DENOISE_DEFAULT_SIGMA_DEPTH 1.0f
#define QA_DENOISE_DEFAULT_SIGMA_NORMAL 0.1f
#define QA_DENOISE_DEFAULT_VARIANCE_SCALE 4.0f
#define QA_DENOISE_RELIABLE_NORMAL 0.02f
#define QA_DENOISE_RELIABLE_ALBEDO 0.3f
#define QA_DENOISE_SIGMA_ALBEDO 0.02f
#define QA_DENOISE_AUX_VALID_N 1u
#define QA_DENOISE_AUX_VALID_A 2u
#define QA_DENOISE_AUX_RELIABLE 4u

struct DenoisePixel {
  float r, g, b, z;
  uint32_t ns;
};
// what the iterations work on.  Colour plane: r, g, b, variance.  Guide plane: depth and slope; slope < 0 marks a void pixel
struct DenoiseColor { float r, g, b, var; };
struct DenoiseGuide { float z, slope; };
// the guided form's plane: normal, albedo and the QA_DENOISE_AUX_* bits of the pixel
struct DenoiseAux { float nx, ny, nz; uint32_t bits; float ar, ag, ab, pad; };

__host__ __device__ __forceinline__ bool denoiseFinite(float x) { return (qa_asuint(x) & 0x7f800000u) != 0x7f800000u; }
__host__ __device__ __forceinline__ bool denoiseVoid(const DenoisePixel &p)
{
  return p.ns == 0u || !denoiseFinite(p.r) || !denoiseFinite(p.g) || !denoiseFinite(p.b) || !denoiseFinite(p.z);
}
__host__ __device__ __forceinline__ float denoiseLuma(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// Pass 0 of pixel (x, y).  src(x, y) -> DenoisePixel, called for pixels inside the image only
template <class Src>
__host__ __device__ __forceinline__ void denoiseGuide(const Src &src, int x, int y, int W, int H, DenoiseColor &c, DenoiseGuide &g)
{
  const DenoisePixel p = src(x, y);
  c.r = p.r; c.g = p.g; c.b = p.b; c.var = 0.f;
  g.z = 0.f; g.slope = -1.f;
  if (denoiseVoid(p)) return;
  const bool miss = p.z == QA_DENOISE_MISS;
  float l[9];
  int n = 0;
  float sum = 0.f;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      const DenoisePixel q = src(qx, qy);
      if (denoiseVoid(q) || (q.z == QA_DENOISE_MISS) != miss) continue;
      l[n] = denoiseLuma(q.r, q.g, q.b);
      sum += l[n];
      ++n;
    }
  if (n > 1) {
    const float mean = sum / (float) n;
    float dev = 0.f;
    for (int k = 0; k < n; ++k) dev += (l[k] - mean) * (l[k] - mean);
    c.var = dev / (float) n;
  }
  g.z = p.z; g.slope = 0.f;
  if (miss) return;
  float slope = 0.f;
  for (int axis = 0; axis < 2; ++axis) {
    float d = 0.f;
    bool have = false;
    for (int side = -1; side <= 1; side += 2) {
      const int qx = axis ? x : x + side, qy = axis ? y + side : y;
      if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      const DenoisePixel q = src(qx, qy);
      if (denoiseVoid(q) || q.z == QA_DENOISE_MISS) continue;
      const float dz = qabs(p.z - q.z);
      d = have ? qmin(d, dz) : dz;
      have = true;
    }
    slope = qmax(slope, d);
  }
  g.slope = qmax(slope, 1e-3f * qabs(p.z));
}

// Pass 0 of the variance form for pixel (x, y): denoiseGuide, then the prefiltered estimate of the caller's plane in var's place where
// the pixel is trusted.  vsrc(x, y) -> the plane's value, called for pixels inside the image only
__host__ __device__ __forceinline__ bool denoiseTrusted(float t) { return denoiseFinite(t) && t >= 0.f; }
template <class Src, class VSrc>
__host__ __device__ __forceinline__ void denoiseGuideVariance(const Src &src, const VSrc &vsrc, float varianceScale, int x, int y, int W, int H,
                                                              DenoiseColor &c, DenoiseGuide &g)
{
  denoiseGuide(src, x, y, W, H, c, g);
  if (g.slope < 0.f || !denoiseTrusted(vsrc(x, y))) return;
  const bool miss = g.z == QA_DENOISE_MISS;
  float sw = 0.f, st = 0.f;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      const DenoisePixel q = src(qx, qy);
      if (denoiseVoid(q) || (q.z == QA_DENOISE_MISS) != miss) continue;
      const float t = vsrc(qx, qy);
      if (!denoiseTrusted(t)) continue;
      const float w = (dx == 0 ? 2.f : 1.f) * (dy == 0 ? 2.f : 1.f);
      sw += w;
      st += w * t;
    }
  c.var = varianceScale * (st / sw);
}

// ---- the guided form: its pass 0 (the aux plane) ----
__host__ __device__ __forceinline__ float denoiseDn(const DenoiseAux &p, const DenoiseAux &q) { return 1.f - (p.nx * q.nx + p.ny * q.ny + p.nz * q.nz); }
__host__ __device__ __forceinline__ float denoiseDa(const DenoiseAux &p, const DenoiseAux &q)
{
  return qmax(qmax(qabs(p.ar - q.ar), qabs(p.ag - q.ag)), qabs(p.ab - q.ab));
}

// The guides of one pixel and its valid bits.  gsrc(x, y, n, a) fetches normal and albedo (three floats each; a plane that is not
// given is left alone), called for pixels inside the image only; px is the pixel's colour / depth / ns
template <class GSrc>
__host__ __device__ __forceinline__ DenoiseAux denoiseAuxLoad(const GSrc &gsrc, const DenoisePixel &px, int x, int y, uint32_t flags)
{
  float n[3] = {0.f, 0.f, 0.f}, a[3] = {0.f, 0.f, 0.f};
  gsrc(x, y, n, a);
  DenoiseAux o;
  o.nx = n[0]; o.ny = n[1]; o.nz = n[2]; o.ar = a[0]; o.ag = a[1]; o.ab = a[2]; o.pad = 0.f;
  o.bits = 0u;
  if (denoiseVoid(px)) return o;
  if ((flags & 1u) && px.z != QA_DENOISE_MISS && denoiseFinite(n[0]) && denoiseFinite(n[1]) && denoiseFinite(n[2]) &&
      (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f))
    o.bits |= QA_DENOISE_AUX_VALID_N;
  if ((flags & 2u) && denoiseFinite(a[0]) && denoiseFinite(a[1]) && denoiseFinite(a[2])) o.bits |= QA_DENOISE_AUX_VALID_A;
  return o;
}

// Pass 0 of the guided form for pixel (x, y): its guides, valid bits and whether it is reliable
template <class Src, class GSrc>
__host__ __device__ __forceinline__ DenoiseAux denoiseAux(const Src &src, const GSrc &gsrc, int x, int y, int W, int H, uint32_t flags)
{
  const DenoisePixel p = src(x, y);
  DenoiseAux P = denoiseAuxLoad(gsrc, p, x, y, flags);
  if (denoiseVoid(p)) return P;
  const bool miss = p.z == QA_DENOISE_MISS;
  bool reliable = true;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      const DenoisePixel q = src(qx, qy);
      if (denoiseVoid(q)) continue;
      if ((q.z == QA_DENOISE_MISS) != miss) { reliable = false; continue; }
      const DenoiseAux Q = denoiseAuxLoad(gsrc, q, qx, qy, flags);
      if ((P.bits & Q.bits & QA_DENOISE_AUX_VALID_N) && !(denoiseDn(P, Q) <= QA_DENOISE_RELIABLE_NORMAL)) reliable = false;
      if ((P.bits & Q.bits & QA_DENOISE_AUX_VALID_A) && !(denoiseDa(P, Q) <= QA_DENOISE_RELIABLE_ALBEDO)) reliable = false;
    }
  if (reliable) P.bits |= QA_DENOISE_AUX_RELIABLE;
  return P;
}

// ---- the iterations of every form ----
// the aux argument of the forms without guides: never called
struct DenoiseNoAux {};

// One iteration of pixel (x, y) at step s.  tap(x, y, c, g) fetches a pixel's planes, called for pixels inside the image only.
// GUIDED: aux(x, y) -> DenoiseAux of a pixel inside the image, and its guides add their terms to a tap's exponent
template <bool GUIDED, class Tap, class Aux>
__host__ __device__ __forceinline__ DenoiseColor denoiseIterate(const Tap &tap, const Aux &aux, int x, int y, int W, int H, int s, float sigmaColor,
                                                                float sigmaDepth, float sigmaNormal)
{
  DenoiseColor P;
  DenoiseGuide GP;
  tap(x, y, P, GP);
  if (GP.slope < 0.f) return P;
  [[maybe_unused]] DenoiseAux AP;
  [[maybe_unused]] uint32_t guided = 0u;
  if constexpr (GUIDED) {
    AP = aux(x, y);
    guided = (AP.bits & QA_DENOISE_AUX_RELIABLE) ? AP.bits : 0u;
  }
  const bool miss = GP.z == QA_DENOISE_MISS;
  const float lp = denoiseLuma(P.r, P.g, P.b);
  const float denL = sigmaColor * qsqrt(P.var) + 1e-4f;
  const float denZ = sigmaDepth * GP.slope * (float) s;
  const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) {
        const float w = 0.140625f;
        sw += w; sv += (w * w) * P.var;
        continue;
      }
      const int qx = x + s * dx, qy = y + s * dy;
      if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
      DenoiseColor Q;
      DenoiseGuide GQ;
      tap(qx, qy, Q, GQ);
      if (GQ.slope < 0.f || (GQ.z == QA_DENOISE_MISS) != miss) continue;
      float e = qabs(lp - denoiseLuma(Q.r, Q.g, Q.b)) / denL;
      if (!miss && GP.z != GQ.z) {
        const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
        e = e + qabs(GP.z - GQ.z) / (denZ * (float) (ax > ay ? ax : ay));
      }
      if constexpr (GUIDED) {
        if (guided & (QA_DENOISE_AUX_VALID_N | QA_DENOISE_AUX_VALID_A)) {
          const DenoiseAux AQ = aux(qx, qy);
          if (guided & AQ.bits & QA_DENOISE_AUX_VALID_N) {
            const float dn = denoiseDn(AP, AQ);
            if (dn > 0.f) e = e + dn / sigmaNormal;
          }
          if (guided & AQ.bits & QA_DENOISE_AUX_VALID_A) e = e + denoiseDa(AP, AQ) / QA_DENOISE_SIGMA_ALBEDO;
        }
      }
      const float w = (h[dx + 2] * h[dy + 2]) * qexpf(-e);
      sw += w;
      sr += w * (Q.r - P.r); sg += w * (Q.g - P.g); sb += w * (Q.b - P.b);
      sv += (w * w) * Q.var;
    }
  }
  DenoiseColor o;
  o.r = P.r + sr / sw; o.g = P.g + sg / sw; o.b = P.b + sb / sw;
  o.var = sv / (sw * sw);
  return o;
}

}  // namespace qa
