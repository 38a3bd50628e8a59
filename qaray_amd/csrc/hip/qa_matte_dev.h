// qa_matte_dev.h — the matte planes of a pixel (coverage, albedo, normal, backdrop) reduced over the camera rays of ALL its
// samples, and the 8-bit straight-alpha RGBA made from them.  This comment is the specification; tests/matte_util.py restates it in
// float32 numpy and tests/test_matte_host.py holds the host build of the functions below to that restatement bit for bit.
//
// All arithmetic is fp32 in the order written, nothing is contracted, and `/` is the correctly rounded division.
//
// THE SAMPLES.  Sample s of pixel (px, py) is the camera ray qa_kernel.h section B builds for sample index s: the Halton pair of s
// (halton[2 s], halton[2 s + 1]) added to (px, py), the point (A + U x) + V y of the image plane, the direction normalised, and in
// textured scenes the two differential rays through x + QA_DX and y + QA_DX.  That is what qa_gbuffer casts for s = 0 and what
// qa_camera_sample_rays_device hands out.  It is cast with traceClosest<RES, TEX, false>, as qa_gbuffer casts.  A camera with depth
// of field (dof > 0.1) is refused (QA_EUNSUPPORTED), as qa_camera_sample_rays_device refuses it: its lens draws sit in the middle
// of the pixel's random stream.
//
// A pixel takes samples 0 .. n - 1: n = spp for every pixel, or, with an ns plane, n = min(ns[q], spp).  n = 0 writes 0 to every
// plane of that pixel.
//
// THE PLANES, per pixel and in sample order:
//   hits        the number of samples that hit.
//   coverage    (float) hits / (float) n.
//   albedo[3]   m = 0; then, for s = 0 .. n - 1, m = m + (x_s - m) / (float) (s + 1), where x_s is exactly the value qa_gbuffer
//               writes to its albedo plane for that ray: on a hit the diffuse colour section D would shade with (textured lookup
//               included; white or black where the hit has no material), on a miss the backdrop a camera ray returns (the
//               background colour, through its texture map in textured scenes).  This is section E's running mean
//               (qa_kernel_body.h: dc = (pL - mean) / inv; mean = mean + dc), so the plane IS the frame of the scene's
//               "emission := diffuse" twin at n samples and no bounce, bit for bit.
//   backdrop[3] the same rule with x_s = that backdrop colour on a miss and +0 on a hit: the part of a frame's colour that came
//               from camera rays which met nothing (the frame of the scene's "all black" twin).  rgb - backdrop is the premultiplied
//               foreground.
//   normal[3]   the running mean of h.N over the HIT samples only, by the same rule: the divisor counts hits, not samples.  0 when
//               no sample hits.  Not normalised: its length says how much the samples agree.
// With spp = 1 and no ns plane, albedo and normal are qa_gbuffer's bits, coverage is 0 or 1, backdrop is the albedo on a miss and 0
// on a hit.
//
// THE RGBA PRODUCT (straight alpha, what PNG stores), per pixel from the frame's rgb, the backdrop and coverage planes and ns:
//   ns == 0 ........ bytes 0, 0, 0, 0
//   otherwise ...... a = coverage; per component f = rgb - backdrop, c = a > 0 ? f / a : 0;
//                    colour byte = displayColorByte(c, srgb), alpha byte = displayColorByte(a, false)
// The byte functions are qa_display_dev.h's, included here and not restated.  Non-finite inputs end where those functions send them:
// a NaN component (or NaN coverage, for which a > 0 is false: c = 0 and the alpha byte is displayColorByte(NaN) = 0) passes MIN and
// MAX and ends as byte 0; +inf clamps to 255 and -inf to 0 as any value out of [0, 1] does, inf - inf and inf / inf are NaNs: byte 0.
//
// Every function here is compiled for the host too: qa_test_matte_accumulate_host / qa_test_matte_rgba_host and the kernels of
// qa_matte.hip run the same source.
#pragma once
#include "qa_display_dev.h"

namespace qa {

// one step of the running mean: the mean of k values from the mean m of the first k - 1 and the k-th value x
__host__ __device__ __forceinline__ float matteMeanStep(float m, float x, float k) { return m + (x - m) / k; }

// What a lane carries through its sample loop: ten floats' worth of state
struct MatteAcc {
  float albedo[3], backdrop[3], normal[3];
  uint32_t hits;
};
__host__ __device__ __forceinline__ MatteAcc matteAccInit()
{
  MatteAcc a;
  for (int k = 0; k < 3; ++k) a.albedo[k] = a.backdrop[k] = a.normal[k] = 0.f;
  a.hits = 0u;
  return a;
}
// sample s (0-based): x = the value qa_gbuffer's albedo plane would hold for the ray, N = the hit's normal (read on a hit only)
__host__ __device__ __forceinline__ void matteAccSample(MatteAcc &a, uint32_t s, bool hit, float x0, float x1, float x2, float n0, float n1, float n2)
{
  const float k = (float) (s + 1u);
  a.albedo[0] = matteMeanStep(a.albedo[0], x0, k);
  a.albedo[1] = matteMeanStep(a.albedo[1], x1, k);
  a.albedo[2] = matteMeanStep(a.albedo[2], x2, k);
  a.backdrop[0] = matteMeanStep(a.backdrop[0], hit ? 0.f : x0, k);
  a.backdrop[1] = matteMeanStep(a.backdrop[1], hit ? 0.f : x1, k);
  a.backdrop[2] = matteMeanStep(a.backdrop[2], hit ? 0.f : x2, k);
  if (hit) {
    a.hits += 1u;
    const float kh = (float) a.hits;
    a.normal[0] = matteMeanStep(a.normal[0], n0, kh);
    a.normal[1] = matteMeanStep(a.normal[1], n1, kh);
    a.normal[2] = matteMeanStep(a.normal[2], n2, kh);
  }
}
// n = 0 has no samples: 0, like every other plane of that pixel
__host__ __device__ __forceinline__ float matteCoverage(uint32_t hits, uint32_t n) { return n ? (float) hits / (float) n : 0.f; }
// the samples a pixel takes
__host__ __device__ __forceinline__ uint32_t matteSamples(uint32_t ns, uint32_t spp) { return ns < spp ? ns : spp; }

struct MatteRgba {
  uint8_t r, g, b, a;
};
__host__ __device__ __forceinline__ float matteStraight(float rgb, float backdrop, float a)
{
  const float f = rgb - backdrop;
  return a > 0.f ? f / a : 0.f;
}
__host__ __device__ __forceinline__ MatteRgba matteRgbaEncode(float r, float g, float b, float br, float bg, float bb, float a, uint32_t ns, bool useSRGB)
{
  MatteRgba o;
  o.r = o.g = o.b = o.a = 0;
  if (ns == 0u) return o;
  o.r = displayColorByte(matteStraight(r, br, a), useSRGB);
  o.g = displayColorByte(matteStraight(g, bg, a), useSRGB);
  o.b = displayColorByte(matteStraight(b, bb, a), useSRGB);
  o.a = displayColorByte(a, false);
  return o;
}

}  // namespace qa
