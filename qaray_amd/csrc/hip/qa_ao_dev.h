// qa_ao_dev.h — ambient occlusion on the resident scene: how much of the hemisphere over a surface point is open within a radius,
// as a count of open rays.  This comment is the specification; tests/ao_util.py restates it in float32 numpy and
// tests/test_ao_host.py holds the host build of the functions below to that restatement bit for bit.
//
// All arithmetic is fp32 in the order written, nothing is contracted, `/` and sqrtf are the correctly rounded ones.  No trig, exp
// or pow is used.  Integers are uint32 and wrap.
//
// RANDOM WORDS.  The generator is counter-based: the direction of a ray depends on (seed, stream, counter) alone, not on the order
// in which rays are cast, on the kernel's shape or on what else a call holds.
//   mix(h)   the 32-bit finaliser of qa_pixel_rand (include/qa_seed.h):
//            h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
//   key    = mix(seed ^ stream * 0x9E3779B9)      stream: the pixel's stream id, y * image_width + x on the FULL image (the
//                                                 stream_ids of qa_camera_sample_rays_device); for the points form the point's
//                                                 index, or the caller's id
//   kr     = mix(key ^ mix(c + 0x632BE5AB))       c: the ray's counter
//   attempts a = 0 .. 7; for j = 0, 1:  w_j = mix(kr ^ (2 a + j + 1) * 0x9E3779B9)
//                                       x_j = (float) (w_j >> 8) * 2^-23 - 1          exact, in [-1, 1)
//
// A POINT ON THE SPHERE (Marsaglia).  q = x0 * x0 + x1 * x1; the first attempt with q < 1 is taken:
//   r = sqrtf(1 - q);  s = (2 * x0 * r, 2 * x1 * r, 1 - 2 * q)            (2 * x0 * r is (2 * x0) * r)
// If all eight attempts fail (about 4.5e-6 of the counters), s = (0, 0, 1).
//
// THE DIRECTION, cosine-weighted about the unit normal n:
//   v = n + s;  l2 = (v.x * v.x + v.y * v.y) + v.z * v.z
//   d = v / sqrtf(l2) componentwise if l2 > 1e-6f, else d = n
//
// THE FACING NORMAL OF A CAMERA HIT.  n = N if (N.x * d.x + N.y * d.y) + N.z * d.z <= 0, else -N: N is Hit::N as qa_cast_rays
// returns it, d the camera ray's direction.
//
// THE AO RAYS OF A HIT.  Origin Hit::p; directions of the counters c = s * K + k, k = 0 .. K - 1, s the sample's index; the test is
// shadow(ray, tmax) with tmax = min(radius, 1e30), the integrators' bias and walks, exactly as qa_occluded.  A ray is OPEN iff
// shadow returns non-zero (nothing is met at QA_BIAS < t < tmax).
//
// THE SAMPLES OF A PIXEL are qa_matte_region's camera rays (qa_kernel.h section B through qa_firsthit.h), indices
// first .. first + n - 1: n = spp, or with an ns plane n = min(max(ns[q] - first, 0), spp).  They are cast with the untextured
// traceClosest<RES, false, false>, as qa_cast_rays casts.  A camera with dof > 0.1 is refused (QA_EUNSUPPORTED), as the matte
// refuses it.
//
// PLANES, per pixel:
//   rays  uint32   hit samples * K
//   open  uint32   the open rays among them
//   ao    float    rays ? (float) open / (float) rays : 1.f
// A pixel with n = 0 writes 0, 0 and 1.
//
// POINTS FORM.  Point i takes its normal n_i as given (unit length is assumed), the counters c = first + k, k = 0 .. K - 1, and the
// stream i, or stream_ids[i] when given.  A void point - a component of the point or the normal that is not finite, or the normal
// (0, 0, 0) - is not walked and answers open = K, ao = 1 (void rays are not occluded).  ao = (float) open / (float) K.
//
// REFUSALS (QA_EINVAL): K == 0 or K > 256; (first + spp) * K (points: first + K) does not fit 32 bits; radius NaN or <= QA_BIAS
// (+inf is allowed and counts as 1e30); no output plane; for the points form the ray queries' rules for n.
//
// Every function here is compiled for the host too: qa_test_ao_*_host and the kernels of qa_ao.hip run the same source.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace qa {

#define QA_AO_ATTEMPTS 8u
#define QA_AO_GOLDEN 0x9E3779B9u
#define QA_AO_COUNTER_SALT 0x632BE5ABu
#define QA_AO_MAX_T 1e30f   /* QA_BIGFLOAT: what a closest-hit cast can see */

struct AoVec { float x, y, z; };

__host__ __device__ __forceinline__ uint32_t aoMix(uint32_t h)
{
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__host__ __device__ __forceinline__ uint32_t aoKey(uint32_t seed, uint32_t stream) { return aoMix(seed ^ stream * QA_AO_GOLDEN); }
__host__ __device__ __forceinline__ uint32_t aoRayKey(uint32_t key, uint32_t c) { return aoMix(key ^ aoMix(c + QA_AO_COUNTER_SALT)); }
// a word's top 24 bits as a float of [-1, 1): both steps are exact
__host__ __device__ __forceinline__ float aoSigned(uint32_t w) { return (float) (w >> 8) * 1.1920928955078125e-07f - 1.f; }

// the ray's point on the unit sphere; `fallback` tells that no attempt fell into the disc
__host__ __device__ __forceinline__ AoVec aoSphere(uint32_t kr, bool &fallback)
{
  AoVec s = {0.f, 0.f, 1.f};
  fallback = true;
  for (uint32_t a = 0; a < QA_AO_ATTEMPTS; ++a) {
    const float x0 = aoSigned(aoMix(kr ^ (2u * a + 1u) * QA_AO_GOLDEN));
    const float x1 = aoSigned(aoMix(kr ^ (2u * a + 2u) * QA_AO_GOLDEN));
    const float q = x0 * x0 + x1 * x1;
    if (q < 1.f) {
      const float r = sqrtf(1.f - q);
      s.x = 2.f * x0 * r;
      s.y = 2.f * x1 * r;
      s.z = 1.f - 2.f * q;
      fallback = false;
      break;
    }
  }
  return s;
}
// the direction about n from the sphere point s
__host__ __device__ __forceinline__ AoVec aoDirectionFrom(AoVec n, AoVec s)
{
  AoVec v = {n.x + s.x, n.y + s.y, n.z + s.z};
  const float l2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
  if (!(l2 > 1e-6f)) return n;
  const float l = sqrtf(l2);
  v.x = v.x / l;
  v.y = v.y / l;
  v.z = v.z / l;
  return v;
}
__host__ __device__ __forceinline__ AoVec aoDirection(uint32_t key, uint32_t c, AoVec n)
{
  bool fallback;
  return aoDirectionFrom(n, aoSphere(aoRayKey(key, c), fallback));
}
__host__ __device__ __forceinline__ AoVec aoFaceNormal(AoVec N, AoVec d)
{
  const float c = (N.x * d.x + N.y * d.y) + N.z * d.z;
  if (c <= 0.f) return N;
  const AoVec m = {-N.x, -N.y, -N.z};
  return m;
}
// a void point of the points form
__host__ __device__ __forceinline__ bool aoVoidPoint(AoVec p, AoVec n)
{
  const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(n.x) && isfinite(n.y) && isfinite(n.z);
  return !finite || (n.x == 0.f && n.y == 0.f && n.z == 0.f);
}
// the samples a pixel takes from `have` (spp, or its ns entry)
__host__ __device__ __forceinline__ uint32_t aoSamples(uint32_t have, uint32_t first, uint32_t spp)
{
  const uint32_t n = have > first ? have - first : 0u;
  return n < spp ? n : spp;
}
__host__ __device__ __forceinline__ float aoTmax(float radius) { return radius < QA_AO_MAX_T ? radius : QA_AO_MAX_T; }
__host__ __device__ __forceinline__ float aoValue(uint32_t open, uint32_t rays) { return rays ? (float) open / (float) rays : 1.f; }

}  // namespace qa
