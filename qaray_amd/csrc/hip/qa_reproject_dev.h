// qa_reproject_dev.h — temporal reprojection: the accumulated frame of an EARLIER camera (the history) carried into the frame just
// rendered from the camera as it now stands, so that a camera move keeps the samples of every surface point both cameras see.  No
// reference counterpart: the reference renders every frame from nothing.  Every function here is compiled for the host too:
// qa_test_reproject_host and the kernel of qa_reproject.hip run the same source (tests/test_gpu_reproject.py: equal bit for bit);
// tests/reproject_util.py restates THIS COMMENT in float64 numpy.  The steps below are this header's functions; the pixel that
// runs them, for this form and the two that extend it, is reprojectPixel<FORM> of qa_reproject_moments_dev.h (this form: FORM 0).
//
// SPECIFICATION.  All arithmetic is fp32 in the order written, without contraction; / and sqrtf are correctly rounded.  Vector
// operations are those of qa_device_math.h: dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z summed left to right, cross as glm's,
// normalize(v) = v * (1 / sqrtf(dot(v, v))), |v| = sqrtf(dot(v, v)).
//
// Both frames cover the region (x0, y0, W, H) of the image, row-major.
// Current frame (camera C1): rgb[3], depth, ns, optional ids[2].      History (camera C0): rgb[3], depth, length, optional ids[2].
// length is the effective sample count behind a history pixel; a pixel whose length is not > 0 holds no history.  The ids are
// compared only when both planes are given.  A camera is the 76-byte qa_camera record: A = screenA, U = screenU, V = screenV,
// pos = cam_pos; screenX, screenY and dof take part in the still-camera comparison only.
// Parameters: depth_tolerance (finite, >= 0; default 0.05), max_history (finite, > 0; default 64 samples), flags 0.
// Outputs: out_rgb[3] and out_length.  The caller keeps the current frame's depth and ids as the next frame's history planes.
//
// Per pixel (px, py) = (x0 + tx, y0 + ty), with colour c, depth z, n = (float) ns:
//
// 1. Classes, as in qa_denoise_dev.h.  VOID: ns == 0, or a colour component or the depth is not finite: the output is the input's
//    bits and out_length = 0.  MISS: not void and depth == 1e30.  HIT: everything else.
// 2. The camera ray of sample 0 under C1, as qa_gbuffer.hip builds it (its Halton offset is 0):
//      d = normalize(((A1 + U1 * (float) px) + V1 * (float) py) - pos1)
//    hit:  P = pos1 + d * z;   w = P - pos0          miss:  w = d   (the backdrop is reprojected by direction)
// 3. Projection into C0, for any U0, V0 (they need not be perpendicular).  Per call:
//      a = A0 - pos0;  nrm = cross(U0, V0);  an = dot(a, nrm);  vn = cross(V0, nrm);  nu = cross(nrm, U0);  du = dot(U0, vn);  dv = dot(V0, nu)
//    per pixel:
//      wn = dot(w, nrm);  s = an / wn;  r = w * s - a;  u = dot(r, vn) / du;  v = dot(r, nu) / dv
//      ul = u - (float) x0;  vl = v - (float) y0        (region-local)          hit: z' = |w|, the depth C0 saw the point at
//    NO HISTORY when wn == 0; when s > 0 does not hold (the point lies behind C0, or s is not a number); when ul or vl is not
//    finite; when -1 <= ul < W and -1 <= vl < H does not hold; for a hit, when z' is not finite (|w|^2 overflows from |w| of
//    about 1e19 on).  These tests are made on the floats before any conversion to an integer, and no tap outside the region is
//    ever addressed.
// 4. Still camera: when the 19 floats of C0 and C1 compare equal, ul = (float) tx, vl = (float) ty and z' = z, exactly, in place of
//    2 and 3.  The weights of 5 then leave one tap of weight 1: accumulation without motion is exact.
// 5. Four bilinear taps.  i = floorf(ul), j = floorf(vl), fx = ul - i, fy = vl - j; the taps (i, j), (i + 1, j), (i, j + 1),
//    (i + 1, j + 1) in this order weigh (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy.  A tap COUNTS when its weight is
//    not 0, it lies in the region, its length > 0, its colour and depth are finite, it has the centre's class (miss / hit, by its
//    depth == 1e30), for hits |depth_h - z'| <= depth_tolerance * z', and with ids both id words equal the centre's.
//      sw += wt;  sc += wt * c_h per component;  sl += wt * length_h        (all from 0, over the counting taps)
//    sw < 0.25: no history.
// 6. Accumulate.  c_h = sc / sw;  L = min(sl / sw, max_history);  k = n / (L + n)
//      out = c_h + (c - c_h) * k per component, and c's bits where c - c_h == 0;      out_length = L + n
//    With no history: out = c's bits, out_length = n.  A pixel whose history equals its colour comes back exactly.
//
// WHAT THIS FORM DOES NOT DO.  No neighbourhood colour clamp: a history that has gone wrong (a light moved, a reflection slid
// over the surface) fades at the rate 1 / max_history and no faster.  No per-pixel variance.  No motion of objects: only the camera
// moves; the ids catch an edited node as a mismatch only if its id changes, and any other scene edit wants a fresh history
// (hip.TemporalPreview.reset).  A pinhole lens: the lens draw of a camera with dof > 0.1 is ignored, so its history lands where
// the lens centre would put it.
#pragma once
#include "qa_device_math.h"
#include "qa_flat_scene.h"

namespace qa {

#define QA_REPROJECT_MISS 1.0e30f
#define QA_REPROJECT_DEFAULT_DEPTH_TOLERANCE 0.05f
#define QA_REPROJECT_DEFAULT_MAX_HISTORY 64.0f
#define QA_REPROJECT_MIN_WEIGHT 0.25f

struct ReprojectPixel {
  float r, g, b, z;
  uint32_t ns;
};
struct ReprojectTap {
  float r, g, b, z, length;
};

// What a call computes once (on the host, for the kernel and for the host form alike)
struct ReprojectSetup {
  f3 A1, U1, V1, pos1;                // C1
  f3 pos0, a, nrm, vn, nu;            // C0
  float an, du, dv;
  float depthTolerance, maxHistory;
  int x0, y0, W, H;
  int still;
};

__host__ __device__ __forceinline__ bool reprojectFinite(float x) { return (qa_asuint(x) & 0x7f800000u) != 0x7f800000u; }

inline ReprojectSetup reprojectSetup(const qa_camera &c0, const qa_camera &c1, int x0, int y0, int W, int H, float depthTolerance, float maxHistory)
{
  ReprojectSetup s;
  s.A1 = ld3(c1.screenA); s.U1 = ld3(c1.screenU); s.V1 = ld3(c1.screenV); s.pos1 = ld3(c1.cam_pos);
  const f3 A0 = ld3(c0.screenA), U0 = ld3(c0.screenU), V0 = ld3(c0.screenV);
  s.pos0 = ld3(c0.cam_pos);
  s.a = A0 - s.pos0;
  s.nrm = cross(U0, V0);
  s.an = dot(s.a, s.nrm);
  s.vn = cross(V0, s.nrm);
  s.nu = cross(s.nrm, U0);
  s.du = dot(U0, s.vn);
  s.dv = dot(V0, s.nu);
  s.depthTolerance = depthTolerance; s.maxHistory = maxHistory;
  s.x0 = x0; s.y0 = y0; s.W = W; s.H = H;
  const float *p = c0.screenA, *q = c1.screenA;   // (the record is 19 floats and nothing else: include/qa_flat_scene.h)
  s.still = 1;
  for (int i = 0; i < 19; ++i)
    if (!(p[i] == q[i])) s.still = 0;
  return s;
}

// Step 3 for a pixel's w: -> false for NO HISTORY, else the region-local (ul, vl) and, for a hit, z'
__host__ __device__ __forceinline__ bool reprojectProject(const ReprojectSetup &S, f3 w, bool miss, float &ul, float &vl, float &zh)
{
  const float wn = dot(w, S.nrm);
  if (wn == 0.f) return false;
  const float s = S.an / wn;
  if (!(s > 0.f)) return false;
  const f3 r = w * s - S.a;
  const float u = dot(r, S.vn) / S.du, v = dot(r, S.nu) / S.dv;
  ul = u - (float) S.x0; vl = v - (float) S.y0;
  if (!reprojectFinite(ul) || !reprojectFinite(vl)) return false;
  if (!(ul >= -1.f && ul < (float) S.W && vl >= -1.f && vl < (float) S.H)) return false;
  zh = 0.f;
  if (!miss) {
    zh = length(w);
    if (!reprojectFinite(zh)) return false;
  }
  return true;
}

// Step 5 around (ul, vl) for a centre of class `miss` and ids cid: -> sw, and the sums sc[3] and sl over the counting taps
template <class Tap, class Ids>
__host__ __device__ __forceinline__ float reprojectTaps(const ReprojectSetup &S, const Tap &tap, const Ids &ids, bool withIds, const int *cid, bool miss,
                                                        float ul, float vl, float zh, float *sc, float &sl)
{
  const float fi = __builtin_floorf(ul), fj = __builtin_floorf(vl);
  const float fx = ul - fi, fy = vl - fj;
  const int i0 = (int) fi, j0 = (int) fj;   // -1 .. W - 1, -1 .. H - 1
  const float tol = S.depthTolerance * zh;
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
  sl = 0.f;
#pragma unroll
  for (int dj = 0; dj < 2; ++dj) {
#pragma unroll
    for (int di = 0; di < 2; ++di) {
      const float wt = (di ? fx : 1.f - fx) * (dj ? fy : 1.f - fy);
      const int i = i0 + di, j = j0 + dj;
      if (wt == 0.f || i < 0 || j < 0 || i >= S.W || j >= S.H) continue;
      ReprojectTap t;
      tap(i, j, t);
      if (!(t.length > 0.f) || !reprojectFinite(t.r) || !reprojectFinite(t.g) || !reprojectFinite(t.b) || !reprojectFinite(t.z)) continue;
      if ((t.z == QA_REPROJECT_MISS) != miss) continue;
      if (!miss && !(qabs(t.z - zh) <= tol)) continue;
      if (withIds) {
        int hid[2];
        ids(1, i, j, hid);
        if (hid[0] != cid[0] || hid[1] != cid[1]) continue;
      }
      sw += wt;
      sr += wt * t.r; sg += wt * t.g; sb += wt * t.b;
      sl += wt * t.length;
    }
  }
  sc[0] = sr; sc[1] = sg; sc[2] = sb;
  return sw;
}

// Step 6 with the history colour ch[3] and the sums of step 5: -> out[3] and the new length
__host__ __device__ __forceinline__ float reprojectAccumulate(const ReprojectSetup &S, const ReprojectPixel &p, float n, const float *ch, float sw, float sl,
                                                              float *out)
{
  const float L = qmin(sl / sw, S.maxHistory);
  const float k = n / (L + n);
  const float c[3] = {p.r, p.g, p.b};
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float diff = c[e] - ch[e];
    out[e] = diff == 0.f ? c[e] : ch[e] + diff * k;
  }
  return L + n;
}

}  // namespace qa
