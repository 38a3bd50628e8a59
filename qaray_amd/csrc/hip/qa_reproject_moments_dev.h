// qa_reproject_moments_dev.h — temporal reprojection that carries luminance moments and shortens clamped history: the form of
// qa_reproject_motion_dev.h with two more additions, each behind a flag.  No reference counterpart.  Every function here is compiled
// for the host too: qa_test_reproject_moments_host and the kernel qa_reproject_k<2> of qa_reproject.hip run the same source
// (tests/test_gpu_reproject_moments.py: equal bit for bit); tests/reproject_moments_util.py restates THIS COMMENT in float64 numpy.
//
// SPECIFICATION.  Steps 1 - 6, 2', 4' and 5', the arithmetic rules (fp32 in the order written, no contraction, correctly rounded /
// and sqrtf), the frames, the classes, the motion table and the outputs out_rgb and out_length are those of qa_reproject_dev.h and
// qa_reproject_motion_dev.h; with neither new flag every output has qa_reproject_motion_dev.h's bits.
// Parameters: depth_tolerance, max_history, clamp_radius, clamp_gamma as there; flags, a set of QA_REPROJECT_MOTION = 1,
// QA_REPROJECT_CLAMP = 2, QA_REPROJECT_MOMENTS = 4 and QA_REPROJECT_SHORTEN = 8 (SHORTEN only together with CLAMP); min_frames (finite,
// >= 1; default 4), read only with MOMENTS; shorten_rate (finite, >= 0; default 4: DESIGN 4k has the sweep), read only with SHORTEN.
//
// SHORTENED LENGTH (QA_REPROJECT_SHORTEN).  For a pixel that has history, after step 5':
//   5''. With c_h before and after the clamp of 5', and sigma of 5' per component:
//          d = 0;  per component in the order r, g, b:  x = |c_h before - c_h after|;  d = x where x > d   (an x that is not a
//          number is passed over)
//          s = 0;  per component:  x = clamp_gamma * sigma;  s = x where x > s
//          b = (shorten_rate * d) / (s + 1e-4f);  a b that is not > 0 (0 * infinity is not a number) is 0
//        Where 5' leaves c_h as it is - a window of one contributing pixel, a bound that is not finite - b = 0.
//   6'.  Step 6 runs with L' = L / (1 + b) in place of L = min(sl / sw, max_history):  k = n / (L' + n),  out_length = L' + n.
//        A history inside the box has d == 0, hence b == 0 and L' == L: the colour and the length keep the bits they have with
//        the flag clear.  A history far outside a quiet window (d large against s + 1e-4) enters the next frame as if it had
//        just been uncovered.
//
// MOMENTS (QA_REPROJECT_MOMENTS).  One more history plane, hist_moments[2] per pixel (the accumulated first and second moment of
// the luma), which may be NULL: then no pixel has moment history.  Two more outputs: out_moments[2] and out_variance[1].
//   l = luma(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b         (denoiseLuma of qa_denoise_dev.h)
//   5m. Over the counting taps of step 5, with their weights and in their order, (h1, h2) the tap's two moments:
//         sm1 += wt * h1;  sm2 += wt * h2        (from 0)
//       A pixel has MOMENT HISTORY when it has history, the plane is given and every moment of every counting tap is finite.  One
//       moment that is not finite among them: the pixel keeps its colour history and has no moment history.
//   6m. With k of the call (after 6'):   h1 = sm1 / sw;  h2 = sm2 / sw
//         o1 = h1 + (l - h1) * k;   o2 = h2 + (l * l - h2) * k                  without moment history:  o1 = l,  o2 = l * l
//       out_moments = (o1, o2).   v = o2 - o1 * o1
//       The pixel is TRUSTED when it has moment history, out_length >= min_frames * n, and v is finite:
//         out_variance = max(v, 0) * k               every other pixel:  out_variance = -1   ("none" to qa_denoise_dev.h)
//   A void pixel: out_moments = (0, 0), out_variance = -1.
//   v is the variance of ONE frame's luma at this pixel, as the exponentially weighted moments estimate it; times k, one frame's
//   share of the accumulation, it is the variance of the accumulated colour's luma.  That product is exact when all frames behind the
//   pixel weigh the same (a still pixel below max_history: k = 1 / frames, and the variance of a mean of `frames` equal draws is v /
//   frames).  Once max_history caps L the weights decay geometrically and the true factor is k / (2 - k): v * k overstates by up to
//   2x, on the safe side for a filter.  It does not see the clamp: the moments are blended and not clamped, so a history that 5'
//   pulled in still shows its old spread in v until 6' or time has let it go.  min_frames counts in units of THIS frame's n: the
//   threshold is in samples, not frames, and a pixel whose earlier frames had fewer samples each waits longer.
//
// WHAT THIS FORM STILL DOES NOT DO.  The variance is of the luma only; the moments are not clamped; the trust threshold is in
// samples, not frames; no deforming meshes (a node moves rigidly or affinely as a whole); an edit that changes ids or topology
// wants a fresh history; a pinhole lens.  A shadow or a reflection that an object's move drags over an unmoved surface is stale
// history there: the clamp bounds it and the shortened length lets it go, the motion table knows nothing of it.
#pragma once
#include "qa_denoise_dev.h"
#include "qa_reproject_motion_dev.h"

namespace qa {

#define QA_REPROJECT_DEFAULT_MIN_FRAMES 4.0f
#define QA_REPROJECT_DEFAULT_SHORTEN_RATE 4.0f
#define QA_REPROJECT_SHORTEN_FLOOR 1.0e-4f

// What a call adds to ReprojectMotionSetup
struct ReprojectMomentsSetup {
  float minFrames, shortenRate;
};

// A history pixel's moments as a tap of step 5: (h1, h2) in the first two colour slots, and in the third 1 where one of them is not
// finite (both then enter as 0), else 0; the colour itself only decides, as in step 5, whether the tap counts.  Over the counting
// taps reprojectTaps then returns sm1, sm2 and - above 0 - the weight of the taps without moments.
template <class Tap, class Mom>
struct ReprojectMomentTap {
  const Tap &tap;
  const Mom &mom;
  __host__ __device__ __forceinline__ void operator()(int x, int y, ReprojectTap &t) const
  {
    tap(x, y, t);
    if (!reprojectFinite(t.r) || !reprojectFinite(t.g) || !reprojectFinite(t.b)) return;   // does not count: as it is
    float h[2];
    mom(x, y, h);
    const bool whole = reprojectFinite(h[0]) && reprojectFinite(h[1]);
    t.r = whole ? h[0] : 0.f;
    t.g = whole ? h[1] : 0.f;
    t.b = whole ? 0.f : 1.f;
  }
};

// Steps 5' and 5'' on c_h[3]: the clamp of reprojectClamp, and -> b of what it moved (0 where it moved nothing)
template <class Win>
__host__ __device__ __forceinline__ float reprojectClampShorten(const ReprojectMotionSetup &M, const ReprojectMomentsSetup &X, const Win &win, uint32_t cls,
                                                                int tx, int ty, float *ch)
{
  float lo[3], hi[3], g[3];
  if (!reprojectClampBox(M, win, cls, tx, ty, lo, hi, g)) return 0.f;
  float d = 0.f, s = 0.f;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float before = ch[e];
    ch[e] = before < lo[e] ? lo[e] : (before > hi[e] ? hi[e] : before);
    const float x = qabs(before - ch[e]);
    if (x > d) d = x;
    if (g[e] > s) s = g[e];
  }
  const float b = X.shortenRate * d / (s + QA_REPROJECT_SHORTEN_FLOOR);
  return b > 0.f ? b : 0.f;
}

// THE PIXEL OF ALL THREE FORMS.  FORM is the rank of the form the caller's entry belongs to, a compile-time fact: 0 the plain form of
// qa_reproject_dev.h, 1 with steps 2', 4' and 5' of qa_reproject_motion_dev.h, 2 with steps 5'', 6', 5m and 6m of this header.  What
// a lower rank does not have is not compiled into it: it reads neither M, X, mom, win, om nor var (rank 0), or neither X, mom, om
// nor var (rank 1), whatever their types, and a flag of a higher rank in M.flags means nothing to it.
// Pixel (tx, ty) of the region.  cur(tx, ty) -> ReprojectPixel; tap(i, j, t) fetches a history pixel, and ids(which, i, j, out)
// the two id words of the current (which = 0) or the history (1) frame, all called for pixels inside the region only; withIds:
// both ids planes are given.  win(x, y) -> ReprojectWin as for reprojectClamp (called with QA_REPROJECT_CLAMP only); mom(x, y, h)
// fetches a history pixel's two moments, called only with withMoments: QA_REPROJECT_MOMENTS is set and the plane is given.
// -> out[3] and the new length; in rank 2 also om[2] and var, which the caller stores with QA_REPROJECT_MOMENTS only
template <int FORM, class Cur, class Tap, class Mom, class Ids, class Win>
__host__ __device__ __forceinline__ float reprojectPixel(const ReprojectSetup &S, const ReprojectMotionSetup &M, const ReprojectMomentsSetup &X, const Cur &cur,
                                                         const Tap &tap, const Mom &mom, const Ids &ids, const Win &win, bool withIds, bool withMoments, int tx,
                                                         int ty, float *out, float *om, float &var)
{
  const ReprojectPixel p = cur(tx, ty);
  out[0] = p.r; out[1] = p.g; out[2] = p.b;
  if constexpr (FORM >= 2) {
    om[0] = 0.f; om[1] = 0.f; var = -1.f;
  }
  if (p.ns == 0u || !reprojectFinite(p.r) || !reprojectFinite(p.g) || !reprojectFinite(p.b) || !reprojectFinite(p.z)) return 0.f;
  const float n = (float) p.ns;
  const bool miss = p.z == QA_REPROJECT_MISS;
  float l = 0.f;
  if constexpr (FORM >= 2) {
    l = denoiseLuma(p.r, p.g, p.b);
    om[0] = l; om[1] = l * l;
  }
  int cid[2] = {0, 0};
  if (withIds) ids(0, tx, ty, cid);
  // steps 2 - 4: those of rank 1 with no node's record to find, which is all rank 0 knows
  const ReprojectMotionSetup unmoved = {nullptr, 0, 0u, 0, 0.f};
  float ul, vl, zh;
  if (!reprojectMotionWhere(S, FORM >= 1 ? M : unmoved, p, miss, cid, tx, ty, ul, vl, zh)) return n;
  float sc[3], sl;
  const float sw = reprojectTaps(S, tap, ids, withIds, cid, miss, ul, vl, zh, sc, sl);
  if (sw < QA_REPROJECT_MIN_WEIGHT) return n;
  float ch[3] = {sc[0] / sw, sc[1] / sw, sc[2] / sw};
  float b = 0.f;
  if constexpr (FORM >= 1) {
    if (M.flags & QA_REPROJECT_CLAMP) {
      if (FORM >= 2 && (M.flags & QA_REPROJECT_SHORTEN))
        b = reprojectClampShorten(M, X, win, miss ? 1u : 2u, tx, ty, ch);
      else
        reprojectClamp(M, win, miss ? 1u : 2u, tx, ty, ch);
    }
  }
  if constexpr (FORM < 2) {
    return reprojectAccumulate(S, p, n, ch, sw, sl, out);
  } else {
    float len;
    float k;
    if (M.flags & QA_REPROJECT_SHORTEN) {
      // step 6 on L' : min(L' / 1, max_history) is L', since L' <= L <= max_history
      const float L = qmin(sl / sw, S.maxHistory) / (1.f + b);
      len = reprojectAccumulate(S, p, n, ch, 1.f, L, out);
      k = n / (L + n);
    } else {
      len = reprojectAccumulate(S, p, n, ch, sw, sl, out);
      k = n / (qmin(sl / sw, S.maxHistory) + n);
    }
    if (!withMoments) return len;
    const ReprojectMomentTap<Tap, Mom> mtap = {tap, mom};
    float sm[3], sl2;
    const float sw2 = reprojectTaps(S, mtap, ids, withIds, cid, miss, ul, vl, zh, sm, sl2);   // the same taps count: sw2 has sw's bits
    if (sm[2] > 0.f || !(sw2 >= QA_REPROJECT_MIN_WEIGHT)) return len;
    const float h1 = sm[0] / sw2, h2 = sm[1] / sw2;
    const float o1 = h1 + (l - h1) * k, o2 = h2 + (l * l - h2) * k;
    om[0] = o1; om[1] = o2;
    const float v = o2 - o1 * o1;
    if (len >= X.minFrames * n && reprojectFinite(v)) var = qmax(v, 0.f) * k;
    return len;
  }
}

}  // namespace qa
