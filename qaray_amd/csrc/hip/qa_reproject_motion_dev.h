// qa_reproject_motion_dev.h — temporal reprojection that follows moved nodes and clamps stale history: the form of
// qa_reproject_dev.h with two additions, each behind a flag.  No reference counterpart.  Every function here is compiled for the host
// too: qa_test_reproject_motion_host and the kernel qa_reproject_k<1> of qa_reproject.hip run the same source
// (tests/test_gpu_reproject_motion.py: equal bit for bit); tests/reproject_motion_util.py restates THIS COMMENT in float64 numpy.
// The pixel that runs these steps is reprojectPixel<FORM> of qa_reproject_moments_dev.h (this form: FORM 1).
//
// SPECIFICATION.  Steps 1 - 6, the arithmetic rules (fp32 in the order written, no contraction, correctly rounded / and sqrtf), the
// frames, the classes and the outputs are those of qa_reproject_dev.h; with flags 0 every output has that form's bits.
// Parameters: depth_tolerance and max_history as there; flags, a set of QA_REPROJECT_MOTION = 1 and QA_REPROJECT_CLAMP = 2;
// clamp_radius r (1 .. 3) and clamp_gamma (finite, >= 0), read only with QA_REPROJECT_CLAMP.
//
// NODE MOTION (QA_REPROJECT_MOTION).  A further input: a table of `count` records qa_node_motion { float m[12]; uint32_t moved;
// uint32_t pad[3]; } of 64 bytes, one per node of the scene.  m is a 3x3 matrix, row-major in m[0 .. 8], then a translation in
// m[9 .. 11]: it takes a world point of the CURRENT scene to the world point where the same point of the node lay in the PREVIOUS
// scene (the scene the history was rendered from).  moved == 0: the node and all its ancestors stand where they stood.  Both ids
// planes are required; word 0 of an id is the node's index (h.node of the guide planes).  How the table was built takes no part
// here (qa_reproject_node_motion builds it from two instance tables, below).
//   2'. After step 2's P = pos1 + d * z, for a HIT pixel whose current id word 0 is n with 0 <= n < count and motion[n].moved != 0
//       (a MOVED pixel):
//         P0.x = ((m[0] * P.x + m[1] * P.y) + m[2] * P.z) + m[9]
//         P0.y = ((m[3] * P.x + m[4] * P.y) + m[5] * P.z) + m[10]
//         P0.z = ((m[6] * P.x + m[7] * P.y) + m[8] * P.z) + m[11];        w = P0 - pos0
//       Every other pixel is UNMOVED and keeps w of step 2: a miss, an id word below 0 or >= count (the table is never addressed
//       with it), a record whose moved is 0 (its m is not read).
//   4'. The still-camera shortcut of step 4 applies to a pixel only when the cameras are equal AND the pixel is unmoved; a moved
//       pixel under equal cameras goes through steps 2, 2' and 3.
//   Steps 3 and 5 run unchanged on w: z' = |w| is the depth the old camera saw the point at where it then lay, and the ids test
//   finds the moved object there.  A pixel the object uncovered meets another id among its taps and gets no history.
//
// COLOUR CLAMP (QA_REPROJECT_CLAMP).  Between steps 5 and 6, for a pixel that has history (sw >= 0.25), with c_h = sc / sw:
//   5'. The window is [tx - r, tx + r] x [ty - r, ty + r] clipped to the region.  Its CONTRIBUTING pixels are the pixels of the
//       CURRENT frame in it that are not void and have the centre's class (miss / hit); the centre is one of them.  They are
//       scanned row after row from the top, each row from the left.  k: their number; kf = (float) k.  Per colour component:
//         s = 0;  s += c  over the scan;              m = s / kf
//         q = 0;  e = c - m;  q += e * e  (a second scan);      sigma = sqrtf(q / kf)
//         lo = m - clamp_gamma * sigma;               hi = m + clamp_gamma * sigma
//       When k >= 2 and all six bounds are finite:  c_h <- lo where c_h < lo, hi where c_h > hi, else c_h as it is (a c_h inside
//       the box, and one that is not a number, keep their bits).  With k == 1, or a bound that is not finite, c_h stays as it is.
//   Step 6 then runs on the clamped c_h; L and out_length are those of the call without the clamp.
//
// THE TABLE.  qa_reproject_node_motion(prev, cur, count, out): with L_k(p) = tm_k p + pos_k (tm column-major, as everywhere) and
// W(k) = W(parent(k)) o L_k (the root's parent is -1: W(-1) is the identity), record k is  M_k = Wprev(k) o Wcur(k)^-1, where the
// inverse runs through the itm chain as the integrators take a ray into a node:  Wcur(k)^-1 (q) = itm_k (Wcur(parent(k))^-1 (q) - pos_k).
// Composed in double precision and rounded once to float.  moved = 0 if and only if tm, itm and pos compare equal as floats
// between the two tables for k and every ancestor of k; m is then the exact identity (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0).
//
// WHAT THIS FORM STILL DOES NOT DO.  The length is not reduced when the clamp bites; no per-pixel variance; no deforming meshes
// (a node moves rigidly or affinely as a whole); an edit that changes ids or topology wants a fresh history; a pinhole lens.  A
// shadow or a reflection that an object's move drags over an unmoved surface is stale history there: the clamp bounds it, the
// motion table knows nothing of it.
#pragma once
#include "qa_reproject_dev.h"
#include "qaray_hip.h"

namespace qa {

#define QA_REPROJECT_DEFAULT_CLAMP_RADIUS 1
#define QA_REPROJECT_DEFAULT_CLAMP_GAMMA 1.0f

// What a call adds to ReprojectSetup
struct ReprojectMotionSetup {
  const qa_node_motion *motion;   // read only with QA_REPROJECT_MOTION
  int count;
  uint32_t flags;
  int clampRadius;
  float clampGamma;
};

// A pixel of the clamp's window: its colour and 0 (does not contribute: void, or outside the region), 1 (miss) or 2 (hit)
struct ReprojectWin {
  float r, g, b;
  uint32_t cls;
};

__host__ __device__ __forceinline__ ReprojectWin reprojectWinOf(const ReprojectPixel &p)
{
  ReprojectWin q;
  q.r = p.r; q.g = p.g; q.b = p.b;
  const bool isVoid = p.ns == 0u || !reprojectFinite(p.r) || !reprojectFinite(p.g) || !reprojectFinite(p.b) || !reprojectFinite(p.z);
  q.cls = isVoid ? 0u : (p.z == QA_REPROJECT_MISS ? 1u : 2u);
  return q;
}

// The box of step 5' around (tx, ty): -> false when the window clamps nothing (k < 2, or a bound that is not finite), else lo[3],
// hi[3] and g[3] = clamp_gamma * sigma.  win(x, y) -> ReprojectWin for x in tx - r .. tx + r, y in ty - r .. ty + r (cls 0 outside
// the region)
template <class Win>
__host__ __device__ __forceinline__ bool reprojectClampBox(const ReprojectMotionSetup &M, const Win &win, uint32_t cls, int tx, int ty, float *lo, float *hi,
                                                           float *g)
{
  const int r = M.clampRadius;
  int k = 0;
  float s[3] = {0.f, 0.f, 0.f};
  for (int y = ty - r; y <= ty + r; ++y)
    for (int x = tx - r; x <= tx + r; ++x) {
      const ReprojectWin q = win(x, y);
      if (q.cls != cls) continue;
      ++k;
      s[0] += q.r; s[1] += q.g; s[2] += q.b;
    }
  if (k < 2) return false;
  const float kf = (float) k;
  const float m[3] = {s[0] / kf, s[1] / kf, s[2] / kf};
  float v[3] = {0.f, 0.f, 0.f};
  for (int y = ty - r; y <= ty + r; ++y)
    for (int x = tx - r; x <= tx + r; ++x) {
      const ReprojectWin q = win(x, y);
      if (q.cls != cls) continue;
      const float e0 = q.r - m[0], e1 = q.g - m[1], e2 = q.b - m[2];
      v[0] += e0 * e0; v[1] += e1 * e1; v[2] += e2 * e2;
    }
  bool finite = true;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float sigma = qsqrt(v[e] / kf);
    g[e] = M.clampGamma * sigma;
    lo[e] = m[e] - g[e]; hi[e] = m[e] + g[e];
    finite = finite && reprojectFinite(lo[e]) && reprojectFinite(hi[e]);
  }
  return finite;
}

// Step 5': c_h[3] clamped to the window around (tx, ty); win as for reprojectClampBox
template <class Win>
__host__ __device__ __forceinline__ void reprojectClamp(const ReprojectMotionSetup &M, const Win &win, uint32_t cls, int tx, int ty, float *ch)
{
  float lo[3], hi[3], g[3];
  if (!reprojectClampBox(M, win, cls, tx, ty, lo, hi, g)) return;
#pragma unroll
  for (int e = 0; e < 3; ++e) ch[e] = ch[e] < lo[e] ? lo[e] : (ch[e] > hi[e] ? hi[e] : ch[e]);
}

// Steps 2, 2', 3 and 4' for the non-void pixel p at (tx, ty) with ids cid: -> false for NO HISTORY, else where its taps lie
__host__ __device__ __forceinline__ bool reprojectMotionWhere(const ReprojectSetup &S, const ReprojectMotionSetup &M, const ReprojectPixel &p, bool miss,
                                                              const int *cid, int tx, int ty, float &ul, float &vl, float &zh)
{
  // the node's record: addressed only with an id inside the table, read only when the node moved
  const qa_node_motion *rec = nullptr;
  if ((M.flags & QA_REPROJECT_MOTION) && !miss && cid[0] >= 0 && cid[0] < M.count && M.motion[cid[0]].moved != 0u) rec = M.motion + cid[0];
  if (S.still && !rec) {
    ul = (float) tx; vl = (float) ty; zh = p.z;
    return true;
  }
  const float fpx = (float) (S.x0 + tx), fpy = (float) (S.y0 + ty);
  const f3 cpt = (S.A1 + S.U1 * fpx) + S.V1 * fpy;
  const f3 d = normalize(cpt - S.pos1);
  f3 w = d;
  if (!miss) {
    f3 P = S.pos1 + d * p.z;
    if (rec) {
      const float *m = rec->m;
      P = F3(((m[0] * P.x + m[1] * P.y) + m[2] * P.z) + m[9], ((m[3] * P.x + m[4] * P.y) + m[5] * P.z) + m[10],
             ((m[6] * P.x + m[7] * P.y) + m[8] * P.z) + m[11]);
    }
    w = P - S.pos0;
  }
  return reprojectProject(S, w, miss, ul, vl, zh);
}

}  // namespace qa
