// qa_tilecull.h — which leaves of a mesh's own tree (qa_fastbvh.h) can the camera rays of one 8x8 pixel tile reach?
//
// Every camera ray of a tile leaves the same origin (no depth of field) through the same window of the screen plane, so the
// leaves such a ray can enter depend on the tile alone.  qa_integrate builds the list once per work item and its camera
// casts test the listed leaves' triangles instead of walking the tree (qa_kernel.h, section A and hitMesh).  Shared by host
// and device: tests/cpp/tile_cull_check.cpp compares the routine with the walk's own box test, ray by ray.
//
// The question is asked in the mesh's node space: the origin and the window's four corners go through the node chain as
// points (affine maps keep the window planar and the rays inside the pyramid they span).  The answer is conservative - "yes"
// for a box no ray enters only costs triangle tests, "no" for a box a ray enters would lose a hit:
//   * the window is half a pixel wider than the tile on every side (sample offsets lie in [0, 1) of a pixel);
//   * the walk tests LINES, not rays (entry <= exit, exit may be negative): the box is kept when it meets the pyramid or its
//     mirror image behind the origin; an origin inside the box meets both;
//   * the walk ignores an axis on which |d| < 1e-7 (slab()): where a tile's directions can come that close to zero on an axis,
//     the box counts as unbounded on it;
//   * the box is widened by the walk's pad and by what fp32 can move a ray or a slab distance by (relative to the coordinates
//     involved), with a wide margin.
#pragma once
#include "qa_device_math.h"
#include "qa_flat_scene.h"
#include "qa_scene_dev.h"   // QA_SLACK_SCALE

#define QA_TILE_LEAF_CAP 64   /* leaves per mesh a leaf table may hold: one ballot fills a list */
// A wave's lists, 30 words of LDS - what the Cornell box's workgroups can add and stay five to a CU (PlanScene):
#define QA_TILE_LIST_HDR 4    /* one word for each of the first four mesh nodes with a leaf table, in scene order: bit 31 = the node has a list, count << 8 | first entry */
#define QA_TILE_LIST_CAP 26   /* listed leaves per wave, all those nodes together; one word each: */
#define QA_TILE_LIST_DWORDS (QA_TILE_LIST_HDR + QA_TILE_LIST_CAP)
// entry = upper half of the entry bound's float (cut off: a smaller, still valid bound) | triangles - 1 << 12 | first triangle
#define QA_TILE_ENTRY(word, boundBits) (((boundBits) & 0xFFFF0000u) | ((((word) >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) << 12) | ((word) & 0xFFFu))
#define QA_TILE_ENTRY_FACES 4096u   /* meshes of more triangles have no leaf table (a resident scene has at most 512) */
#ifndef QA_TILE_LISTS_AUTO
#define QA_TILE_LISTS_AUTO 8  /* "tile_lists" = -1: tiles whose list for a mesh is longer than this walk the tree (profiles/tile_lists.txt) */
#endif

namespace qa {

// ---- the walk's own text, here so that the host check applies it to the same rays (qa_kernel.h uses these) ------------------
struct Ray { f3 p, d; };

// Node::ToNodeCoords (src/core/node.cpp:112-118, src/core/transform.h:47-61)
__host__ __device__ __forceinline__ Ray toNode(const qa_instance &in, const Ray &r)
{
  const f3 pos = ld3(in.pos);
  Ray o;
  o.p = mulMV(in.itm, r.p - pos);
  o.d = mulMV(in.itm, (r.p + r.d) - pos) - o.p;
  return o;
}

// One axis of the slab test (src/objects/objects.cpp:360-395, src/core/box.cpp:103-123)
__host__ __device__ __forceinline__ void slab(float d, float p0, float p1, float &t0, float &t1)
{
  if (qabs(d) < 1e-7f) { t0 = -QA_BIGFLOAT; t1 = QA_BIGFLOAT; }
  else { t0 = qmin(p0, p1); t1 = qmax(p0, p1); }
}

// Slab tests of the library's own tree: the box is widened by `pad` on every side (folded into two
// copies of the ray origin, so the widening costs nothing per box).  Any conservative form will do
// here - these tests only decide where the own tree is searched, never what the reference accepts.
__host__ __device__ __forceinline__ void boxEntryExitPadFast(f3 pLo, f3 pHi, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const f3 p0 = (bmin - pLo) * drcp;
  const f3 p1 = (bmax - pHi) * drcp;
  entry = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(p0.x, p1.x), __builtin_fminf(p0.y, p1.y)), __builtin_fminf(p0.z, p1.z));
  exit_ = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(p0.x, p1.x), __builtin_fmaxf(p0.y, p1.y)), __builtin_fmaxf(p0.z, p1.z));
}
__host__ __device__ __forceinline__ void boxEntryExitPad(f3 pLo, f3 pHi, f3 d, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const f3 p0 = (bmin - pLo) * drcp;
  const f3 p1 = (bmax - pHi) * drcp;
  f3 t0, t1;
  slab(d.x, p0.x, p1.x, t0.x, t1.x);   // a near-zero direction component leaves the axis unbounded
  slab(d.y, p0.y, p1.y, t0.y, t1.y);
  slab(d.z, p0.z, p1.z, t0.z, t1.z);
  entry = qmax(t0.x, qmax(t0.y, t0.z));
  exit_ = qmin(t1.x, qmin(t1.y, t1.z));
}

// The fast form with the ray's share of a plane distance formed once per ray and mesh: (b - q) * drcp = b * drcp + c with
// c = -(q * drcp), one fma per plane (walkBVH<true> carries cLo / cHi where the other forms carry pLo / pHi).  Only for rays
// whose every |d| component is >= 1e-7, as boxEntryExitPadFast: then every drcp is finite.
// Rounding (u = 2^-24, T = the exact plane distance (b - q) * drcp):
//   old form   fl(fl(b - q) * drcp):   |error| <= u |b - q| |drcp| + u |T|            = 2 u |b - q| |drcp|
//   this form  fma(b, drcp, fl(-q drcp)): |error| <= u |q| |drcp| + u |T|             = u (|q| + |b - q|) |drcp|
// (second order terms dropped).  An error e of a plane distance is the error of a plane moved by e / |drcp|: at most 2 u |b - q|
// before, u (|q| + |b - q|) now.  With P = max(|o|, |b|) the largest coordinate involved and pad << P: |q| <= P + pad and
// |b - q| <= 2 P + pad, so the old form moves a plane by up to 4 u P and this one by up to 3 u P ~ 1.8e-7 P - its worst case is the
// smaller one, although it is the larger one where b ~ q (an origin on a box face: the difference is exact, the product q drcp
// is not; there this form is off by u |q| <= 6e-8 P).  drcp itself is 1 / d rounded: another u / 2 of |b - q| in both forms, 4 u P ~
// 2.4e-7 P in all for this one.  Either way it is a quarter of the 1e-6 P term of fastWalkPad, which was sized
// for the slab arithmetic of the old form and the error of the ray's own point together: the pad stays as it is.  The tile
// lists' margin (TileCone::rel >= 3e-5 = 500 u of the same coordinates) covers this form as it covers the old one
// (tests/cpp/slab_form_check.cpp asks both questions ray by ray).
__host__ __device__ __forceinline__ f3 slabRayTerm(f3 q, f3 drcp) { return -(q * drcp); }
__host__ __device__ __forceinline__ void boxEntryExitPadFma(f3 cLo, f3 cHi, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const float p0x = __builtin_fmaf(bmin.x, drcp.x, cLo.x), p0y = __builtin_fmaf(bmin.y, drcp.y, cLo.y), p0z = __builtin_fmaf(bmin.z, drcp.z, cLo.z);
  const float p1x = __builtin_fmaf(bmax.x, drcp.x, cHi.x), p1y = __builtin_fmaf(bmax.y, drcp.y, cHi.y), p1z = __builtin_fmaf(bmax.z, drcp.z, cHi.z);
  entry = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(p0x, p1x), __builtin_fminf(p0y, p1y)), __builtin_fminf(p0z, p1z));
  exit_ = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(p0x, p1x), __builtin_fmaxf(p0y, p1y)), __builtin_fmaxf(p0z, p1z));
}

// The leaf test of refReaches (qa_kernel.h) on the reference's own slab interval of the accepted triangle's leaf.
// atFound = false: `limit` is a distance the reference held when it tested the box (an any-hit query's fixed t_max), or one not
// larger than that: its strict test.  atFound = true: `limit` is the distance t the search just found for a closest-hit query and
// no tie was seen - the reference then held MORE than t when it tested this box (refReaches has the argument), so entry == t passes
// its strict test too.
__host__ __device__ __forceinline__ bool refLeafReached(float entry, float exit_, float limit, bool atFound)
{
  return (atFound ? entry <= limit : entry < limit) && entry < exit_;
}

// The widening of the own tree's boxes for a ray whose origin's largest |coordinate| is oMax (hitMesh explains the constants);
// invH, absMax: DMesh.  Camera rays without depth of field share their origin: one pad per tile and mesh.
__host__ __device__ __forceinline__ float fastWalkPad(float invH, float absMax, float oMax)
{
  const float P = qmax(absMax, oMax);
  return ((QA_SLACK_SCALE * 1.2e-5f) * invH) * (P * P) + (QA_SLACK_SCALE * 1e-6f) * P;
}

// ---- the tile's pyramid ---------------------------------------------------------------------------------------------------
// Node::ToNodeCoords of a point, one level (the origin half of toNode, qa_kernel.h)
__host__ __device__ __forceinline__ f3 tileNodePoint(const qa_instance &in, f3 p) { return mulMV(in.itm, p - ld3(in.pos)); }

// The screen window of the tile whose first pixel is (X0, Y0), half a pixel wider on every side, in the order of a walk around
// it; (A + U * x) + V * y is the camera formula (renderer.cpp:312-328, qa_integrate section B)
__host__ __device__ __forceinline__ void tileWindow(f3 A, f3 U, f3 V, float X0, float Y0, f3 c[4])
{
  const float xa = X0 - 0.5f, xb = X0 + 8.5f, ya = Y0 - 0.5f, yb = Y0 + 8.5f;
  c[0] = (A + U * xa) + V * ya;
  c[1] = (A + U * xb) + V * ya;
  c[2] = (A + U * xb) + V * yb;
  c[3] = (A + U * xa) + V * yb;
}

// What the window's world-space shape contributes: the shortest and longest distance from the origin to a corner, and the
// window's diagonal (a ray's world direction is a unit vector, whatever the node chain does to it afterwards)
struct TileLens { float lenMin, lenMax, diag; };
__host__ __device__ __forceinline__ TileLens tileLens(f3 oW, const f3 cW[4])
{
  TileLens l;
  const float l0 = length(cW[0] - oW), l1 = length(cW[1] - oW), l2 = length(cW[2] - oW), l3 = length(cW[3] - oW);
  l.lenMin = qmin(qmin(l0, l1), qmin(l2, l3));
  l.lenMax = qmax(qmax(l0, l1), qmax(l2, l3));
  l.diag = qmax(length(cW[2] - cW[0]), length(cW[3] - cW[1]));
  return l;
}

// The tile's pyramid in one mesh's node space, 24 words.  Kept in memory (qa_integrate: wave-private LDS), not in registers.
struct TileCone {
  float o[3];      // the origin in node space
  float n[4][3];   // side planes through the origin, normals pointing into the pyramid
  float n1[4];     // |n|_1
  float oAbs;      // largest |coordinate| of the origin
  float rel;       // relative slack of a position: fp32 error of the rays and of the walk's slab arithmetic, with margin
  float dMax;      // upper bound of |d| of a tile's rays in node space
  uint32_t open;   // bit a: the walk may ignore axis a for some ray of the tile
};

// o, c: origin and window in node space
__host__ __device__ __forceinline__ void tileCone(const TileLens lens, f3 o, const f3 c[4], TileCone *t)
{
  const float oAbs = qmax(qmax(qabs(o.x), qabs(o.y)), qabs(o.z));
  t->o[0] = o.x; t->o[1] = o.y; t->o[2] = o.z;
  t->oAbs = oAbs;
  const f3 v0 = c[0] - o, v1 = c[1] - o, v2 = c[2] - o, v3 = c[3] - o;
  const f3 g = ((v0 + v1) + (v2 + v3)) * 0.25f;
  const f3 v[5] = {v0, v1, v2, v3, v0};
  for (int i = 0; i < 4; ++i) {
    f3 n = cross(v[i], v[i + 1] - v[i]);
    if (dot(n, g) < 0) n = -n;
    t->n[i][0] = n.x; t->n[i][1] = n.y; t->n[i][2] = n.z;
    t->n1[i] = (qabs(n.x) + qabs(n.y)) + qabs(n.z);
  }
  // a ray's node-space direction is M (w / |w|) with w = its window point - origin in world space and M the chain's linear
  // part: |M w| is largest at a corner (a norm is convex), |w| is nowhere smaller than the shortest corner distance less the
  // window's diagonal
  const float vMax = qmax(qmax(length(v0), length(v1)), qmax(length(v2), length(v3)));
  const float lenLow = lens.lenMin - lens.diag;
  t->dMax = lenLow > 0 ? (vMax / lenLow) * 1.0001f : 3e38f;
  // a component of M w is linear in w: it comes within the walk's 1e-7 of zero only where it changes sign between corners
  // or is that small at one of them (|w| <= lenMax); four times the threshold for the rounding of the chain
  const float tiny = 4e-7f * lens.lenMax;
  const bool openX = !((v0.x > tiny && v1.x > tiny && v2.x > tiny && v3.x > tiny) || (v0.x < -tiny && v1.x < -tiny && v2.x < -tiny && v3.x < -tiny));
  const bool openY = !((v0.y > tiny && v1.y > tiny && v2.y > tiny && v3.y > tiny) || (v0.y < -tiny && v1.y < -tiny && v2.y < -tiny && v3.y < -tiny));
  const bool openZ = !((v0.z > tiny && v1.z > tiny && v2.z > tiny && v3.z > tiny) || (v0.z < -tiny && v1.z < -tiny && v2.z < -tiny && v3.z < -tiny));
  t->open = (openX ? 1u : 0u) | (openY ? 2u : 0u) | (openZ ? 4u : 0u);
  // toNode forms a direction as the difference of two transformed points of the origin's size: an absolute error of a few
  // ulps of |o| on a vector of length >= vInfMin / lenMax, at every level of the chain; and the slab products carry a few
  // ulps of the distances themselves.  3e-5 is 250 ulps.
  const float i0 = qmax(qmax(qabs(v0.x), qabs(v0.y)), qabs(v0.z)), i1 = qmax(qmax(qabs(v1.x), qabs(v1.y)), qabs(v1.z));
  const float i2 = qmax(qmax(qabs(v2.x), qabs(v2.y)), qabs(v2.z)), i3 = qmax(qmax(qabs(v3.x), qabs(v3.y)), qabs(v3.z));
  const float dLow = qmin(qmin(i0, i1), qmin(i2, i3)) / lens.lenMax;
  t->rel = 3e-5f + (dLow > 0 ? 2e-6f * (oAbs / dLow) : 3e38f);
}

// Can a ray of the tile enter [bmin, bmax] widened by pad?  *tLow: a lower bound of the ray parameter at which it does
// (hit distances of camera rays inside this box are not smaller).
__host__ __device__ __forceinline__ bool tileConeMeetsBox(const TileCone *t, f3 bmin, f3 bmax, float pad, float *tLow)
{
  const float BIG = 3e38f;
  const float bAbs = qmax(qmax(qmax(qabs(bmin.x), qabs(bmax.x)), qmax(qabs(bmin.y), qabs(bmax.y))), qmax(qabs(bmin.z), qabs(bmax.z)));
  const float slack = pad + t->rel * ((t->oAbs + bAbs) + pad);
  // box relative to the origin; unbounded on the axes the walk may ignore
  const f3 o = ld3(t->o);
  f3 lo = bmin - o, hi = bmax - o;
  const uint32_t open = t->open;
  if (open & 1u) { lo.x = -BIG; hi.x = BIG; }
  if (open & 2u) { lo.y = -BIG; hi.y = BIG; }
  if (open & 4u) { lo.z = -BIG; hi.z = BIG; }
  bool fwdOut = false, bwdOut = false;
  for (int i = 0; i < 4; ++i) {
    const f3 n = ld3(t->n[i]);
    const float ax = n.x * lo.x, bx = n.x * hi.x, ay = n.y * lo.y, by = n.y * hi.y, az = n.z * lo.z, bz = n.z * hi.z;
    // largest and smallest n . (p - o) over the box (its p- and n-vertex); an overflow gives inf or NaN: never "out"
    const float sMax = (qmax(ax, bx) + qmax(ay, by)) + qmax(az, bz);
    const float sMin = (qmin(ax, bx) + qmin(ay, by)) + qmin(az, bz);
    const float tol = t->n1[i] * slack;
    fwdOut = fwdOut || (sMax < -tol);
    bwdOut = bwdOut || (sMin > tol);
  }
  // distance from the origin to the widened box over the largest |d|
  const float gx = qmax(qmax(lo.x, -hi.x) - slack, 0.f), gy = qmax(qmax(lo.y, -hi.y) - slack, 0.f), gz = qmax(qmax(lo.z, -hi.z) - slack, 0.f);
  const float dist = qsqrt((gx * gx + gy * gy) + gz * gz);
  const float tl = (dist / t->dMax) * 0.9999f;
  *tLow = tl > 0 ? tl : 0.f;   // (never NaN: the lists are ordered by it)
  return !(fwdOut && bwdOut);
}

}  // namespace qa
