// qa_bake_dev.h — bake maps: which surface point of a node lies behind each texel of a texture laid over it, and the gutter fill
// of a baked picture.  This comment is the specification; tests/bake_util.py restates it in float32 numpy and
// tests/test_bake_host.py holds the host build of the functions below to that restatement bit for bit, and the `face` plane to an
// evaluation of the inside rule in rational arithmetic.
//
// All arithmetic is fp32 in the order written, nothing is contracted, `/` and sqrtf are the correctly rounded ones.  No trig.
//
// PLANES.  Row-major [height][width]; every one is optional, but not all of them:
//   point   3 floats   the surface point, world space
//   normal  3 floats   the interpolated shading normal, world space
//   face    1 int32    the blob's face id (0 / 1 for a plane node), -1 where no face covers the texel
//   bary    2 floats   (a, b), the weights of the face's first two vertices
// An uncovered texel holds face = -1 and zeros in the other planes.
//
// THE SAMPLE OF TEXEL (ix, iy).  Row 0 is the top row as stored.
//   S = ((float) ix / (float) W,  iy == 0 ? 0 : 1 - (float) iy / (float) H)
// the coordinate at which texBilinearAt (qa_texture_dev.h) returns exactly that texel: x = width * u, y = height * (1 - v),
// both fractions zero.  One sample per texel; no supersampling.
//
// FACES.  The node's mesh faces in the blob's qa_face order, read from the raw arrays (vertices, normals, texcoords), not from the
// DTri records; mtl >= 0 keeps the faces with that qa_face::mtl only, mtl = -1 keeps all.  A plane node is the built-in pair
//   face 0: corners 0 1 2,  face 1: corners 0 2 3   of   (-1,-1,0) (1,-1,0) (1,1,0) (-1,1,0),  uv (0,0) (1,0) (1,1) (0,1)
// with normal (0, 0, 1) and mtl 0.  A sphere node is refused (QA_EUNSUPPORTED): its inverse map needs double-precision
// trigonometry that nothing here pins.  A node without an object, a node index out of range and a mesh without texture vertices
// are QA_EINVAL.
//
// A FACE'S TEXTURE VERTICES.  T_i = xformTo(texmap record, (u_i, v_i, 0)).xy with the renderer's xformTo; texmap = -1:
// T_i = (u_i, v_i).  The lookup ignores .z, so the forward affine map is all that is needed.  A face is VOID and skipped when it has
// a vt of -1 (or one beyond the mesh's texcoords), when a component of a T is not finite, or when
//   d = (T1.x - T0.x) * (T2.y - T0.y) - (T2.x - T0.x) * (T1.y - T0.y)
// is 0 (or not finite: it has no |d| to divide by).
//
// TILES.  The lookup wraps, so a face is tried at P = (S.x + m, S.y + n), m = fm0 + (float) j for j = 0 .. nm - 1 with
// fm0 = floorf(min T.x) and nm = floorf(max T.x) - fm0 + 1, likewise n, fn0 and nn in y.  If nm or nn of any face that is not void
// exceeds QA_BAKE_MAX_TILES = 4, the call is refused (QA_EUNSUPPORTED) and writes nothing: a map that shrinks the texture to nothing
// is not a bake map.  The refusal is decided before the launch by a pass of bakeFaceSetup over the host copy of the blob.
//
// INSIDE RULE.  P is tried against a face only within the face's box: min T.x <= P.x <= max T.x and min T.y <= P.y <= max T.y (in
// exact arithmetic the triangle lies in its box; in fp32 the box keeps products that underflow from claiming far texels, and lets
// the kernel skip a face by comparisons alone).  With
//   e(A, B) = (A.x - P.x) * (B.y - P.y) - (B.x - P.x) * (A.y - P.y)
// e0 = e(T1, T2), e1 = e(T2, T0), e2 = e(T0, T1), all three negated when d < 0.  P is inside iff e0 >= 0, e1 >= 0 and e2 >= 0.
// Two faces that share an edge evaluate that edge's function as exact negations of each other (x - y = -(y - x) in round-to-
// nearest), so a sample is never outside both: charts have no cracks.  The first inside combination wins: faces ascending, then n,
// then m.  Overlapping charts therefore give the lowest face.
//
// A COVERED TEXEL.  a = e0 / |d|, b = e1 / |d|, c = 1 - a - b;  p = (V0 * a + V1 * b) + V2 * c;  N = (N0 * a + N1 * b) + N2 * c,
// hitMesh's shading-normal expression, front side, never flipped.  Both go to world space by traceClosest's chain, from the node up:
//   at the root, if it is the identity (DScene::rootIdentity):  N = normalize(N), stop
//   else  p = mulMV(tm, p) + pos;  N = normalize(mulTMV(itm, N))
// so `normal` is unit, or NaN where the mesh's normals cancel (qa_ao_points treats such a point as void).
//
// GUTTER FILL (bakeDilateTexel).  A texel with face >= 0 keeps its bytes.  Another takes the bytes of the covered texel at the
// smallest dx * dx + dy * dy over |dx|, |dy| <= radius, ties to dy ascending, then dx ascending; neighbours wrap modulo width and
// height, as the lookup wraps.  With none in reach it keeps its own bytes.  radius <= QA_BAKE_MAX_RADIUS = 8; out != in.
//
// REFUSALS (QA_EINVAL): width or height 0 or above QA_BAKE_MAX_DIM = 8192; a texmap out of range or without a texture; no plane.
// On the device also QA_EUNSUPPORTED where the scene's traversal stacks leave less than 15 KB of a workgroup's 64 KB of LDS: the
// kernel's face chunk is static LDS beside the dynamic LDS every scene kernel is launched with (qa_bake.hip, BakeCheck).
//
// Every function here is compiled for the host too: qa_test_bake_*_host and the kernels of qa_bake.hip run the same source.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qa_texture_dev.h"

namespace qa {

#define QA_BAKE_MAX_TILES 4
#define QA_BAKE_MAX_DIM 8192u
#define QA_BAKE_MAX_RADIUS 8u

// where the faces come from: the mesh's raw arrays (on whichever side the code runs), or the built-in plane
struct BakeSource {
  const qa_face *faces;
  const float *vertices, *normals, *texcoords;
  uint32_t numFaces, numTexcoords;
  int32_t plane;      // 1: the built-in pair, the pointers are null
  int32_t mtl;        // -1: every face
  int32_t mapped;     // 1: T = xformTo(map, uv)
  qa_texmap map;
};

// a face as the walk needs it; nm == 0: void (or filtered out)
struct BakeFace {
  float t0x, t0y, t1x, t1y, t2x, t2y, d;
  float fm0, fn0;               // the first tile
  float bx0, bx1, by0, by1;     // the box of T
  uint32_t nm, nn;              // tiles per axis, 1 .. QA_BAKE_MAX_TILES
  uint32_t over;                // not void, and a tile count beyond the limit
};

struct BakeCorners { f3 v[3], n[3]; };

__host__ __device__ __forceinline__ float bakePlaneCoord(uint32_t corner, int axis)
{
  // (-1,-1) (1,-1) (1,1) (-1,1)
  const bool hi = axis == 0 ? (corner == 1 || corner == 2) : (corner >= 2);
  return hi ? 1.f : -1.f;
}
__host__ __device__ __forceinline__ uint32_t bakePlaneCorner(uint32_t f, int q) { return q == 0 ? 0u : (f == 0 ? (uint32_t) q : (uint32_t) q + 1u); }

__host__ __device__ __forceinline__ void bakeSample(uint32_t ix, uint32_t iy, uint32_t W, uint32_t H, float &sx, float &sy)
{
  sx = (float) ix / (float) W;
  sy = iy == 0 ? 0.f : 1.f - (float) iy / (float) H;
}

__host__ __device__ __forceinline__ BakeFace bakeFaceSetup(const BakeSource &src, uint32_t f)
{
  BakeFace r = {};
  float u[3], v[3];
  if (src.plane) {
    if (src.mtl >= 0 && src.mtl != 0) return r;
    for (int q = 0; q < 3; ++q) {
      const uint32_t k = bakePlaneCorner(f, q);
      u[q] = (bakePlaneCoord(k, 0) + 1.f) * 0.5f;
      v[q] = (bakePlaneCoord(k, 1) + 1.f) * 0.5f;
    }
  } else {
    const qa_face &fc = src.faces[f];
    if (src.mtl >= 0 && fc.mtl != src.mtl) return r;
    for (int q = 0; q < 3; ++q) {
      const int32_t k = fc.vt[q];
      if (k < 0 || (uint32_t) k >= src.numTexcoords) return r;
      u[q] = src.texcoords[2 * (size_t) k];
      v[q] = src.texcoords[2 * (size_t) k + 1];
    }
  }
  float tx[3], ty[3];
  for (int q = 0; q < 3; ++q) {
    if (src.mapped) {
      const f3 t = xformTo(src.map, F3(u[q], v[q], 0.f));
      tx[q] = t.x;
      ty[q] = t.y;
    } else {
      tx[q] = u[q];
      ty[q] = v[q];
    }
    if (!isfinite(tx[q]) || !isfinite(ty[q])) return r;
  }
  const float d = (tx[1] - tx[0]) * (ty[2] - ty[0]) - (tx[2] - tx[0]) * (ty[1] - ty[0]);
  if (d == 0.f || !isfinite(d)) return r;   // (a d that overflows has no |d| to divide by: void as well)
  r.t0x = tx[0]; r.t0y = ty[0]; r.t1x = tx[1]; r.t1y = ty[1]; r.t2x = tx[2]; r.t2y = ty[2];
  r.d = d;
  r.bx0 = qmin(qmin(tx[0], tx[1]), tx[2]);
  r.bx1 = qmax(qmax(tx[0], tx[1]), tx[2]);
  r.by0 = qmin(qmin(ty[0], ty[1]), ty[2]);
  r.by1 = qmax(qmax(ty[0], ty[1]), ty[2]);
  r.fm0 = floorf(r.bx0);
  r.fn0 = floorf(r.by0);
  const float cm = floorf(r.bx1) - r.fm0 + 1.f, cn = floorf(r.by1) - r.fn0 + 1.f;
  if (!(cm <= (float) QA_BAKE_MAX_TILES) || !(cn <= (float) QA_BAKE_MAX_TILES)) {
    r.over = 1u;
    return r;
  }
  r.nm = (uint32_t) cm;
  r.nn = (uint32_t) cn;
  return r;
}

// the inside rule at tile (j, i) of the face -> inside; e0, e1 oriented (read when inside)
__host__ __device__ __forceinline__ bool bakeInside(const BakeFace &f, float sx, float sy, uint32_t j, uint32_t i, float &e0, float &e1)
{
  const float px = sx + (f.fm0 + (float) j), py = sy + (f.fn0 + (float) i);
  if (!(px >= f.bx0 && px <= f.bx1 && py >= f.by0 && py <= f.by1)) return false;
  const float x0 = f.t0x - px, y0 = f.t0y - py, x1 = f.t1x - px, y1 = f.t1y - py, x2 = f.t2x - px, y2 = f.t2y - py;
  float a = x1 * y2 - x2 * y1;
  float b = x2 * y0 - x0 * y2;
  float c = x0 * y1 - x1 * y0;
  if (f.d < 0.f) { a = -a; b = -b; c = -c; }
  e0 = a;
  e1 = b;
  return a >= 0.f && b >= 0.f && c >= 0.f;
}

// one texel against one face: the first inside tile, n outer, m inner
__host__ __device__ __forceinline__ bool bakeFaceCovers(const BakeFace &f, float sx, float sy, float &e0, float &e1)
{
  for (uint32_t i = 0; i < f.nn; ++i)
    for (uint32_t j = 0; j < f.nm; ++j)
      if (bakeInside(f, sx, sy, j, i, e0, e1)) return true;
  return false;
}

__host__ __device__ __forceinline__ BakeCorners bakeCorners(const BakeSource &src, uint32_t f)
{
  BakeCorners c;
  for (int q = 0; q < 3; ++q) {
    if (src.plane) {
      const uint32_t k = bakePlaneCorner(f, q);
      c.v[q] = F3(bakePlaneCoord(k, 0), bakePlaneCoord(k, 1), 0.f);
      c.n[q] = F3(0.f, 0.f, 1.f);
    } else {
      const qa_face &fc = src.faces[f];
      c.v[q] = ld3(src.vertices + 3 * (size_t) fc.v[q]);
      c.n[q] = ld3(src.normals + 3 * (size_t) fc.vn[q]);
    }
  }
  return c;
}

// what a covered texel holds: (a, b), and p and N in world space
__host__ __device__ __forceinline__ void bakeDetails(const BakeSource &src, const qa_instance *inst, int node, bool rootIdentity, uint32_t f, float d,
                                                     float e0, float e1, float &a, float &b, f3 &p, f3 &N)
{
  const float ad = d < 0.f ? -d : d;
  a = e0 / ad;
  b = e1 / ad;
  const float c = 1.f - a - b;
  const BakeCorners k = bakeCorners(src, f);
  p = (k.v[0] * a + k.v[1] * b) + k.v[2] * c;
  N = (k.n[0] * a + k.n[1] * b) + k.n[2] * c;
  for (int at = node; at >= 0; at = inst[at].parent) {
    if (at == 0 && rootIdentity) {
      N = normalize(N);
      break;
    }
    const qa_instance &in = inst[at];
    p = mulMV(in.tm, p) + ld3(in.pos);
    N = normalize(mulTMV(in.itm, N));
  }
}

struct BakePlanes {
  float *point, *normal;
  int32_t *face;
  float *bary;
};

__host__ __device__ __forceinline__ void bakeStore(const BakePlanes &o, size_t q, int32_t face, float a, float b, f3 p, f3 N)
{
  if (o.point) { o.point[3 * q] = p.x; o.point[3 * q + 1] = p.y; o.point[3 * q + 2] = p.z; }
  if (o.normal) { o.normal[3 * q] = N.x; o.normal[3 * q + 1] = N.y; o.normal[3 * q + 2] = N.z; }
  if (o.face) o.face[q] = face;
  if (o.bary) { o.bary[2 * q] = a; o.bary[2 * q + 1] = b; }
}

// one texel of the whole map, face after face (the host's loop; the kernel walks the same faces in chunks)
__host__ __device__ __forceinline__ void bakeTexel(const BakeSource &src, const qa_instance *inst, int node, bool rootIdentity, uint32_t ix, uint32_t iy,
                                                   uint32_t W, uint32_t H, const BakePlanes &o)
{
  float sx, sy;
  bakeSample(ix, iy, W, H, sx, sy);
  const size_t q = (size_t) iy * W + ix;
  for (uint32_t f = 0; f < src.numFaces; ++f) {
    const BakeFace bf = bakeFaceSetup(src, f);
    float e0, e1;
    if (!bf.nm || !bakeFaceCovers(bf, sx, sy, e0, e1)) continue;
    float a, b;
    f3 p, N;
    bakeDetails(src, inst, node, rootIdentity, f, bf.d, e0, e1, a, b, p, N);
    bakeStore(o, q, (int32_t) f, a, b, p, N);
    return;
  }
  bakeStore(o, q, -1, 0.f, 0.f, F3(0.f, 0.f, 0.f), F3(0.f, 0.f, 0.f));
}

// is any face of the source, void ones apart, spread over more tiles than the limit?
__host__ __device__ __forceinline__ bool bakeOverTiles(const BakeSource &src)
{
  for (uint32_t f = 0; f < src.numFaces; ++f)
    if (bakeFaceSetup(src, f).over) return true;
  return false;
}

// ---- gutter fill ----------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t bakeWrap(int v, uint32_t n)
{
  const int m = v % (int) n;
  return (uint32_t) (m < 0 ? m + (int) n : m);
}

// the offset (dx, dy) of the covered texel an uncovered one takes its bytes from -> found.  covered(dx, dy) answers for the
// neighbour at that offset (the kernel reads its LDS tile, the host the face plane)
template <class Covered>
__host__ __device__ __forceinline__ bool bakeDilatePick(int radius, const Covered &covered, int &bx, int &by)
{
  int best = 0x7FFFFFFF;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx) {
      const int d2 = dx * dx + dy * dy;
      if (d2 < best && covered(dx, dy)) { best = d2; bx = dx; by = dy; }
    }
  return best != 0x7FFFFFFF;
}

struct BakeFaceCovered {
  const int32_t *face;
  uint32_t x, y, W, H;
  __host__ __device__ bool operator()(int dx, int dy) const { return face[(size_t) bakeWrap((int) y + dy, H) * W + bakeWrap((int) x + dx, W)] >= 0; }
};

__host__ __device__ __forceinline__ void bakeDilateTexel(const uint8_t *rgb8, const int32_t *face, uint32_t W, uint32_t H, uint32_t radius, uint32_t x,
                                                         uint32_t y, uint8_t *out)
{
  const size_t q = (size_t) y * W + x;
  size_t from = q;
  if (face[q] < 0) {
    const BakeFaceCovered cov = {face, x, y, W, H};
    int dx = 0, dy = 0;
    if (bakeDilatePick((int) radius, cov, dx, dy)) from = (size_t) bakeWrap((int) y + dy, H) * W + bakeWrap((int) x + dx, W);
  }
  out[3 * q] = rgb8[3 * from];
  out[3 * q + 1] = rgb8[3 * from + 1];
  out[3 * q + 2] = rgb8[3 * from + 2];
}

}  // namespace qa
