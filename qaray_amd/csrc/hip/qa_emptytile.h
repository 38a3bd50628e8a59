// qa_emptytile.h — can NO camera ray of one 8x8 pixel tile meet anything?
//
// A frame wider than its subject has tiles whose every sample is background: the Cornell box at 16:9 leaves 42.7 % of its tiles
// beside the box.  Such a tile's result is known before its first sample - rgb = background, depth = QA_BIGFLOAT, ns = spp_min -
// and qa_integrate_lastcast writes it in closed form instead of tracing it (qa_kernel_lastcast_body.h, section A; option
// "empty_tiles").  Built on qa_tilecull.h's pyramid and shared by host and device in the same way: tests/cpp/empty_tile_check.cpp
// puts the answer against the walk's own gates, ray by ray.
//
// "Empty" is the statement that every camera ray of the tile fails the FIRST gate of every node that holds an object, which is
// where the reference's own sweep returns a miss for that node (so nothing behind the gate - hitMesh's rule for misses, a
// triangle's inside test - is ever reached).  For every node k >= 1 with an object, origin and window go through the node's chain
// exactly as buildTileLists takes them, and the pyramid, or its mirror image (the gates test lines: a mesh's slab test accepts a
// negative exit, and a conservative answer for planes and spheres costs nothing), is put against the node's bounds widened by
// what that intersector's own fp32 arithmetic can move its decision by:
//   * mesh: DMesh::bmin / bmax, the box hitMesh gates on (Box::IntersectRay).  Its slab products are off by a few ulps of the
//     coordinates involved, and a ray's node-space direction by a few ulps of the origin per level of the chain: what
//     TileCone::rel was sized for (250 ulps and the direction term), on |o| + |b|.  Axes the slab test may ignore for a ray of the
//     tile count as unbounded (TileCone::open).  No pad: the gate is the reference's own box, not an own tree's.
//   * plane: [-1, 1]^2 x {0}.  hitPlane accepts where the computed point p + t d has |x|, |y| <= 1: t = -p.z / d.z carries two
//     roundings, the product and the sum two more - a few ulps of |o| + 1 in all, inside rel * (|o| + 1) as above.  Its |d.z| < 1e-7
//     gate only turns hits into misses, so no axis is open.
//   * sphere: [-1, 1]^3.  hitSphere misses where delta = b b - 4 a c < 0 with a = d.d, b = 2 p.d, c = p.p - 1.  Exactly,
//     delta = 4 |d|^2 (1 - s^2) with s the line's distance from the centre; computed (u = 2^-24; P = |p|, D = |d|): the dot
//     products carry 3 u of their terms' sum, so b b is off by up to 4 * 7 u P^2 D^2, 4 a c by up to 4 * 8 u (P^2 + 1) D^2 (the
//     rounding of p.p - 3 u P^2 - and of the subtraction survive the product with 4 a) and the difference by u of the larger:
//     |error| <= 4 D^2 * 16 u (P^2 + 1).  A line is therefore certain to miss only when s^2 > 1 + 16 u (P^2 + 1): the sphere counts
//     with the radius sqrt(1 + x), x = 1.2e-5 (oAbs^2 + 1) >= 4 * 16 u (3 oAbs^2 + 1) - the term in the SQUARE of the origin's
//     distance that fastWalkPad has for the inside test.  A glow sphere of radius 0.01 at distance 5000 stands at 5e5 in its own
//     space: its discriminant cancels at 2.5e11, and the sphere the test must assume has a radius of some 1700 units, not 1; a slack
//     relative to |o| would be wrong by orders of magnitude the other way at distance 50.  rel * (|o| + 1 + pad) comes on top for
//     the direction, as for the others.  No axis is open.
// Not a number anywhere (an overflowing chain, a degenerate window) compares false in tileConeMeetsBox: "not out", never empty.
//
// Never empty, whatever the tile: a background component that is not finite (the mean of such samples is not the colour),
// more nodes than QA_EMPTY_TILE_NODES, a chain deeper than the walk follows; and, by the caller, launches without tile lists
// (RenderParams::tile_lists <= 0: depth of field, where the rays of a tile share no origin, among them).
#pragma once
#include "qa_tilecull.h"

// (what the shortcut costs and returns: profiles/empty_tiles_cost.txt; the run-time option "empty_tiles" turns it off)
#define QA_EMPTY_TILE_NODES 64   /* scenes of more nodes have no empty tile (a resident scene has at most QA_KARG_INST) */

namespace qa {

// What the unit sphere's radius must be taken as for an origin whose largest |coordinate| is oAbs, less 1: sqrt(1 + x) - 1
__host__ __device__ __forceinline__ float emptySpherePad(float oAbs)
{
  const float x = 1.2e-5f * (oAbs * oAbs + 1.f);
  return x / (qsqrt(1.f + x) + 1.f);
}

__host__ __device__ __forceinline__ bool emptyFinite(float v) { return (v - v) == 0.f; }

// S: inst(k) -> the scene-graph node, mesh(i) -> its DMesh (device: the kernel's tables, host: the built scene's).
// The tile whose first pixel is (X0, Y0); `cone`: 24 words of scratch (qa_integrate_lastcast: row 0 of the wave's stacks).
// Wave-uniform on the device: every lane asks the same question and writes the same words.
template <class S>
__host__ __device__ __forceinline__ bool tileIsEmpty(const S &s, const DCamera &cam, const float *background, int numInst, bool rootIdentity,
                                                      float X0, float Y0, TileCone *cone)
{
  if (numInst > QA_EMPTY_TILE_NODES) return false;
  if (!(emptyFinite(background[0]) && emptyFinite(background[1]) && emptyFinite(background[2]))) return false;
  TileLens lens;
  {
    f3 cW[4];
    tileWindow(ld3(cam.screenA), ld3(cam.screenU), ld3(cam.screenV), X0, Y0, cW);
    lens = tileLens(ld3(cam.pos), cW);
  }
  for (int k = 1; k < numInst; ++k) {
    const int type = s.inst(k).obj_type;
    if (type == QA_OBJ_NONE) continue;
    const int depth = s.inst(k).depth;
    if (depth > QA_MAX_NODE_DEPTH) return false;
    {
      // origin and window through the node chain (buildTileLists, qa_kernel.h: outermost level first)
      f3 o = ld3(cam.pos), c[4];
      tileWindow(ld3(cam.screenA), ld3(cam.screenU), ld3(cam.screenV), X0, Y0, c);
      for (int lvl = rootIdentity ? 1 : 0; lvl <= depth; ++lvl) {
        int a = k;
        for (int up = depth; up > lvl; --up) a = s.inst(a).parent;
        const qa_instance &in = s.inst(a);
        o = tileNodePoint(in, o);
        for (int i = 0; i < 4; ++i) c[i] = tileNodePoint(in, c[i]);
      }
#if defined(__HIP_DEVICE_COMPILE__)
      __builtin_amdgcn_wave_barrier();   // (the last node's test has read the pyramid)
#endif
      tileCone(lens, o, c, cone);
      if (type != QA_OBJ_MESH) cone->open = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" ::: "memory");     // read it back below: do not keep it in registers
#endif
    }
    f3 bmin, bmax;
    float pad = 0.f;
    if (type == QA_OBJ_MESH) {
      bmin = ld3(s.mesh(s.inst(k).mesh).bmin);
      bmax = ld3(s.mesh(s.inst(k).mesh).bmax);
    } else if (type == QA_OBJ_PLANE) {
      bmin = F3(-1.f, -1.f, 0.f);
      bmax = F3(1.f, 1.f, 0.f);
    } else {
      bmin = F3(-1.f, -1.f, -1.f);
      bmax = F3(1.f, 1.f, 1.f);
      pad = emptySpherePad(cone->oAbs);
    }
    float tLow;
    if (tileConeMeetsBox(cone, bmin, bmax, pad, &tLow)) return false;
  }
  return true;
}

}  // namespace qa
