// qa_kernel.h — the integrator: one persistent HIP kernel that runs qaray's whole per-pixel
// Monte-Carlo loop on gfx950.
//
// What it replaces (reference file:line): Renderer::ThreadRender/PixelRender
// (src/renderers/renderer.cpp:302-423), SuperSamplerHalton (src/scene/scene.cpp:83-123),
// Scene::TraceNodeNormal/TraceNodeShadow (src/scene/scene.cpp:35-74), Sphere/Plane/TriObj
// intersectors and the BVH walk (src/objects/objects.cpp:55-420), MtlBlinn_PhotonMap::Shade with
// MultiMtl dispatch (src/materials/MtlBlinn_PhotonMap.cpp:65-500, materials.h:70-76), the lights
// (src/lights/lights.cpp:39-144) and the xorshift32 sampler (src/samplers/Sampler_Marsaglia.cpp).
//
// Execution model (MI355X-first, not a translation of the CPU recursion):
//  * Persistent threads.  The grid is sized to what is resident on the chip; every LANE owns one
//    pixel at a time and runs a small state machine: [fetch pixel] -> [start sample: camera ray]
//    -> trace -> shade -> (next bounce | sample finished).  A finished path is replaced in the same
//    loop iteration by the pixel's next sample, a finished pixel by a new pixel pulled from a
//    global work counter with ONE atomic per wavefront (ballot + mbcnt prefix), so all 64 lanes of
//    a wave trace a ray in every iteration and no ray/hit queue ever goes through HBM: path state
//    lives in VGPRs, the BVH stack and (for scenes that fit) the whole scene image in LDS.
//  * The reference's recursion (Shade -> TraceNodeNormal -> Shade ...) is a chain, because exactly
//    one of reflect / transmit / diffuse is followed per hit; it is unrolled into an iteration
//    that carries a throughput.  Random numbers are drawn in the reference's order (select, lobe
//    sample, then the deeper hits); lights that draw random numbers (area lights) are evaluated by a
//    post-order replay of the path's hit log when the path ends (AREA kernel variants).
//  * BVH traversal is "while-while": a lane descends inner nodes until it holds a leaf, then the
//    wave intersects leaves together; the per-lane visiting order is exactly the reference's
//    (near child first, far child pushed), which decides ties between equal hit distances.
//  * One xorshift32 stream per pixel (include/qa_seed.h); a pixel's samples are sequential by
//    construction, pixels are the parallel dimension.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "qa_device_math.h"
#include "qa_scene_dev.h"
#include "qa_seed.h"
#include "qa_texture_dev.h"
#include "qa_tilecull.h"
#include "qa_emptytile.h"

namespace qa {

#ifndef QA_MIN_WAVES
#define QA_MIN_WAVES 4          /* waves per SIMD the register allocator must leave room for */
#endif
#define QA_BIAS 0.005f         /* src/objects/objects.cpp:19 */
#define QA_DX 0.01f            /* DiffRay::dx = dy, src/core/ray.cpp:31-32 */
// qa_integrate's DCounters are per LANE, reduced by shuffles at the end.  (-DQA_WAVE_TALLIES: the lanes that reach a tally add
// their number to a wave-uniform count in scalar registers instead - eight vector registers less on paper; measured on the
// Cornell-box kernel: 101 instead of 87 spilled registers and 12.4 instead of 13.1 Gsamples/s, profiles/round03/experiments.txt.
// qa_integrate_cs does tally per wave.)
#ifdef QA_WAVE_TALLIES
#define QA_TALLY(x) (x) += (unsigned long long) __popcll(__ballot(1))
#else
#define QA_LANE_TALLIES 1
#define QA_TALLY(x) (x)++
#endif

#ifdef QA_STAMPS
#define QA_T(var) const unsigned long long var = __builtin_readcyclecounter();
#define QA_TACC(dst, since)                                                                                  \
  {                                                                                                          \
    const unsigned long long d_ = __builtin_readcyclecounter() - (since);                                    \
    if ((int) __lane_id() == __ffsll((long long) __ballot(1)) - 1) dst += d_;                                \
  }
#else
#define QA_T(var)
#define QA_TACC(dst, since)
#endif

struct RayDiff { f3 dx, dy; };  // directions of the x / y differential rays (they share the origin)

struct Hit {
  float z;      // world-parametric distance (rays are not renormalised in node space)
  f3 p, N;      // node-local until traceClosest() maps them to world space
  int node;     // instance index, -1 = none
  int mtlID;
  bool front;
};

// Where the traversal reads the scene from: the LDS-resident image or global memory.
template <bool RES>
struct SceneMem {
  const uint4 *img;  // LDS image (RES) - unused otherwise
};

__device__ __forceinline__ float asF(uint32_t u) { return __uint_as_float(u); }

}  // namespace qa
#include "qa_photon_dev.h"   // needs QA_BLOCK and asF
namespace qa {

// Scene-graph nodes and mesh descriptors: resident scenes carry them BY VALUE in the kernel
// arguments (constant address space: wave-uniform indices become scalar loads into SGPRs, no
// vector-memory round trip on the critical path of every cast); larger scenes read the tables
// from global memory.
//
// The tables in global memory are read through the CONSTANT address space: no kernel writes them, and only then may
// the compiler turn a wave-uniform index into scalar loads (s_load into SGPRs: lower latency, no VGPRs for the
// matrices) - through a plain pointer out of DScene it cannot rule out that the frame's stores alias the table and
// issues one vector (flat) load per lane and field instead.  The record is returned by value; fields that are not
// used are never loaded.
template <class T>
__device__ __forceinline__ T ldTable(const T *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  // dword by dword: a whole-struct copy becomes one wide load, which the compiler keeps in the vector path when its
  // users are vector ALU operations
  static_assert(sizeof(T) % 4 == 0 && alignof(T) >= 4, "table records are made of dwords");
  const __attribute__((address_space(4))) uint32_t *w = (const __attribute__((address_space(4))) uint32_t *) p;
  T v;
  uint32_t *d = reinterpret_cast<uint32_t *>(&v);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i) d[i] = w[i];
  return v;
#else
  return *p;
#endif
}
// A pointer that comes out of such a record (DMesh::wnodes, wtris, ...) has no address space the compiler can see, and
// a load through it is a FLAT load: LDS or global decided per access at run time, and counted on both wait counters,
// so that it also waits for the LDS traffic of the traversal stack.  Where the pointer can only be global memory the
// load says so.
__device__ __forceinline__ uint4 ldGlobal(const uint4 *p);
// GMEM: the pointer is known to be global memory (non-resident scenes); otherwise a plain load (LDS image or unknown)
template <bool GMEM>
__device__ __forceinline__ uint4 ld16(const uint4 *p)
{
  if constexpr (GMEM) return ldGlobal(p);
  else return *p;
}
__device__ __forceinline__ uint4 ldGlobal(const uint4 *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  // (through the native vector type: uint4 is a class, and its copy would go back through a generic reference)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = *(const __attribute__((address_space(1))) u32x4 *) p;
  return make_uint4(v.x, v.y, v.z, v.w);
#else
  return *p;
#endif
}
template <bool RES>
__device__ __forceinline__ std::conditional_t<RES, const qa_instance &, qa_instance> instAt(const DScene &sc, int k)
{
  if constexpr (RES) return sc.instv[k];
  else return ldTable(sc.inst + k);
}
template <bool RES>
__device__ __forceinline__ std::conditional_t<RES, const DMesh &, DMesh> meshAt(const DScene &sc, int k)
{
  if constexpr (RES) return sc.meshv[k];
  else return ldTable(sc.mesh + k);
}

// ---------------------------------------------------------------------------------------------
// RNG: Sampler_Marsaglia::xorshift32 (src/samplers/Sampler_Marsaglia.cpp:43-53)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float rng1(uint32_t &state)
{
  uint32_t x = state;
  x ^= x << 13;
  x ^= x >> 17;
  x ^= x << 5;
  state = x;
  return (float) x / 4294967296.0f;
}

// Sampler::UniformBall (src/core/sampler.cpp:42-53); z uses r2 like the reference
__device__ __forceinline__ f3 uniformBall(uint32_t &rng, float radius)
{
  f3 p;
  do {
    const float r1 = rng1(rng), r2 = rng1(rng);
    (void) rng1(rng);
    p.x = (2.f * r1 - 1.f) * radius;
    p.y = (2.f * r2 - 1.f) * radius;
    p.z = (2.f * r2 - 1.f) * radius;
  } while (length(p) > radius);
  return p;
}

// TransformToLocalFrame (src/math/math.cpp:37-46)
__device__ __forceinline__ f3 toLocalFrame(f3 N, f3 sample)
{
  const f3 Z = N;
  const f3 Y = (qabs(Z.x) > qabs(Z.y)) ? normalize(F3(Z.z, 0, -Z.x)) : normalize(F3(0, -Z.z, Z.y));
  const f3 X = normalize(cross(Y, Z));
  const f3 unit = normalize(sample);
  return (X * unit.x + Y * unit.y) + Z * unit.z;
}

// ---------------------------------------------------------------------------------------------
// Node transforms (src/core/node.cpp:112-139, src/core/transform.h:47-61)
// ---------------------------------------------------------------------------------------------
// (toNode: qa_tilecull.h)

// Node::ToNodeCoords(DiffRay) (src/core/node.cpp:119-126) for the x / y rays: same origin as the
// central ray, so only the direction needs its own transform.  `before` is the central ray before
// this level, `afterP` its origin after it.
__device__ __forceinline__ f3 toNodeDir(const qa_instance &in, f3 beforeP, f3 afterP, f3 dir)
{
  return mulMV(in.itm, (beforeP + dir) - ld3(in.pos)) - afterP;
}
template <bool RES>
__device__ __forceinline__ void localRayDiff(const DScene &sc, int k, const Ray &world, const RayDiff &wd, Ray &r, RayDiff &rd)
{
  // root level
  Ray cur;
  RayDiff cd;
  if (sc.rootIdentity) {
    cur.p = world.p;
    cur.d = (world.p + world.d) - world.p;
    cd.dx = (world.p + wd.dx) - world.p;
    cd.dy = (world.p + wd.dy) - world.p;
  } else {
    cur = toNode(instAt<RES>(sc, 0), world);
    cd.dx = toNodeDir(instAt<RES>(sc, 0), world.p, cur.p, wd.dx);
    cd.dy = toNodeDir(instAt<RES>(sc, 0), world.p, cur.p, wd.dy);
  }
  int chain[QA_MAX_NODE_DEPTH];
  int n = 0;
  for (int a = k; a > 0 && n < QA_MAX_NODE_DEPTH; a = instAt<RES>(sc, a).parent) chain[n++] = a;
  for (int q = n - 1; q >= 0; --q) {
    const qa_instance &in = instAt<RES>(sc, chain[q]);
    const Ray nx = toNode(in, cur);
    cd.dx = toNodeDir(in, cur.p, nx.p, cd.dx);
    cd.dy = toNodeDir(in, cur.p, nx.p, cd.dy);
    cur = nx;
  }
  r = cur;
  rd = cd;
}

// The root node of a qaray scene never carries a transform (Node::Init, src/core/node.cpp:41-48):
// tm = itm = I, pos = 0.  Multiplying by the identity and subtracting zero return their operand
// (up to the sign of a zero), so Node::ToNodeCoords at the root reduces to dir' = (p + dir) - p,
// whose two roundings are what the reference performs and must be kept.
template <bool RES>
__device__ __forceinline__ Ray rootRay(const DScene &sc, const Ray &world)
{
  if (!sc.rootIdentity) return toNode(instAt<RES>(sc, 0), world);
  Ray o;
  o.p = world.p;
  o.d = (world.p + world.d) - world.p;
  return o;
}

// Local ray of instance k: the root's transform has already been applied (r0); walk the rest of
// the ancestor chain top-down.  All lanes work on the same k, so the chain is wave-uniform.
template <bool RES>
__device__ __forceinline__ Ray localRay(const DScene &sc, int k, const Ray &r0)
{
  const int depth = instAt<RES>(sc, k).depth;
  if (depth == 1) return toNode(instAt<RES>(sc, k), r0);
  int chain[QA_MAX_NODE_DEPTH];
  int n = 0;
  for (int a = k; a > 0 && n < QA_MAX_NODE_DEPTH; a = instAt<RES>(sc, a).parent) chain[n++] = a;
  Ray r = r0;
  for (int q = n - 1; q >= 0; --q) r = toNode(instAt<RES>(sc, chain[q]), r);
  return r;
}

// The same for the instance loops of global-memory scenes, which visit the nodes in pre-order: the children of a group
// follow each other, so the group's own local ray is kept from one sibling to the next instead of being rebuilt from
// the root for every child (five walls in one group: five times).  The chain is evaluated top-down either way - the
// same operations on the same operands.  (Resident kernels keep localRay: their scenes are flat, and the six registers
// of the kept ray are what the Cornell-box kernel does not have.)
struct GroupRay { int node; Ray ray; };
template <bool RES>
__device__ __forceinline__ Ray localRayInGroup(const DScene &sc, int k, const Ray &r0, GroupRay &g)
{
  if constexpr (RES) return localRay<RES>(sc, k, r0);
  else {
    const qa_instance &in = instAt<RES>(sc, k);
    if (in.depth == 1) return toNode(in, r0);
    if (in.parent != g.node) {
      g.ray = localRay<RES>(sc, in.parent, r0);
      g.node = in.parent;
    }
    return toNode(in, g.ray);
  }
}

// ---------------------------------------------------------------------------------------------
// Intersectors.  `closest` = false is a shadow query (diffray == NULL in the reference): only
// h.z is maintained and the caller stops at the first hit.
// ---------------------------------------------------------------------------------------------
// Sphere::IntersectRay (src/objects/objects.cpp:55-141)
__device__ __forceinline__ bool hitSphere(const Ray &ray, Hit &h, int k, bool closest)
{
  const float a = dot(ray.d, ray.d);
  const float b = 2.f * dot(ray.p, ray.d);
  const float c = dot(ray.p, ray.p) - 1;
  const float rcp2a = 1.f / (2.f * a);
  const float delta = b * b - 4 * a * c;
  float t = QA_BIGFLOAT;
  if (delta < 0) return false;
  if (delta == 0) {
    const float t0 = -b * rcp2a;
    if (t0 <= QA_BIAS) return false;
    t = t0;
  } else {
    const float sq = qsqrt(delta);
    const float t1 = (-b - sq) * rcp2a;
    const float t2 = (-b + sq) * rcp2a;
    if (t1 <= QA_BIAS && t2 <= QA_BIAS) return false;
    else if (t1 > QA_BIAS) t = qmin(t, t1);
    else if (t2 > QA_BIAS) t = qmin(t, t2);
  }
  if (h.z > t) {
    h.z = t;
    if (closest) {
      const f3 p = ray.p + ray.d * t;
      const f3 N = normalize(p);
      h.p = p;
      h.N = N;
      h.front = (dot(N, ray.d) <= 0);
      h.node = k;
    }
    return true;
  }
  return false;
}

// Plane::IntersectRay (src/objects/objects.cpp:149-208)
__device__ __forceinline__ bool hitPlane(const Ray &ray, Hit &h, int k, bool closest)
{
  const f3 N = F3(0, 0, 1);
  const float dz = dot(ray.d, N);
  if (qabs(dz) < 1e-7f) return false;
  const float pz = dot(ray.p, N);
  const float t = -pz / dz;
  if (t <= QA_BIAS) return false;
  if (h.z > t) {
    const f3 p = ray.p + ray.d * t;
    if (qabs(p.x) > 1.f || qabs(p.y) > 1.f) return false;
    h.z = t;
    if (closest) {
      h.p = p;
      h.N = N;
      h.front = (dot(N, ray.d) <= 0);
      h.node = k;
    }
    return true;
  }
  return false;
}

// (slab, one axis of the slab test: qa_tilecull.h)
__device__ __forceinline__ void boxEntryExit(const Ray &ray, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const f3 p0 = (-(ray.p - bmin)) * drcp;
  const f3 p1 = (-(ray.p - bmax)) * drcp;
  f3 t0, t1;
  slab(ray.d.x, p0.x, p1.x, t0.x, t1.x);
  slab(ray.d.y, p0.y, p1.y, t0.y, t1.y);
  slab(ray.d.z, p0.z, p1.z, t0.z, t1.z);
  entry = qmax(t0.x, qmax(t0.y, t0.z));
  exit_ = qmin(t1.x, qmin(t1.y, t1.z));
}

// Fast slab test for rays whose direction has no near-zero component (|d| >= 1e-7 on every axis,
// the reference's threshold): then every product below is finite and not NaN, and the reference's
// MIN/MAX macros return the same VALUES as the hardware min/max instructions (they can only differ
// in the sign of a zero, which the comparisons that consume entry/exit cannot see).
// -(p - b) and (b - p) are the same number up to the sign of zero for the same reason.
__device__ __forceinline__ void boxEntryExitFast(const Ray &ray, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const f3 p0 = (bmin - ray.p) * drcp;
  const f3 p1 = (bmax - ray.p) * drcp;
  entry = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(p0.x, p1.x), __builtin_fminf(p0.y, p1.y)), __builtin_fminf(p0.z, p1.z));
  exit_ = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(p0.x, p1.x), __builtin_fmaxf(p0.y, p1.y)), __builtin_fmaxf(p0.z, p1.z));
}

// Slab tests of the library's own tree: the box is widened by `pad` on every side (folded into two
// copies of the ray origin, so the widening costs nothing per box).  Any conservative form will do
// here - these tests only decide where the own tree is searched, never what the reference accepts.
// (boxEntryExitPadFast, boxEntryExitPad: qa_tilecull.h - the host check of the tile lists runs the same text)

// TriObj::IntersectTriangle (src/objects/objects.cpp:212-306) on a precomputed 48-byte record
// (three 16-byte words q0..q2, see DTri).  TriangleArea(axis, P, Q, R) =
// (Q.u-P.u)*(R.v-P.v) - (R.u-P.u)*(Q.v-P.v) with (u,v) the two coordinates kept after dropping
// `axis` (objects.cpp:30-41).  Written without early exits: in a 64-wide wave some lane almost
// always survives each of the reference's five rejections, so the branches only cost; every
// quantity is a pure function of the inputs, and the accept condition is the conjunction of the
// reference's tests in its own order (a rejected test's later values are simply ignored).
__device__ __forceinline__ bool hitTriangle(const uint4 q0, const uint4 q1, const uint4 q2, const Ray &ray, Hit &h,
                                            float &ba, float &bb)
{
  const f3 N = F3(asF(q0.x), asF(q0.y), asF(q0.z));
  const f3 A = F3(asF(q0.w), asF(q1.x), asF(q1.y));
  const float dz = dot(ray.d, N);
  const float pz = dot(ray.p - A, N);
  const float t = -pz / dz;
  bool ok = !(qabs(dz) < 1e-7f) && !(t <= QA_BIAS) && (h.z > t);
  const uint32_t axis = q2.w;
  const f3 p = ray.p + ray.d * t;
  const bool ax0 = (axis == 0), ax2 = (axis == 2);
  const float pu = ax0 ? p.y : p.x;
  const float pv = ax2 ? p.y : p.z;
  const float au = ax0 ? A.y : A.x;
  const float av = ax2 ? A.y : A.z;
  const float bu = asF(q1.z), bv = asF(q1.w), cu = asF(q2.x), cv = asF(q2.y), s = asF(q2.z);
  const float a = ((bu - pu) * (cv - pv) - (cu - pu) * (bv - pv)) * s;
  const float b = ((cu - pu) * (av - pv) - (au - pu) * (cv - pv)) * s;
  const float c = 1.f - a - b;
  ok = ok && !(a < 0 || b < 0 || c < 0);
  if (ok) {
    h.z = t;
    h.p = p;
    h.front = (dz <= 0);
    ba = a;
    bb = b;
  }
  return ok;
}

// The same test reduced to what the traversal itself needs: accept / reject and the distance.
// The hit point, facing and barycentrics of the finally accepted triangle are recomputed once per
// mesh by triangleDetails() with the very same expressions (t is the stored h.z), instead of being
// carried through seven conditional moves on every one of the ~20 tests of a cast.
__device__ __forceinline__ bool hitTriangleZ(const uint4 q0, const uint4 q1, const uint4 q2, const Ray &ray, float &hz)
{
  const f3 N = F3(asF(q0.x), asF(q0.y), asF(q0.z));
  const f3 A = F3(asF(q0.w), asF(q1.x), asF(q1.y));
  const float dz = dot(ray.d, N);
  const float pz = dot(ray.p - A, N);
  const float t = -pz / dz;
  bool ok = !(qabs(dz) < 1e-7f) && !(t <= QA_BIAS) && (hz > t);
  const uint32_t axis = q2.w;
  const f3 p = ray.p + ray.d * t;
  const bool ax0 = (axis == 0), ax2 = (axis == 2);
  const float pu = ax0 ? p.y : p.x;
  const float pv = ax2 ? p.y : p.z;
  const float au = ax0 ? A.y : A.x;
  const float av = ax2 ? A.y : A.z;
  const float bu = asF(q1.z), bv = asF(q1.w), cu = asF(q2.x), cv = asF(q2.y), s = asF(q2.z);
  const float a = ((bu - pu) * (cv - pv) - (cu - pu) * (bv - pv)) * s;
  const float b = ((cu - pu) * (av - pv) - (au - pu) * (cv - pv)) * s;
  const float c = 1.f - a - b;
  ok = ok && !(a < 0 || b < 0 || c < 0);
  if (ok) hz = t;
  return ok;
}
// The same test on the library's own tree: the accept rule is unchanged, and `tie` is raised when a
// triangle passes everything but arrives at exactly the distance already held - the one situation
// in which the order of the tests decides who wins (hitMesh then repeats the query in the
// reference's order).
// PACKED: the record comes from DMesh::wtris (element id above the 2-bit axis).
template <bool PACKED = false>
__device__ __forceinline__ bool hitTriangleZTie(const uint4 q0, const uint4 q1, const uint4 q2, const Ray &ray, float &hz, bool &tie)
{
  const f3 N = F3(asF(q0.x), asF(q0.y), asF(q0.z));
  const f3 A = F3(asF(q0.w), asF(q1.x), asF(q1.y));
  const float dz = dot(ray.d, N);
  const float pz = dot(ray.p - A, N);
  const float t = -pz / dz;
  const bool pre = !(qabs(dz) < 1e-7f) && !(t <= QA_BIAS);
  const uint32_t axis = PACKED ? (q2.w & 3u) : q2.w;
  const f3 p = ray.p + ray.d * t;
  const bool ax0 = (axis == 0), ax2 = (axis == 2);
  const float pu = ax0 ? p.y : p.x;
  const float pv = ax2 ? p.y : p.z;
  const float au = ax0 ? A.y : A.x;
  const float av = ax2 ? A.y : A.z;
  const float bu = asF(q1.z), bv = asF(q1.w), cu = asF(q2.x), cv = asF(q2.y), s = asF(q2.z);
  const float a = ((bu - pu) * (cv - pv) - (cu - pu) * (bv - pv)) * s;
  const float b = ((cu - pu) * (av - pv) - (au - pu) * (cv - pv)) * s;
  const float c = 1.f - a - b;
  const bool inside = pre && !(a < 0 || b < 0 || c < 0);
  const bool ok = inside && (hz > t);
  tie = tie || (inside && hz == t);
  if (ok) hz = t;
  return ok;
}
__device__ __forceinline__ void triangleDetails(const uint4 q0, const uint4 q1, const uint4 q2, const Ray &ray, Hit &h,
                                                float &ba, float &bb)
{
  const f3 N = F3(asF(q0.x), asF(q0.y), asF(q0.z));
  const f3 A = F3(asF(q0.w), asF(q1.x), asF(q1.y));
  const float dz = dot(ray.d, N);
  const float t = h.z;
  const uint32_t axis = q2.w;
  const f3 p = ray.p + ray.d * t;
  const bool ax0 = (axis == 0), ax2 = (axis == 2);
  const float pu = ax0 ? p.y : p.x;
  const float pv = ax2 ? p.y : p.z;
  const float au = ax0 ? A.y : A.x;
  const float av = ax2 ? A.y : A.z;
  const float bu = asF(q1.z), bv = asF(q1.w), cu = asF(q2.x), cv = asF(q2.y), s = asF(q2.z);
  ba = ((bu - pu) * (cv - pv) - (cu - pu) * (bv - pv)) * s;
  bb = ((cu - pu) * (av - pv) - (au - pu) * (cv - pv)) * s;
  h.p = p;
  h.front = (dz <= 0);
}

// TriObj::IntersectRay + TraceBVHNode (src/objects/objects.cpp:310-420).  The traversal stack
// holds node DATA words (leaf flag + range, or child index) instead of ids: the word arrives with
// the node's box when the parent tests its two children, so an inner visit is a single 64-byte
// read of the sibling pair.
struct TriPick { uint32_t tri; float a, b; };  // accepted triangle (element order) and its barycentrics

// One BVH walk.  FAST = false: the reference's tree and rules - near child first, far child stacked,
// strict tests (entry < t_max, entry < exit), a leaf's triangles in element order, first accepted
// wins at equal distance (objects.cpp:342-419).  FAST = true: the library's own tree (qa_fastbvh.h)
// with non-strict box tests, and `tie` is raised when a triangle passes the inside test at exactly
// the distance already held.  Returns whether a triangle was accepted; best = its element index in
// the walked tree's order.  closest = false stops at the first accepted triangle.
// STRIDE: distance between a lane's stack entries (QA_BLOCK: the per-lane columns of the LDS stacks; 1: a private array).
// FMA (FAST only): the fast slab step in its one-fma-per-plane form (boxEntryExitPadFma, qa_tilecull.h).  A flag, because the shared
// text costs the lit and textured resident variants 7 - 50 spilled registers (profiles/cast_cost.txt): theirs is the old form.
template <bool FAST, bool STATS, bool GMEM = false, int STRIDE = QA_BLOCK, bool FMA = false>
__device__ __forceinline__ bool walkBVH(const uint4 *nodes, const uint4 *tris, uint32_t rootData, const Ray &ray, f3 drcp,
                                        bool fastSlab, float &hz, bool closest, uint32_t *stack, DCounters &cnt,
                                        uint32_t &best, bool &tie, float pad = 0.f)
{
  // FAST only: the origin moved by the pad; in the fast form the ray's share of a plane distance instead (slabRayTerm, qa_tilecull.h)
  f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
  if (FAST && FMA && fastSlab) { pLo = slabRayTerm(pLo, drcp); pHi = slabRayTerm(pHi, drcp); }
  bool hasHit = false;
  int sp = 0;
  uint32_t cur = rootData;
  while (cur != QA_DONE) {
    // ---- descend inner nodes until this lane holds a leaf (or runs out of work) --------------
    while (!(cur & QA_BVH_LEAF_BIT)) {
      if (STATS) QA_TALLY(cnt.bvh_nodes);
      const uint4 *pair = nodes + 2 * (size_t) (cur & QA_BVH_CHILD_MASK);
      const uint4 a0 = ld16<GMEM>(pair), a1 = ld16<GMEM>(pair + 1), b0 = ld16<GMEM>(pair + 2), b1 = ld16<GMEM>(pair + 3);
      float entry0, exit0, entry1, exit1;
      const f3 min0 = F3(asF(a0.x), asF(a0.y), asF(a0.z)), max0 = F3(asF(a0.w), asF(a1.x), asF(a1.y));
      const f3 min1 = F3(asF(b0.x), asF(b0.y), asF(b0.z)), max1 = F3(asF(b0.w), asF(b1.x), asF(b1.y));
      if constexpr (FAST) {
        if (fastSlab) {
          if constexpr (FMA) {
            boxEntryExitPadFma(pLo, pHi, drcp, min0, max0, entry0, exit0);
            boxEntryExitPadFma(pLo, pHi, drcp, min1, max1, entry1, exit1);
          } else {
            boxEntryExitPadFast(pLo, pHi, drcp, min0, max0, entry0, exit0);
            boxEntryExitPadFast(pLo, pHi, drcp, min1, max1, entry1, exit1);
          }
        } else {
          boxEntryExitPad(pLo, pHi, ray.d, drcp, min0, max0, entry0, exit0);
          boxEntryExitPad(pLo, pHi, ray.d, drcp, min1, max1, entry1, exit1);
        }
      } else if (fastSlab) {
        boxEntryExitFast(ray, drcp, min0, max0, entry0, exit0);
        boxEntryExitFast(ray, drcp, min1, max1, entry1, exit1);
      } else {
        boxEntryExit(ray, drcp, min0, max0, entry0, exit0);
        boxEntryExit(ray, drcp, min1, max1, entry1, exit1);
      }
      const float t_max = hz;
      const bool hit0 = FAST ? (entry0 <= t_max && entry0 <= exit0) : (entry0 < t_max && entry0 < exit0);
      const bool hit1 = FAST ? (entry1 <= t_max && entry1 <= exit1) : (entry1 < t_max && entry1 < exit1);
      const uint32_t d0 = a1.z, d1 = b1.z;
      if (hit0 && hit1) {
        // the reference pushes the far child, then the near one, and pops the near one next
        const bool nearFirst = entry0 < entry1;
        stack[(sp++) * STRIDE] = nearFirst ? d1 : d0;
        cur = nearFirst ? d0 : d1;
      } else if (hit0) cur = d0;
      else if (hit1) cur = d1;
      else cur = sp ? stack[(--sp) * STRIDE] : QA_DONE;
    }
    if (cur == QA_DONE) break;
    // ---- leaf: its triangles in element order -----------------------------------------------
    if (STATS) QA_TALLY(cnt.bvh_nodes);
    const uint32_t count = ((cur >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1;
    const uint32_t first = cur & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i) {
      if (STATS) QA_TALLY(cnt.tri_tests);
      const uint4 *t = tris + 3 * (size_t) (first + i);
      const uint4 t2 = ld16<GMEM>(t + 2);
      bool accepted;
      if constexpr (FAST) accepted = hitTriangleZTie<true>(ld16<GMEM>(t), ld16<GMEM>(t + 1), t2, ray, hz, tie);
      else accepted = hitTriangleZ(ld16<GMEM>(t), ld16<GMEM>(t + 1), t2, ray, hz);
      if (accepted) {
        hasHit = true;
        best = FAST ? (t2.w >> 2) : first + i;   // own tree: element | reference leaf << 15 (DMesh::ftris)
        if (!closest) return true;
      }
    }
    cur = sp ? stack[(--sp) * STRIDE] : QA_DONE;
  }
  return hasHit;
}

// The four children of a DWideNode (qa_scene_dev.h, its 4 x 16 bytes in q0..q3) against a ray whose origin has been
// split into pLo / pHi (origin -/+ pad: the boxes widened by `pad`): K = entry distance of child c, or +inf when the
// ray misses it, the slot is empty or the box lies beyond hz; W = its child word.  Boxes are decoded with one fma per
// plane - conservative by construction (quantised outwards, checked by the builder with the same fma).
#define QA_WIDE_BYTE(X, C) ((float) (((X) >> (8 * (C))) & 0xFFu))
#define QA_WIDE_CHILD(K, W, C)                                                                                                       \
  {                                                                                                                                  \
    const f3 lo = F3(__builtin_fmaf(QA_WIDE_BYTE(q1.z, C), asF(q0.w), asF(q0.x)), __builtin_fmaf(QA_WIDE_BYTE(q1.w, C), asF(q1.x), asF(q0.y)), \
                     __builtin_fmaf(QA_WIDE_BYTE(q2.x, C), asF(q1.y), asF(q0.z)));                                                   \
    const f3 hi = F3(__builtin_fmaf(QA_WIDE_BYTE(q2.y, C), asF(q0.w), asF(q0.x)), __builtin_fmaf(QA_WIDE_BYTE(q2.z, C), asF(q1.x), asF(q0.y)), \
                     __builtin_fmaf(QA_WIDE_BYTE(q2.w, C), asF(q1.y), asF(q0.z)));                                                   \
    const f3 p0 = (lo - pLo) * drcp, p1 = (hi - pHi) * drcp;                                                                         \
    const float en = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(p0.x, p1.x), __builtin_fminf(p0.y, p1.y)), __builtin_fminf(p0.z, p1.z)); \
    const float ex = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(p0.x, p1.x), __builtin_fmaxf(p0.y, p1.y)), __builtin_fmaxf(p0.z, p1.z)); \
    K = (W != QA_DONE && en <= hz && en <= ex) ? en : INF;                                                                           \
  }
#define QA_WIDE_CE(KA, WA, KB, WB)  \
  {                                 \
    const bool sw = KA > KB;        \
    const float tk = sw ? KB : KA;  \
    KB = sw ? KA : KB;              \
    KA = tk;                        \
    const uint32_t tw = sw ? WB : WA; \
    WB = sw ? WA : WB;              \
    WA = tw;                        \
  }
// all four children, sorted by entry distance (missed ones last, K = +inf)
#define QA_WIDE_NODE(q0, q1, q2, q3)                          \
  float k0, k1, k2, k3;                                       \
  uint32_t w0 = q3.x, w1 = q3.y, w2 = q3.z, w3 = q3.w;        \
  QA_WIDE_CHILD(k0, w0, 0)                                    \
  QA_WIDE_CHILD(k1, w1, 1)                                    \
  QA_WIDE_CHILD(k2, w2, 2)                                    \
  QA_WIDE_CHILD(k3, w3, 3)                                    \
  QA_WIDE_CE(k0, w0, k1, w1)                                  \
  QA_WIDE_CE(k2, w2, k3, w3)                                  \
  QA_WIDE_CE(k0, w0, k2, w2)                                  \
  QA_WIDE_CE(k1, w1, k3, w3)                                  \
  QA_WIDE_CE(k1, w1, k2, w2)

// One walk of the library's 4-wide tree (qa_widebvh.h).  Boxes are widened by `pad` (folded into two copies of the
// origin) and tested non-strictly, so every triangle the reference's inside test can accept at or before the distance
// held is tested; children are entered nearest first.  `tris` = DMesh::wtris (leaf order, element id in the axis
// word); `best` returns the element.  `tie` is raised when a triangle passes the inside test at exactly the
// distance already held.  closest = false stops at the first accepted triangle.  `stack`: LDS, stride QA_BLOCK,
// `cap` entries - on overflow `tie` is raised too (the caller then repeats the query on the reference tree).
__device__ __forceinline__ bool walkWide(const uint4 *wn, const uint4 *tris, uint32_t rootWord, const Ray &ray, f3 drcp, float pad,
                                         float &hz, bool closest, uint32_t *stack, uint32_t cap, uint32_t &best, bool &tie)
{
  const f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
  const float INF = __builtin_inff();
  bool hasHit = false;
  uint32_t sp = 0;
  uint32_t cur = rootWord;
  while (cur != QA_DONE) {
    while (!(cur & QA_BVH_LEAF_BIT)) {
      const uint4 *nd = wn + 4 * (size_t) cur;
      const uint4 q0 = ldGlobal(nd), q1 = ldGlobal(nd + 1), q2 = ldGlobal(nd + 2), q3 = ldGlobal(nd + 3);
      QA_WIDE_NODE(q0, q1, q2, q3)
      // nearest child next, the others stacked farthest first
      if (k3 < INF) { if (sp < cap) stack[(sp++) * QA_BLOCK] = w3; else tie = true; }
      if (k2 < INF) { if (sp < cap) stack[(sp++) * QA_BLOCK] = w2; else tie = true; }
      if (k1 < INF) { if (sp < cap) stack[(sp++) * QA_BLOCK] = w1; else tie = true; }
      if (k0 < INF) cur = w0;
      else cur = sp ? stack[(--sp) * QA_BLOCK] : QA_DONE;
    }
    if (cur == QA_DONE) break;
    const uint32_t count = ((cur >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1;
    const uint32_t first = cur & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i) {
      const uint4 *t = tris + 3 * (size_t) (first + i);
      const uint4 t2 = ldGlobal(t + 2);
      if (hitTriangleZTie<true>(ldGlobal(t), ldGlobal(t + 1), t2, ray, hz, tie)) {
        hasHit = true;
        best = t2.w >> 2;               // element (the reference's triangle order)
        if (!closest) return true;
      }
    }
    cur = sp ? stack[(--sp) * QA_BLOCK] : QA_DONE;
  }
  return hasHit;
}

// May this ray be searched with a pruned walk of mesh m?  The reference's inside test can accept, by cancellation of
// its 2-D areas, a point farther than DMesh::cancelDist (qa_widebvh.h ComputeMeshSlack) from a triangle.  A pruned
// search goes wrong only if such a "hit" lies before the triangle's leaf box on the ray, i.e. on the segment from the
// origin to the mesh bounds - which is never farther from any triangle than the origin's farthest corner of the
// bounds, or the bounds' diagonal.
template <class M>
__device__ __forceinline__ bool insideCancelReach(const M &m, f3 o)
{
  const f3 bmin = ld3(m.bmin), bmax = ld3(m.bmax);
  const f3 f = F3(qmax(qabs(o.x - bmin.x), qabs(o.x - bmax.x)), qmax(qabs(o.y - bmin.y), qabs(o.y - bmax.y)), qmax(qabs(o.z - bmin.z), qabs(o.z - bmax.z)));
  const f3 dg = bmax - bmin;
  const float reach2 = qmax(dot(f, f), dot(dg, dg));
  return reach2 * 1.0001f < m.cancelDist * m.cancelDist;
}

// Would the reference's walk have reached the leaf `leaf` of its tree?  It enters a node when the
// strict box test passes against the distance held at that moment.  Every inner box of the tree is
// the union of its children's boxes (min / max of the same floats), and the slab arithmetic is
// monotone in the box bounds, so an ancestor's [entry, exit] interval contains the leaf's: if the
// LEAF's box passes the strict test against `limit`, every node above it does.  `limit` is the
// fixed t_max for an any-hit query (exact).  DTriShade::pad holds an element's leaf id.
// atFound (closest-hit queries in which no tie was seen): `limit` is the distance t just found, and
// the leaf passes with entry <= t (refLeafReached, qa_tilecull.h), because the reference held more
// than t when it tested that box:
//   * let X be the closest accepted triangle, at t.  The own search tests every triangle whose padded
//     leaf the ray enters at entry <= the distance held (the tile lists by their h.z >= bound rule),
//     X's and that of any other triangle the inside test accepts at t among them: a second triangle
//     accepted at exactly t would have raised `tie`, whichever of the two came first;
//   * the reference's running t_max starts above t (X was accepted against it) and falls only to
//     distances of accepted triangles: none is below t (X is the closest), none equals t (no tie).
//     So until the reference accepts X itself, its t_max is strictly larger than t;
//   * the reference tests a child's box when it visits the parent and never again when it pops the
//     child, and it visits X's leaf before it accepts X: the leaf's box, with entry == t, met
//     entry < t_max.  The ancestors' entries are not larger and their exits not smaller, and they
//     were tested earlier, against a t_max at least as large: they pass as well.
// An entry that exceeds t (by the rounding of the slab products: the triangle's plane is a face of a
// flat leaf box) still fails, and the lane repeats the query.
template <bool GMEM = false>
__device__ __forceinline__ bool refReaches(const uint4 *nodes, uint32_t leaf, const Ray &ray, f3 drcp, bool fastSlab, float limit, bool atFound = false)
{
  if (leaf <= 1) return true;   // the root is entered unconditionally (the mesh bounds were tested by the caller)
  const uint4 n0 = ld16<GMEM>(nodes + 2 * (size_t) leaf), n1 = ld16<GMEM>(nodes + 2 * (size_t) leaf + 1);
  float entry, exit_;
  const f3 bmin = F3(asF(n0.x), asF(n0.y), asF(n0.z)), bmax = F3(asF(n0.w), asF(n1.x), asF(n1.y));
  if (fastSlab) boxEntryExitFast(ray, drcp, bmin, bmax, entry, exit_);
  else boxEntryExit(ray, drcp, bmin, bmax, entry, exit_);
  return refLeafReached(entry, exit_, limit, atFound);
}

// TriObj::IntersectRay + TraceBVHNode (src/objects/objects.cpp:310-420).
//
// The closest hit of a mesh does not depend on the tree it is searched with - except where the
// reference's own search is not exhaustive: it enters a child box only on strict inequalities (a
// flat box is never entered), and at equal distance it keeps the triangle it met first.  Counting
// kernels (STATS) therefore walk the reference's tree exactly as the reference does.  The others
// walk the library's SAH tree (qa_fastbvh.h: two triangles per leaf, padded boxes, non-strict
// tests, so that it reaches every triangle the reference can reach; 2.7 instead of 15 triangle
// tests per cast on the Cornell box) and then check the answer against the reference's rules:
// the found triangle must be reachable in the reference's tree (refReaches) and no tie may have
// been seen; otherwise the lane repeats the query on the reference's tree.
// TL: `tileList` may point at the wave's tile lists (qa_tilecull.h; qa_integrate, section A), `listHdr` is this node's header word
// there (0: none) and `primary` says which lanes hold a camera ray: where the node has a list, those lanes test the listed
// leaves' triangles instead of walking the own tree.
template <bool RES, bool STATS, bool TL = false>
__device__ __forceinline__ bool hitMesh(const SceneMem<RES> mem, const DMesh &m, const Ray &ray, Hit &h, int k,
                                        bool closest, uint32_t *stack /* LDS, stride QA_BLOCK */, DCounters &cnt,
                                        TriPick &pick, uint32_t stackCap = 0xFFFFu, const uint32_t *tileList = nullptr, uint32_t listHdr = 0,
                                        bool primary = false)
{
  const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
  // wave-uniform choice: the exact MIN/MAX/threshold form only when some lane needs it
  const bool fastSlab = !__any(qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f);
  float meshExit;
  {
    float entry;
    if (fastSlab) boxEntryExitFast(ray, drcp, ld3(m.bmin), ld3(m.bmax), entry, meshExit);
    else boxEntryExit(ray, drcp, ld3(m.bmin), ld3(m.bmax), entry, meshExit);
    if (entry > h.z || entry > meshExit) return false;  // Box::IntersectRay, src/core/box.cpp:94-128
  }
  if (m.num_faces == 0) return false;
  const uint4 *nodes = RES ? mem.img + m.resNodes : reinterpret_cast<const uint4 *>(m.nodes);
  const uint4 *tris = RES ? mem.img + m.resTris : reinterpret_cast<const uint4 *>(m.tris);
  const uint4 *shade = RES ? mem.img + m.resShade : reinterpret_cast<const uint4 *>(m.shade);
  bool hasHit = false;
  uint32_t bestTri = 0;
  bool tie = false;
  // Global-memory scenes keep the reference tree: there every inner step is a dependent memory round
  // trip, and the SAH tree's longer chains of small nodes cost more than its fewer triangle tests save
  // (measured: tower scene 182 -> 199 ms, glossy caustics 52 -> 61 ms, project7_object 99 -> 93 ms),
  // while carrying both walks in one kernel costs those scenes 5 - 10 % in registers alone.
  if constexpr (STATS) {
    hasHit = walkBVH<false, STATS>(nodes, tris, m.rootData, ray, drcp, fastSlab, h.z, closest, stack, cnt, bestTri, tie);
  } else if constexpr (!RES) {
    // Global-memory meshes: the library's 4-wide tree (qa_widebvh.h) - a third of the dependent node reads, a fifth
    // of the triangle tests - with the answer checked against the reference's rules: the found triangle's leaf must
    // pass the reference's strict box test at the found distance (refReaches: then the reference's walk, whose
    // running distance is at least that, reaches the triangle too), and no tie may have been seen.  A miss needs no
    // check: every triangle the reference can accept is tested (boxes are unions of triangle bounds, widened by the
    // fp32 slack of its inside test).  Otherwise, and for ray origins so
    // far out that the inside test's areas can cancel, the lane walks the reference tree as the reference does.
    const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
    bool redo = true;
    const float hz0 = h.z;
    if (m.useWide && insideCancelReach(m, ray.p)) {
      const float pad = m.nearPad + (QA_SLACK_SCALE * 1e-6f) * (oMax + m.absMax);
      hasHit = walkWide(reinterpret_cast<const uint4 *>(m.wnodes), reinterpret_cast<const uint4 *>(m.wtris), m.wrootWord, ray, drcp, pad, h.z, closest, stack, stackCap, bestTri, tie);
      redo = tie;
      if (hasHit && !redo) {
        const uint32_t leaf = ldGlobal(shade + 3 * (size_t) bestTri + 2).w;   // DTriShade::pad
        redo = !refReaches<true>(nodes, leaf, ray, drcp, fastSlab, closest ? h.z : hz0, closest);   // (no tie: redo was `tie`)
      }
    }
    if (redo) {
      h.z = hz0;
      tie = false;
      hasHit = walkBVH<false, false, true>(nodes, tris, m.rootData, ray, drcp, fastSlab, h.z, closest, stack, cnt, bestTri, tie);
    }
  } else if (!m.useFast) {
    hasHit = walkBVH<false, STATS>(nodes, tris, m.rootData, ray, drcp, fastSlab, h.z, closest, stack, cnt, bestTri, tie);
  } else {
    const uint4 *fnodes = RES ? mem.img + m.resFNodes : reinterpret_cast<const uint4 *>(m.fnodes);
    const uint4 *ftris = RES ? mem.img + m.resFTris : reinterpret_cast<const uint4 *>(m.ftris);
    const float hz0 = h.z;
    uint32_t bestF = 0;
    // How far from a triangle can a point be that the reference's inside test still accepts?  The test
    // evaluates 2-D signed areas of magnitude <= (2P)^2 (P: largest coordinate involved) in fp32 and
    // scales them by 1 / area: the barycentrics are off by at most ~64 eps P^2 / area, i.e. the point
    // may lie up to ~200 eps P^2 / h outside an edge (h: the smallest altitude of any triangle of the
    // mesh, DMesh::invH = 1 / h), plus the error of the point itself.  The own tree's boxes are widened
    // by that much for this ray, so it reaches every triangle the reference can accept up to the far
    // side of the mesh bounds.
    // (every point of the ray up to the far side of the bounds lies between the origin and the bounds)
    const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
    const float pad = fastWalkPad(m.invH, m.absMax, oMax);
    bool listed = false;
    if constexpr (TL) {
      // Camera rays of a tile with a list for this node: the list holds every leaf a ray of the tile can enter, nearest first by a
      // lower bound of the entry distance, so testing its leaves' triangles - the same test on the same operands - finds what the
      // walk finds: the closest accepted distance, its triangle, and a tie where two triangles share that distance.
      // Wave-uniform: no stack, no box tests, every record read at one address by all lanes.
      listed = primary && (listHdr >> 31);
      if (listed) {
        const uint32_t n = (listHdr >> 8) & 0xFFu;
        const uint32_t *e = tileList + QA_TILE_LIST_HDR + (listHdr & 0xFFu);
        for (uint32_t j = 0; j < n; ++j) {
          const uint32_t entry = __builtin_amdgcn_readfirstlane(e[j]);   // QA_TILE_ENTRY
          const float bound = asF(entry & 0xFFFF0000u);
          if (!__any(h.z >= bound)) break;   // no lane's held distance reaches this leaf or any later one
          const uint32_t count = ((entry >> 12) & QA_BVH_COUNT_MASK) + 1;
          const uint32_t first = entry & 0xFFFu;
          for (uint32_t i = 0; i < count; ++i) {
            const uint4 *t = ftris + 3 * (size_t) (first + i);
            const uint4 t2 = t[2];
            if (hitTriangleZTie<true>(t[0], t[1], t2, ray, h.z, tie)) {
              hasHit = true;
              bestF = t2.w >> 2;
            }
          }
        }
      }
    }
    if (!listed)
      hasHit = walkBVH<true, false, false, QA_BLOCK, TL>(fnodes, ftris, m.frootData, ray, drcp, fastSlab, h.z, closest, stack, cnt, bestF, tie, pad);
    // Beyond the mesh bounds a triangle can only be "hit" by cancellation: at a distance D from the
    // triangle the inside test is off by ~64 eps D^2 / (L h) and would have to be off by D / L, i.e.
    // D >= h / (64 eps) ~ 2.6e5 h (all three areas then round to the same product: barycentrics 0, 0, 1).
    // The reference does accept such a hit when nothing nearer holds the ray.  The ray meets a triangle's
    // plane that far out only if it runs within (|o| + |mesh|) / D of parallel to it, so a miss on the
    // own tree is trusted unless the ray is that close to one of the mesh's (few) distinct face normals;
    // D is taken as 1e5 h.  With a hit in hand the question does not arise: D is far beyond the bounds.
    bool redo = tie;
    if (!hasHit && hz0 > meshExit) {
      const float theta = ((QA_SLACK_SCALE * 1.8e-5f) * m.invH) * (oMax + m.absMax) + QA_SLACK_SCALE * 2e-5f;   // + the tolerance the normal list was merged with
      const float lim = (theta * theta) * dot(ray.d, ray.d);
      bool parallel = m.numNormals == 0;   // no list (too many distinct normals): never trust a miss
      const float4 *nrm = reinterpret_cast<const float4 *>(mem.img + m.resNormals);
      for (uint32_t i = 0; i < m.numNormals; ++i) {
        const float4 n = nrm[i];
        const float dn = __builtin_fmaf(ray.d.x, n.x, __builtin_fmaf(ray.d.y, n.y, ray.d.z * n.z));   // not reference arithmetic: fused is fine
        parallel = parallel || (dn * dn <= lim);
      }
      redo = redo || parallel;
    }
    if (hasHit) {
      bestTri = bestF & 0x7FFFu;                  // element
      const uint32_t leaf = bestF >> 15;          // its leaf in the reference tree (the record's word, see DMesh::ftris)
      // closest: the distance just found; any-hit: the fixed t_max (h.z is untouched by walkBVH then... it is
      // set to the accepted distance, so take the saved one)
      // (at the found distance in the variant without lights only: the shared text costs the lit resident variants four spilled
      // registers and 1 % of their frames, profiles/cast_cost.txt)
      redo = redo || !refReaches(nodes, leaf, ray, drcp, fastSlab, closest ? h.z : hz0, TL && closest && !tie);
    }
    if (redo) {
      h.z = hz0;
      hasHit = walkBVH<false, false>(nodes, tris, m.rootData, ray, drcp, fastSlab, h.z, closest, stack, cnt, bestTri, tie);
    }
  }
  if (!closest) return hasHit;
  if (hasHit) {
    float ba = 0, bb = 0;
    {
      const uint4 *t = tris + 3 * (size_t) bestTri;
      triangleDetails(ld16<!RES>(t), ld16<!RES>(t + 1), ld16<!RES>(t + 2), ray, h, ba, bb);
    }
    // shading normal: TriMesh::GetNormal (src/mesh/TriMesh.h:196-204), left un-normalised
    const uint4 *s = shade + 3 * (size_t) bestTri;
    const uint4 s0 = ld16<!RES>(s), s1 = ld16<!RES>(s + 1), s2 = ld16<!RES>(s + 2);
    const float bc = 1.f - ba - bb;
    const f3 n0 = F3(asF(s0.x), asF(s0.y), asF(s0.z)), n1 = F3(asF(s0.w), asF(s1.x), asF(s1.y)),
             n2 = F3(asF(s1.z), asF(s1.w), asF(s2.x));
    h.N = (n0 * ba + n1 * bb) + n2 * bc;
    h.mtlID = (int) s2.y;
    h.node = k;
    pick.tri = bestTri;
    pick.a = ba;
    pick.b = bb;
  }
  return hasHit;
}

// Scene::TraceNodeNormal (src/scene/scene.cpp:50-74): closest hit over every node in pre-order.
// TEX: also maintains HitInfo::uvw / duvw / hasTexture exactly as the intersectors do (fields are
// only overwritten by the object types that set them, so stale values survive like in the reference).
template <bool RES, bool TEX, bool STATS, bool TL = false>
__device__ __forceinline__ bool traceClosest(const SceneMem<RES> mem, const DScene &sc, const Ray &world, const RayDiff &wd,
                                             Hit &h, TexHit &th, uint32_t *stack, DCounters &cnt, const uint32_t *tileList = nullptr,
                                             bool primary = false)
{
  QA_TALLY(cnt.casts_normal);
  const Ray r0 = rootRay<RES>(sc, world);
  GroupRay grp;
  grp.node = -1;
  grp.ray = r0;
  bool any = false;
  uint32_t listSlot = 0;   // TL: mesh nodes with a leaf table met so far (the order buildTileLists numbers them in)
  for (int k = 1; k < sc.num_inst; ++k) {
    const int type = instAt<RES>(sc, k).obj_type;
    if (type == QA_OBJ_NONE) continue;
    Ray r;
    RayDiff rd;
    if (TEX) localRayDiff<RES>(sc, k, world, wd, r, rd);
    else r = localRayInGroup<RES>(sc, k, r0, grp);
    bool hit;
    if (type == QA_OBJ_SPHERE) {
      hit = hitSphere(r, h, k, true);
      if (TEX && hit) texSphere(r.p, rd.dx, rd.dy, h.p, h.N, th);
    } else if (type == QA_OBJ_PLANE) {
      hit = hitPlane(r, h, k, true);
      if (TEX && hit) texPlane(r.p, rd.dx, rd.dy, h.p, th);
    } else {
      const DMesh &m = meshAt<RES>(sc, instAt<RES>(sc, k).mesh);
      TriPick pick;
      QA_T(tm0)
      uint32_t listHdr = 0;
      if constexpr (TL) {
        if (tileList && m.useFast && m.numLeaves) {
          if (listSlot < QA_TILE_LIST_HDR) listHdr = __builtin_amdgcn_readfirstlane(tileList[listSlot]);
          ++listSlot;
        }
      }
      hit = hitMesh<RES, STATS, TL>(mem, m, r, h, k, true, stack, cnt, pick, sc.stackDepth, tileList, listHdr, primary);
      QA_TACC(cnt.sl[3], tm0)
#ifdef QA_STAMPS
      if (TL && !__any(primary)) QA_TACC(cnt.sl[19], tm0)   // of which: casts of a wave without a camera ray
#endif
      if (TEX && hit && m.hasVT) {
        const uint4 *t = (RES ? mem.img + m.resTris : reinterpret_cast<const uint4 *>(m.tris)) + 3 * (size_t) pick.tri;
        const float *vt = m.vt + 6 * (size_t) pick.tri;
        texTriangle(t[0], t[1], t[2], vt, r.p, rd.dx, rd.dy, pick.a, pick.b, th);
      }
    }
    any |= hit;
  }
  if (any) {
    // Node::FromNodeCoords at every level from the hit node up to and including the root
    // (src/core/node.cpp:127-139); the reference applies them as its recursion unwinds.
    for (int a = h.node; a >= 0; a = instAt<RES>(sc, a).parent) {
      if (a == 0 && sc.rootIdentity) {
        h.N = normalize(h.N);  // identity root: p unchanged, the normal is still re-normalised
        break;
      }
      const qa_instance &in = instAt<RES>(sc, a);
      h.p = mulMV(in.tm, h.p) + ld3(in.pos);
      h.N = normalize(mulTMV(in.itm, h.N));
    }
  }
  return any;
}

// GenLight::Shadow -> Scene::TraceNodeShadow (src/lights/lights.cpp:39-48, src/scene/scene.cpp:35-46)
template <bool RES, bool STATS>
__device__ __forceinline__ float shadow(const SceneMem<RES> mem, const DScene &sc, const Ray &world, float t_max,
                                        uint32_t *stack, DCounters &cnt)
{
  QA_TALLY(cnt.casts_shadow);
  Hit h;
  h.z = t_max;
  h.node = -1;
  const Ray r0 = rootRay<RES>(sc, world);
  GroupRay grp;
  grp.node = -1;
  grp.ray = r0;
  for (int k = 1; k < sc.num_inst; ++k) {
    const int type = instAt<RES>(sc, k).obj_type;
    if (type == QA_OBJ_NONE) continue;
    const Ray r = localRayInGroup<RES>(sc, k, r0, grp);
    bool hit;
    if (type == QA_OBJ_SPHERE) hit = hitSphere(r, h, k, false);
    else if (type == QA_OBJ_PLANE) hit = hitPlane(r, h, k, false);
    else {
      TriPick pick;
      QA_T(tm0)
      hit = hitMesh<RES, STATS>(mem, meshAt<RES>(sc, instAt<RES>(sc, k).mesh), r, h, k, false, stack, cnt, pick, sc.stackDepth);
      QA_TACC(cnt.sl[6], tm0)
    }
    if (hit) return 0.0f;
  }
  return 1.0f;
}

// ---------------------------------------------------------------------------------------------
// The last cast of a path, asked as "which emitter does this ray meet" (scenes whose plan has lastCastQuery: qa_scene_build.cpp
// PlanLastCast).  There the hit of a bounce ray adds T * emission(material), draws RandomSelectMtl's one number and ends
// the path, and only planes and spheres emit ("glow nodes", DScene::lastCastGlow).  So the closest-hit sweep decides two things:
// whether anything is hit (the draw), and whether the nearest thing is a glow node (its emission; everything else adds T * 0).
//   (a) the glow nodes alone, in pre-order, from h.z = QA_BIGFLOAT: tG and G, the nearest of them (the first at equal distance);
//   (b) an any-hit sweep over the other nodes with a fixed limit per node: QA_BIGFLOAT without G; the float above tG for a node before
//       G (the earlier node keeps a tie: every intersector asks h.z > t); tG for a node after G.
// Exact, because the reference's sweep (Scene::TraceNodeNormal) holds a distance >= the node's limit when it reaches a node while
// nothing below a limit has been accepted (earlier glow nodes lie at or beyond tG, those before G beyond it):
//   * found => the reference is blocked too.  Its walk of the mesh starts from a distance >= limit and lowers it only to accepted
//     distances; while none of them is below the limit it enters every box whose strict test passes at the limit - the found
//     triangle's leaf is asked exactly that (refReaches at the fixed limit, as for shadow rays) - in its own order, which does not
//     depend on the distance held, and tests the triangle against a distance >= limit > t: accepted.  And once it holds something
//     below the limit, a non-glow node wins either way.  Planes and spheres are functions of (ray, h.z > t) alone.
//   * not found => no triangle the inside test accepts lies below the limit within the mesh bounds (the own tree reaches all of them:
//     padded boxes, non-strict tests), so the reference accepts none either; beyond the bounds hitMesh's rule for misses applies.
// A lane whose found triangle's leaf fails the strict test at the limit, which saw a triangle at exactly the limit or whose mesh has
// no own tree answers "ask again": it repeats the ray as the closest-hit sweep and shading of every other variant.
// ---------------------------------------------------------------------------------------------
// The bounce rays' any-hit query sweeps a mesh's leaf table where DScene::lastCast says so (profiles/leaf_sweep_cost.txt), a leaf per
// turn (profiles/leaf_pair_cost.txt).  The sweep needs the meshes' leaf-pair bytes in LDS, which qa_kernel_lastcast_body.h provides;
// for a mesh without the bytes the query walks the own tree: the same answers.
#if defined(QA_STAMPS)
// diagnostic builds: slots 13 / 14 = cycles of the sweep's box phase / triangle phase, 17 = turns of the triangle phase's loop,
// 18 = lanes that ran those turns (one popcount a turn); the cooperative kernel's slots otherwise
#define QA_SWEEP_TURN(cnt)                                                                          \
  {                                                                                                 \
    const unsigned long long in_ = __ballot(1);                                                     \
    if ((int) __lane_id() == __ffsll((long long) in_) - 1) { cnt.sl[17] += 1; cnt.sl[18] += (unsigned long long) __popcll(in_); } \
  }
#else
#define QA_SWEEP_TURN(cnt)
#endif

// Box phase of sweepLeaves: leaves j0 .. j1 - 1 (at most 32) of a leaf table -> bit j - j0 = this lane's ray passes the test that
// walkBVH<true> applies to a child's box when it visits the parent (the same operands, the same form), against `limit`.  `rec`: the
// table through the constant address space (no kernel writes it) at a wave-uniform index: scalar loads, the boxes arrive in SGPRs.
typedef const __attribute__((address_space(4))) uint32_t *QaLeafPtr;
__device__ __forceinline__ uint32_t sweepLeafBoxes(QaLeafPtr rec, uint32_t j0, uint32_t j1, const Ray &ray, f3 pLo, f3 pHi, f3 drcp, bool fastSlab, float limit)
{
  uint32_t mask = 0;
#pragma unroll 4   // (several records per wait)
  for (uint32_t j = j0; j < j1; ++j) {
    QaLeafPtr r = rec + 8 * (size_t) j;   // DNode
    const f3 bmin = F3(asF(r[0]), asF(r[1]), asF(r[2])), bmax = F3(asF(r[3]), asF(r[4]), asF(r[5]));
    float entry, exit_;
    if (fastSlab) boxEntryExitPadFma(pLo, pHi, drcp, bmin, bmax, entry, exit_);
    else boxEntryExitPad(pLo, pHi, ray.d, drcp, bmin, bmax, entry, exit_);
    mask |= (entry <= limit && entry <= exit_) ? (1u << (j - j0)) : 0u;
  }
  return mask;
}

// The any-hit query of walkBVH<true, ..., FMA>(closest = false) on a mesh whose own tree has a leaf table (DMesh::resLeaves; 2 ..
// QA_TILE_LEAF_CAP leaves), without the tree: every leaf's box is tested once, all lanes at the same leaf (no stack, no near / far
// choice - an any-hit query at a fixed limit gains nothing from the nearer box first), then each lane tests the triangles of its
// own candidates, in the table's order, until one is accepted (the host hands in the copy of the table that is sorted largest box
// first: an any-hit query wants the likeliest blocker first, and it is the walls that block most rays).  The walk reaches a leaf only after this test on this box has
// passed, so its leaves are among the candidates; what an extra candidate can add is a triangle the reference's own test accepts
// below the limit, and the caller asks refReaches about the found triangle as it does for the walk's.
// `table`: global memory, wave-uniform; `ftris`: DMesh::ftris in LDS.  hz: the limit, the accepted distance on return.
__device__ __forceinline__ bool sweepLeaves(const uint4 *table, uint32_t numLeaves, const uint4 *ftris, const Ray &ray, f3 drcp, bool fastSlab,
                                            float &hz, uint32_t &best, bool &tie, float pad, DCounters &cnt, const uint8_t *pairs)
{
  f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
  if (fastSlab) { pLo = slabRayTerm(pLo, drcp); pHi = slabRayTerm(pHi, drcp); }
  QaLeafPtr rec = (QaLeafPtr) table;
  const uint32_t n0 = numLeaves < 32u ? numLeaves : 32u;
  QA_T(tBox)
  uint32_t lo = sweepLeafBoxes(rec, 0, n0, ray, pLo, pHi, drcp, fastSlab, hz), hi = 0;
  if (numLeaves > 32u) hi = sweepLeafBoxes(rec, 32, numLeaves, ray, pLo, pHi, drcp, fastSlab, hz);
  QA_TACC(cnt.sl[13], tBox)
  QA_T(tTri)
  // `pairs` (LDS, wave-uniform): byte j = first | (count - 1) << 7 of leaf j (qa_scene_build.cpp LeafPairBytes; the caller sweeps only
  // meshes that have them).  One turn is one leaf: both of its triangles are tested against the same limit in straight-line code,
  // and nothing comes from vector memory.  A leaf of one triangle tests that record twice - the second result is the first's, so
  // it neither wins nor adds a tie of its own, and no address leaves the mesh.  The outcome is that of one triangle per turn with a
  // return at the first accepted one (tests/cpp/leaf_pair_check.cpp holds that form): the second triangle counts, its acceptance
  // and its tie, only where the first was not accepted.
  bool found = false;
  while ((lo | hi) && !found) {
    QA_SWEEP_TURN(cnt)
    uint32_t j;
    if (lo) { j = (uint32_t) __ffs((int) lo) - 1u; lo &= lo - 1u; }
    else { j = 31u + (uint32_t) __ffs((int) hi); hi &= hi - 1u; }
    const uint32_t byte = pairs[j];
    const uint4 *t = ftris + 3 * (size_t) (byte & 127u), *u = t + 3 * (size_t) (byte >> 7);
    const uint4 t2 = t[2], u2 = u[2];
    float h1 = hz, h2 = hz;
    bool tie1 = false, tie2 = false;
    const bool ok1 = hitTriangleZTie<true>(t[0], t[1], t2, ray, h1, tie1);
    const bool ok2 = hitTriangleZTie<true>(u[0], u[1], u2, ray, h2, tie2);
    tie = tie || tie1 || (!ok1 && tie2);
    found = ok1 || ok2;
    if (found) {
      best = (ok1 ? t2.w : u2.w) >> 2;   // element | reference leaf << 15 (DMesh::ftris)
      hz = ok1 ? h1 : h2;
    }
  }
  QA_TACC(cnt.sl[14], tTri)
  return found;
}

// One mesh: is there a triangle nearer than `limit`?  `again`: the answer is not known to be the reference's.
// leafTable: where the mesh has a leaf table, sweep it instead of walking the own tree (DScene::lastCast = 2; null: walk)
template <bool RES>
__device__ __forceinline__ bool blocksMesh(const SceneMem<RES> mem, const DMesh &m, const Ray &ray, float limit, uint32_t *stack,
                                           DCounters &cnt, bool &again, const uint4 *leafTable, const uint8_t *leafPairs)
{
  const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
  const bool fastSlab = !__any(qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f);
  // Box::IntersectRay (src/core/box.cpp:94-128).  entry > meshExit: the reference turns back whatever distance it holds.  entry > limit:
  // it may hold more than the entry and walk the mesh, and its inside test may accept a triangle in a face of the bounds a rounding
  // before them: the own tree's padded boxes still find such a triangle, and the lane then asks again
  float meshExit;
  bool gate;
  {
    float entry;
    if (fastSlab) boxEntryExitFast(ray, drcp, ld3(m.bmin), ld3(m.bmax), entry, meshExit);
    else boxEntryExit(ray, drcp, ld3(m.bmin), ld3(m.bmax), entry, meshExit);
    if (entry > meshExit) return false;
    gate = !(entry > limit);
  }
  if (m.num_faces == 0) return false;
  if (!m.useFast) {
    again = true;
    return false;
  }
  const uint4 *nodes = mem.img + m.resNodes, *fnodes = mem.img + m.resFNodes, *ftris = mem.img + m.resFTris;
  const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
  const float pad = fastWalkPad(m.invH, m.absMax, oMax);
  float hz = limit;
  uint32_t bestF = 0;
  bool tie = false;
  bool hit;
  // (a tree that is a single leaf is walked without a box test; numLeaves is 0 for a mesh without a table, and wave-uniform)
  const uint32_t numLeaves = __builtin_amdgcn_readfirstlane(m.numLeaves);
  // (a mesh whose leaves do not fit the bytes - DMesh::leafPairs - keeps the walk.  The one caller always has the bytes; the test of
  // `leafPairs` stays because qa_integrate_lastcast's assembly is another without it.  The table's second copy, behind the first, is
  // sorted largest box first)
  if (leafTable && numLeaves >= 2 && numLeaves <= QA_TILE_LEAF_CAP && m.leafPairs && leafPairs)
    hit = sweepLeaves(leafTable + __builtin_amdgcn_readfirstlane(m.resLeaves) + 2 * (size_t) numLeaves, numLeaves, ftris, ray,
                      drcp, fastSlab, hz, bestF, tie, pad, cnt, leafPairs);
  else
    hit = walkBVH<true, false, false, QA_BLOCK, true>(fnodes, ftris, m.frootData, ray, drcp, fastSlab, hz, false, stack, cnt, bestF, tie, pad);
  if (tie) {
    again = true;
    return false;
  }
  if (!hit) {
    if (limit > meshExit) {
      // (hitMesh: a miss of the own tree is trusted unless the ray runs nearly parallel to one of the mesh's face normals' planes)
      const float theta = ((QA_SLACK_SCALE * 1.8e-5f) * m.invH) * (oMax + m.absMax) + QA_SLACK_SCALE * 2e-5f;
      const float lim = (theta * theta) * dot(ray.d, ray.d);
      bool parallel = m.numNormals == 0;
      const float4 *nrm = reinterpret_cast<const float4 *>(mem.img + m.resNormals);
      for (uint32_t i = 0; i < m.numNormals; ++i) {
        const float4 n = nrm[i];
        const float dn = __builtin_fmaf(ray.d.x, n.x, __builtin_fmaf(ray.d.y, n.y, ray.d.z * n.z));
        parallel = parallel || (dn * dn <= lim);
      }
      // Not trusted: the reference's tree, as hitMesh walks it for such a miss.  Exact here, because the limit lies beyond the bounds:
      // every box of the tree ends before it, so neither the limit nor the distance >= limit that the reference holds turns a walk
      // back from a box until a triangle below the limit is accepted - the two walks are one walk up to there.
      if (parallel) {
        uint32_t bestR = 0;
        hz = limit;
        return walkBVH<false, false>(nodes, mem.img + m.resTris, m.rootData, ray, drcp, fastSlab, hz, false, stack, cnt, bestR, tie);
      }
    }
    return false;
  }
  if (!gate || !refReaches(nodes, bestF >> 15, ray, drcp, fastSlab, limit)) {
    again = true;
    return false;
  }
  return true;
}

// -> false: ask again with the closest-hit sweep.  Else `drawn`: something is hit; emitSet: the material set of the glow node that is
// the nearest thing, -1: none (blocked, or nothing hit)
template <bool RES>
__device__ __forceinline__ bool lastCastQuery(const SceneMem<RES> mem, const DScene &sc, const Ray &world, uint32_t *stack,
                                              DCounters &cnt, bool &drawn, int &emitSet, const uint8_t *leafPairs)
{
  const Ray r0 = rootRay<RES>(sc, world);
  const uint32_t glow = sc.lastCastGlow;
  // (a) the glow nodes
  Hit h;
  h.z = QA_BIGFLOAT;
  int G = -1, setG = -1;
  for (uint32_t rest = glow; rest; rest &= rest - 1) {
    const int k = __ffs((int) rest) - 1;
    if (k >= sc.num_inst) break;
    const qa_instance &in = instAt<RES>(sc, k);
    const Ray r = localRay<RES>(sc, k, r0);
    const bool hit = in.obj_type == QA_OBJ_SPHERE ? hitSphere(r, h, k, false) : hitPlane(r, h, k, false);
    if (hit) {
      G = k;
      setG = in.mtlset;
    }
  }
  const float tG = h.z;
  const float tGup = __uint_as_float(__float_as_uint(tG) + 1u);   // (tG > QA_BIAS: the next float above it)
  // (b) is anything else nearer?
  bool blocked = false, again = false;
  for (int k = 1; k < sc.num_inst; ++k) {
    if ((glow >> k) & 1u) continue;
    const int type = instAt<RES>(sc, k).obj_type;
    if (type == QA_OBJ_NONE) continue;
    const bool open = !blocked && !again;
    if (!__any(open)) break;
    if (open) {
      const float limit = G < 0 ? QA_BIGFLOAT : (k < G ? tGup : tG);
      const Ray r = localRay<RES>(sc, k, r0);
      Hit b;
      b.z = limit;
      if (type == QA_OBJ_SPHERE) blocked = hitSphere(r, b, k, false);
      else if (type == QA_OBJ_PLANE) blocked = hitPlane(r, b, k, false);
      else {
        QA_T(tm0)
        // (leafPairs: QA_TILE_LEAF_CAP bytes per mesh of the kernel's arguments, in LDS - qa_kernel_lastcast_body.h)
        const int mi = instAt<RES>(sc, k).mesh;
        blocked = blocksMesh<RES>(mem, meshAt<RES>(sc, mi), r, limit, stack, cnt, again, sc.lastCast == 2u ? sc.resident : nullptr,
                                  leafPairs ? leafPairs + QA_TILE_LEAF_CAP * (size_t) mi : nullptr);
        QA_TACC(cnt.sl[22], tm0)
      }
    }
  }
  drawn = blocked || G >= 0;
  emitSet = blocked ? -1 : setG;
  return !again;
}

// ---------------------------------------------------------------------------------------------
// Lights (src/lights/lights.h:35-171, src/lights/lights.cpp:23-144); area lights (size > 0.01)
// shoot 16 - 64 shadow rays per evaluation and run in the AREA kernel variants.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float inverseSquareFalloff(f3 v) { return qmin(1.f, 1.f / dot(v, v)); }

// SpotLight::GetAttenuation(Direction(p)) (src/lights/lights.cpp:128-143)
__device__ __forceinline__ float spotAttenuation(const qa_light &l, f3 p)
{
  const f3 d = normalize(p - ld3(l.position));
  const float cosTheta = dot(d, ld3(l.direction));
  if (cosTheta < 0) return 0;
  const float rr = qsqrt(1.f - cosTheta * cosTheta) / cosTheta;
  if (rr > l.outer) return 0;
  return rr < l.inner ? 1.f : qpowf((l.outer - rr) / (l.outer - l.inner), 2.f);
}

template <bool RES, bool STATS>
__device__ __forceinline__ f3 illuminate(const SceneMem<RES> mem, const DScene &sc, const qa_light &l, f3 p,
                                         uint32_t *stack, DCounters &cnt, uint32_t &rng)
{
  const f3 intensity = ld3(l.intensity);
  if (l.type != QA_LIGHT_DIRECT && l.size > 0.01f) {
    // area light: 16 shadow rays towards points of a ball around the light, 64 as soon as the
    // running estimate is a penumbra value (src/lights/lights.cpp:52-65,88-100; shadow_spp 16/64 :16-17)
    int spp = 16, n = 0;
    float inshadow = 0.0f;
    while (n < spp) {
      const f3 dir = (ld3(l.position) + uniformBall(rng, l.size)) - p;
      Ray r;
      r.p = p;
      r.d = normalize(dir);
      inshadow += (shadow<RES, STATS>(mem, sc, r, length(dir), stack, cnt) - inshadow) * inverseSquareFalloff(dir) / (float) (n + 1);
      n++;
      if (inshadow > 0.f && inshadow < 1.f) spp = 64;
    }
    f3 I = intensity * inshadow;
    if (l.type == QA_LIGHT_SPOT) I = I * spotAttenuation(l, p);
    return I;
  }
  if (l.type == QA_LIGHT_DIRECT) {
    Ray r;
    r.p = p;
    r.d = normalize(-ld3(l.direction));
    return intensity * shadow<RES, STATS>(mem, sc, r, QA_BIGFLOAT, stack, cnt);
  }
  // point / spot
  const f3 dir = ld3(l.position) - p;
  Ray r;
  r.p = p;
  r.d = normalize(dir);
  f3 I = (intensity * shadow<RES, STATS>(mem, sc, r, length(dir), stack, cnt)) * inverseSquareFalloff(dir);
  if (l.type == QA_LIGHT_SPOT) I = I * spotAttenuation(l, p);
  return I;
}

__device__ __forceinline__ f3 lightDirection(const qa_light &l, f3 p)
{
  if (l.type == QA_LIGHT_DIRECT) return ld3(l.direction);
  return normalize(p - ld3(l.position));
}

// Direct lighting of one shading point (MtlBlinn_PhotonMap.cpp:481-498): every non-ambient light,
// weight 1/#lights (ambient counted), Blinn lobe around the half vector.
template <bool RES, bool STATS>
__device__ __forceinline__ f3 directLight(const SceneMem<RES> mem, const DScene &sc, f3 p, f3 N, f3 V, f3 kd, f3 ks,
                                          float gloss, uint32_t *stack, DCounters &cnt, uint32_t &rng)
{
  f3 sum = F3(0, 0, 0);
  const float normCoefDI = 1.f / (float) sc.num_lights;
  for (int li = 0; li < sc.num_lights; ++li) {
    const qa_light l = ldTable(sc.light + li);
    if (l.type == QA_LIGHT_AMBIENT) continue;
    if (!STATS && !(l.type != QA_LIGHT_DIRECT && l.size > 0.01f)) {
      // Not an area light, nothing to count: the term first, as if unshadowed (a shadow factor of 1.0f multiplies exactly), the shadow
      // ray only when that term is not zero in every component - a surface facing away from the light (cosNL = max(0, N.L) = 0) adds
      // the same zero whether it is occluded or not; an occluded light's term is the unshadowed one times 0.0f (the reference's term
      // with the factor 0.0f: a zero of some sign - or a NaN exactly when the unshadowed term is not finite; a sum that started
      // from +0 does not see the sign of a zero).  qa_kernel_cs.h's csLightTerms / csLightSum, one lane at a time.
      f3 I;
      Ray r;
      r.p = p;
      float tmax = QA_BIGFLOAT;
      if (l.type == QA_LIGHT_DIRECT) {
        I = ld3(l.intensity) * 1.0f;
        r.d = normalize(-ld3(l.direction));
      } else {
        const f3 dir = ld3(l.position) - p;
        r.d = normalize(dir);
        tmax = length(dir);
        I = (ld3(l.intensity) * 1.0f) * inverseSquareFalloff(dir);
        if (l.type == QA_LIGHT_SPOT) I = I * spotAttenuation(l, p);
      }
      const f3 intensity = I * normCoefDI;
      const f3 Ld = normalize(-lightDirection(l, p));
      const f3 H = normalize(V + Ld);
      const float cosNL = qmax(0.f, dot(N, Ld));
      const float cosNH = qmax(0.f, dot(N, H));
      const f3 brdf = kd + ks * qpowf(cosNH, gloss);
      const f3 u = (intensity * cosNL) * brdf;
      const bool walk = sc.walkZeroTerms || !(u.x == 0.f && u.y == 0.f && u.z == 0.f);
      if (!walk) QA_TALLY(cnt.casts_shadow);   // (the reference casts it: counted, not walked)
      const bool occluded = walk && shadow<RES, STATS>(mem, sc, r, tmax, stack, cnt) == 0.0f;
      sum = sum + (occluded ? u * 0.0f : u);
      continue;
    }
    const f3 intensity = illuminate<RES, STATS>(mem, sc, l, p, stack, cnt, rng) * normCoefDI;
    const f3 Ld = normalize(-lightDirection(l, p));
    const f3 H = normalize(V + Ld);
    const float cosNL = qmax(0.f, dot(N, Ld));
    const float cosNH = qmax(0.f, dot(N, H));
    const f3 brdf = kd + ks * qpowf(cosNH, gloss);
    sum = sum + (intensity * cosNL) * brdf;
  }
  return sum;
}

// ---------------------------------------------------------------------------------------------
// MtlBlinn_PhotonMap::Shade up to (not including) the light loop
// (src/materials/MtlBlinn_PhotonMap.cpp:256-479): sampled colours, Fresnel, the lobe / Russian-
// roulette draw and the sampled secondary direction.  Shared by both kernels.
// ---------------------------------------------------------------------------------------------
struct Surface {
  f3 emission, kd, ks;   // sampled emission / diffuse / specular colours
  float gloss;
  bool spawn;            // a secondary ray follows
  f3 nextDir, bxdf;      // its (un-normalised) direction and the BxDF weight (PDF = 1)
  bool nextFromDiffuse;
  bool selDiffuse;       // RandomSelectMtl returned DIFFUSE (photon-map gathers hang off this)
};

// The textured kernels' form of shadeSurface: the same operations with every texture lookup of the hit FIRST (below).  A function of
// its own because reordering the shared text changes the register allocation of the untextured kernels too (the Cornell-box kernel:
// 87 -> 113 spilled registers, 13.16 -> 12.76 Gsamples/s).
template <bool TEX, class S = DScene>
__device__ __forceinline__ Surface shadeSurfaceTexFirst(const uint4 *mtlTable, const S &sc, const TexTables &tt, int mi, f3 N,
                                                f3 V, bool front, const TexHit &th, int bounceLeft, bool fromDiffuse,
                                                uint32_t &rng)
{
    const uint4 *mr = mtlTable + 6 * (size_t) mi;
    const uint4 m0 = mr[0], m1 = mr[1], m2 = mr[2], m5 = mr[5];
    f3 sampleDiffuse = F3(asF(m0.x), asF(m0.y), asF(m0.z));
    const float kill = asF(m0.w);
    f3 sampleSpecular = F3(asF(m1.x), asF(m1.y), asF(m1.z));
    const float glossSpec = asF(m1.w);
    f3 emission = F3(asF(m2.x), asF(m2.y), asF(m2.z));
    const uint32_t mflags = m5.w;
    f3 rK = F3(0, 0, 0), tK = F3(0, 0, 0);
    float glossRefl = 0.f, glossRefr = 0.f;
    if (mflags & QA_MTL_SPECULAR_LOBES) {
      const uint4 m3 = mr[3], m4 = mr[4];
      rK = F3(asF(m3.x), asF(m3.y), asF(m3.z));
      tK = F3(asF(m4.x), asF(m4.y), asF(m4.z));
      glossRefl = asF(m3.w);
      glossRefr = asF(m4.w);
    }
    if (TEX) {
      // Every texture lookup of the hit FIRST (the reference samples the colours where it uses them, MtlBlinn_PhotonMap.cpp:262-330;
      // the lookups are pure functions of the hit, so their place does not show): the 32-tap loops then run with nothing of the
      // Fresnel / lobe arithmetic alive beside them - they are where the textured kernels spill.
      const int *mt = sc.mtlTex + 8 * (size_t) mi;   // texmaps: diffuse, specular, emission, reflection, refraction
      const int4 mtex0 = make_int4(mt[0], mt[1], mt[2], mt[3]);
      const int mtex4 = mt[4];
      emission = mtlSample(tt, th, emission, mtex0.z);
      if (mflags & QA_MTL_SPECULAR_LOBES) {
        tK = mtlSample(tt, th, tK, mtex4);
        rK = mtlSample(tt, th, rK, mtex0.w);
      }
      sampleSpecular = mtlSample(tt, th, sampleSpecular, mtex0.y);
      sampleDiffuse = mtlSample(tt, th, sampleDiffuse, mtex0.x);
    }
    const f3 Y = dot(N, V) > 0.f ? N : -N;

    // ComputeFresnel (:65-105); skipped when neither lobe can receive energy: with
    // tK = rK = 0 both products below are exactly 0 for any finite Fresnel term.
    f3 sampleTransmission = F3(0, 0, 0), sampleReflection = F3(0, 0, 0);
    f3 tDir = F3(0, 0, 0), rDir = F3(0, 0, 0);
    if (mflags & QA_MTL_SPECULAR_LOBES) {
      const float ior = asF(m2.w);
      const f3 Z = cross(V, Y);
      const f3 X = normalize(cross(Y, Z));
      const float nIOR = front ? 1.f / ior : ior;
      const float cosI = dot(N, V);
      const float sinI = qsqrt(1 - cosI * cosI);
      const float sinO = qmax(0.f, qmin(1.f, sinI * nIOR));
      const float cosO = qsqrt(1.f - sinO * sinO);
      tDir = ((-X) * sinO) - (Y * cosO);
      rDir = ((N * 2.f) * dot(N, V)) - V;
      const bool totReflection = (nIOR * sinI) > 1.001f;
      const float C = (nIOR - 1.f) * (nIOR - 1.f) / ((nIOR + 1.f) * (nIOR + 1.f));
      const float rC = C + (1.f - C) * qpowf(1.f - qabs(cosI), 5.f);
      const float tC = 1.f - rC;
      sampleTransmission = totReflection ? F3(0, 0, 0) : tK * tC;
      sampleReflection = totReflection ? (rK + tK) : (rK + tK * rC);
    }

    // RandomSelectMtl (:107-150): one draw, luma-weighted lobes + Russian roulette
    const float lumaT = luma(sampleTransmission), lumaR = luma(sampleReflection), lumaD = luma(sampleDiffuse);
    const float rsel = rng1(rng);
    const float coefTransmit = lumaT;
    const float coefReflection = coefTransmit + lumaR;
    const float coefDiffuse = coefReflection + lumaD;
    const float coefSum = coefDiffuse + kill;
    const float sel = rsel * coefSum;
    int select;  // 0 transmit, 1 reflect, 2 diffuse, 3 absorb
    if (sel < coefTransmit && lumaT > 0.00001f) select = 0;
    else if (sel < coefReflection && lumaR > 0.00001f) select = 1;
    else if (sel < coefDiffuse && lumaD > 0.00001f) select = 2;
    else select = 3;

    // secondary ray (at most one): reflect / transmit / diffuse blocks (:374-479)
    bool spawn = false;
    f3 nextDir = F3(0, 0, 0), bxdf = F3(0, 0, 0);
    bool nextFromDiffuse = false;
    if (bounceLeft > 0) {
      if (select == 1) {
        if (glossRefl > 0.f) {
          do { nextDir = normalize(normalize(rDir) + uniformBall(rng, 2.f * glossRefl)); } while (dot(nextDir, Y) < 0);
        } else nextDir = rDir;
        bxdf = sampleReflection;
        spawn = true;
      } else if (select == 0) {
        if (glossRefr > 0.f) {
          do { nextDir = normalize(normalize(tDir) + uniformBall(rng, 2.f * glossRefr)); } while (dot(nextDir, Y) > 0);
        } else nextDir = tDir;
        bxdf = sampleTransmission;
        spawn = true;
      } else if (select == 2 && !fromDiffuse && front) {
        // SampleDiffuseBxDF (:199-224) + CosWeightedHemisphere (src/core/sampler.cpp:87-103)
        const float r1 = rng1(rng), r2 = rng1(rng);
        const float cosTheta = qsqrt(r1);
        const float sinTheta = qsqrt(1 - r1);
        const float phi = 2 * QA_PI * r2;
        const f3 smp = F3(sinTheta * qcosf(phi), sinTheta * qsinf(phi), cosTheta);
        nextDir = toLocalFrame(N, smp);
        bxdf = sampleDiffuse;
        if (TEX || (mflags & QA_MTL_HAS_SPECULAR)) {
          const f3 Ld = normalize(nextDir);
          const f3 H = normalize(V + Ld);
          const float cosNH = qmax(0.f, dot(N, H));
          bxdf = sampleDiffuse + sampleSpecular * qpowf(cosNH, glossSpec);
        }
        nextFromDiffuse = true;
        spawn = true;
      }
    }


  Surface o;
  o.emission = emission;
  o.kd = sampleDiffuse;
  o.ks = sampleSpecular;
  o.gloss = glossSpec;
  o.spawn = spawn;
  o.nextDir = nextDir;
  o.bxdf = bxdf;
  o.nextFromDiffuse = nextFromDiffuse;
  o.selDiffuse = (select == 2);
  return o;
}

// (S: anything with the material -> texmap table `mtlTex`: DScene, or the few words an out-of-line caller hands over)
// (LOBES = false: the caller knows that no material has QA_MTL_SPECULAR_LOBES - PlanLastCast - and the Fresnel and lobe code goes)
template <bool TEX, class S = DScene, bool LOBES = true>
__device__ __forceinline__ Surface shadeSurface(const uint4 *mtlTable, const S &sc, const TexTables &tt, int mi, f3 N,
                                                f3 V, bool front, const TexHit &th, int bounceLeft, bool fromDiffuse,
                                                uint32_t &rng)
{
    if constexpr (TEX) return shadeSurfaceTexFirst<TEX, S>(mtlTable, sc, tt, mi, N, V, front, th, bounceLeft, fromDiffuse, rng);
    const uint4 *mr = mtlTable + 6 * (size_t) mi;
    const uint4 m0 = mr[0], m1 = mr[1], m2 = mr[2], m5 = mr[5];
    f3 sampleDiffuse = F3(asF(m0.x), asF(m0.y), asF(m0.z));
    const float kill = asF(m0.w);
    f3 sampleSpecular = F3(asF(m1.x), asF(m1.y), asF(m1.z));
    const float glossSpec = asF(m1.w);
    f3 emission = F3(asF(m2.x), asF(m2.y), asF(m2.z));
    int4 mtex0 = make_int4(-1, -1, -1, -1);  // texmaps: diffuse, specular, emission, reflection
    int mtex4 = -1;                          //          refraction
    if (TEX) {
      const int *mt = sc.mtlTex + 8 * (size_t) mi;
      mtex0 = make_int4(mt[0], mt[1], mt[2], mt[3]);
      mtex4 = mt[4];
      emission = mtlSample(tt, th, emission, mtex0.z);
    }
    const uint32_t mflags = m5.w;
        const f3 Y = dot(N, V) > 0.f ? N : -N;
    
    // ComputeFresnel (:65-105); skipped when neither lobe can receive energy: with
    // tK = rK = 0 both products below are exactly 0 for any finite Fresnel term.
    f3 sampleTransmission = F3(0, 0, 0), sampleReflection = F3(0, 0, 0);
    f3 tDir = F3(0, 0, 0), rDir = F3(0, 0, 0);
    float glossRefl = 0.f, glossRefr = 0.f;
    if (LOBES && (mflags & QA_MTL_SPECULAR_LOBES)) {
      const uint4 m3 = mr[3], m4 = mr[4];
      f3 rK = F3(asF(m3.x), asF(m3.y), asF(m3.z)), tK = F3(asF(m4.x), asF(m4.y), asF(m4.z));
      if (TEX) {
        tK = mtlSample(tt, th, tK, mtex4);
        rK = mtlSample(tt, th, rK, mtex0.w);
      }
      glossRefl = asF(m3.w);
      glossRefr = asF(m4.w);
      const float ior = asF(m2.w);
      const f3 Z = cross(V, Y);
      const f3 X = normalize(cross(Y, Z));
      const float nIOR = front ? 1.f / ior : ior;
      const float cosI = dot(N, V);
      const float sinI = qsqrt(1 - cosI * cosI);
      const float sinO = qmax(0.f, qmin(1.f, sinI * nIOR));
      const float cosO = qsqrt(1.f - sinO * sinO);
      tDir = ((-X) * sinO) - (Y * cosO);
      rDir = ((N * 2.f) * dot(N, V)) - V;
      const bool totReflection = (nIOR * sinI) > 1.001f;
      const float C = (nIOR - 1.f) * (nIOR - 1.f) / ((nIOR + 1.f) * (nIOR + 1.f));
      const float rC = C + (1.f - C) * qpowf(1.f - qabs(cosI), 5.f);
      const float tC = 1.f - rC;
      sampleTransmission = totReflection ? F3(0, 0, 0) : tK * tC;
      sampleReflection = totReflection ? (rK + tK) : (rK + tK * rC);
    }

    if (TEX) {
      sampleSpecular = mtlSample(tt, th, sampleSpecular, mtex0.y);
      sampleDiffuse = mtlSample(tt, th, sampleDiffuse, mtex0.x);
    }
    // RandomSelectMtl (:107-150): one draw, luma-weighted lobes + Russian roulette
    const float lumaT = luma(sampleTransmission), lumaR = luma(sampleReflection), lumaD = luma(sampleDiffuse);
    const float rsel = rng1(rng);
    const float coefTransmit = lumaT;
    const float coefReflection = coefTransmit + lumaR;
    const float coefDiffuse = coefReflection + lumaD;
    const float coefSum = coefDiffuse + kill;
    const float sel = rsel * coefSum;
    int select;  // 0 transmit, 1 reflect, 2 diffuse, 3 absorb
    if (sel < coefTransmit && lumaT > 0.00001f) select = 0;
    else if (sel < coefReflection && lumaR > 0.00001f) select = 1;
    else if (sel < coefDiffuse && lumaD > 0.00001f) select = 2;
    else select = 3;

    // secondary ray (at most one): reflect / transmit / diffuse blocks (:374-479)
    bool spawn = false;
    f3 nextDir = F3(0, 0, 0), bxdf = F3(0, 0, 0);
    bool nextFromDiffuse = false;
    if (bounceLeft > 0) {
      if (select == 1) {
        if (glossRefl > 0.f) {
          do { nextDir = normalize(normalize(rDir) + uniformBall(rng, 2.f * glossRefl)); } while (dot(nextDir, Y) < 0);
        } else nextDir = rDir;
        bxdf = sampleReflection;
        spawn = true;
      } else if (select == 0) {
        if (glossRefr > 0.f) {
          do { nextDir = normalize(normalize(tDir) + uniformBall(rng, 2.f * glossRefr)); } while (dot(nextDir, Y) > 0);
        } else nextDir = tDir;
        bxdf = sampleTransmission;
        spawn = true;
      } else if (select == 2 && !fromDiffuse && front) {
        // SampleDiffuseBxDF (:199-224) + CosWeightedHemisphere (src/core/sampler.cpp:87-103)
        const float r1 = rng1(rng), r2 = rng1(rng);
        const float cosTheta = qsqrt(r1);
        const float sinTheta = qsqrt(1 - r1);
        const float phi = 2 * QA_PI * r2;
        const f3 smp = F3(sinTheta * qcosf(phi), sinTheta * qsinf(phi), cosTheta);
        nextDir = toLocalFrame(N, smp);
        bxdf = sampleDiffuse;
        if (TEX || (mflags & QA_MTL_HAS_SPECULAR)) {
          const f3 Ld = normalize(nextDir);
          const f3 H = normalize(V + Ld);
          const float cosNH = qmax(0.f, dot(N, H));
          bxdf = sampleDiffuse + sampleSpecular * qpowf(cosNH, glossSpec);
        }
        nextFromDiffuse = true;
        spawn = true;
      }
    }


  Surface o;
  o.emission = emission;
  o.kd = sampleDiffuse;
  o.ks = sampleSpecular;
  o.gloss = glossSpec;
  o.spawn = spawn;
  o.nextDir = nextDir;
  o.bxdf = bxdf;
  o.nextFromDiffuse = nextFromDiffuse;
  o.selDiffuse = (select == 2);
  return o;
}

// ---------------------------------------------------------------------------------------------
// Tile lists (qa_tilecull.h): for the tile whose first pixel is (X0, Y0), which leaves of every mesh node's own tree can a camera
// ray enter?  The whole wave, once per work item: lane i tests leaf i of the mesh's leaf table (global memory, behind the image),
// a ballot gives the candidates, and they go to the wave's LDS area `tl` nearest first by the lower bound of their entry
// distance: a header word (bit 31 | count << 8 | first entry) for each of the first QA_TILE_LIST_HDR such nodes, then the entries
// (QA_TILE_ENTRY).  A node whose list would be longer than `limit`, or would not fit the area, gets none: its camera rays walk
// the tree.
// ---------------------------------------------------------------------------------------------
template <bool RES>
__device__ __forceinline__ void buildTileLists(const DScene &sc, uint32_t limit, float X0, float Y0, uint32_t *tl, TileCone *cone)
{
  static_assert(QA_TILE_LEAF_CAP <= 64 && QA_TILE_LIST_CAP <= 255, "one lane per leaf, eight bits of a header word per count");
  static_assert(sizeof(TileCone) <= 64 * sizeof(uint32_t), "the pyramid waits in one row of the wave's traversal stacks");
  const unsigned lane = __lane_id();
  if (lane < QA_TILE_LIST_HDR) tl[lane] = 0u;
  TileLens lens;
  {
    f3 cW[4];
    tileWindow(ld3(sc.cam.screenA), ld3(sc.cam.screenU), ld3(sc.cam.screenV), X0, Y0, cW);
    lens = tileLens(ld3(sc.cam.pos), cW);
  }
  uint32_t cursor = 0, slot = 0;
  for (int k = 1; k < sc.num_inst && slot < QA_TILE_LIST_HDR; ++k) {
    if (instAt<RES>(sc, k).obj_type != QA_OBJ_MESH) continue;
    const DMesh &m = meshAt<RES>(sc, instAt<RES>(sc, k).mesh);
    if (!m.useFast || m.numLeaves == 0) continue;
    const uint32_t mySlot = slot++;
    {
      // origin and window through the node chain, as localRay takes a ray's origin; the pyramid goes to LDS (every lane writes
      // the same words), so that none of it occupies registers while the leaves are tested
      f3 o = ld3(sc.cam.pos), c[4];
      tileWindow(ld3(sc.cam.screenA), ld3(sc.cam.screenU), ld3(sc.cam.screenV), X0, Y0, c);
      // (outermost level first; the ancestor of a level is found by walking up from k: no array of nodes)
      const int depth = instAt<RES>(sc, k).depth;
      for (int lvl = sc.rootIdentity ? 1 : 0; lvl <= depth && lvl <= QA_MAX_NODE_DEPTH; ++lvl) {
        int a = k;
        for (int up = depth; up > lvl; --up) a = instAt<RES>(sc, a).parent;
        const qa_instance &in = instAt<RES>(sc, a);
        o = tileNodePoint(in, o);
        for (int i = 0; i < 4; ++i) c[i] = tileNodePoint(in, c[i]);
      }
      __builtin_amdgcn_wave_barrier();   // (the last node's tests have read the pyramid)
      tileCone(lens, o, c, cone);
      asm volatile("" ::: "memory");     // read it back from LDS below: do not keep it in registers
    }
    const float pad = fastWalkPad(m.invH, m.absMax, cone->oAbs);
    bool cand = false;
    float bound = 0.f;
    uint32_t word = 0;
    if (lane < m.numLeaves) {
      const uint4 *rec = sc.resident + m.resLeaves + 2 * (size_t) lane;   // DNode
      const uint4 a = ldGlobal(rec), b = ldGlobal(rec + 1);
      cand = tileConeMeetsBox(cone, F3(asF(a.x), asF(a.y), asF(a.z)), F3(asF(a.w), asF(b.x), asF(b.y)), pad, &bound);
      word = b.z;
    }
    const unsigned long long mask = __ballot(cand);
    const uint32_t count = (uint32_t) __popcll(mask);
    if (count > limit || cursor + count > QA_TILE_LIST_CAP) continue;
    uint32_t rank = 0;   // candidates that come before this lane's
    for (unsigned long long rest = mask; rest; rest &= rest - 1) {
      const int j = __ffsll((long long) rest) - 1;
      const float bj = __shfl(bound, j);
      rank += (bj < bound || (bj == bound && j < (int) lane)) ? 1u : 0u;
    }
    if (cand) tl[QA_TILE_LIST_HDR + cursor + rank] = QA_TILE_ENTRY(word, __float_as_uint(bound));
    if (lane == 0) tl[mySlot] = 0x80000000u | (count << 8) | cursor;
    cursor += count;
  }
  __builtin_amdgcn_wave_barrier();
}

// The kernel's scene tables as tileIsEmpty reads them (qa_emptytile.h)
template <bool RES>
struct EmptyTileScene {
  const DScene &sc;
  __device__ __forceinline__ decltype(auto) inst(int k) const { return instAt<RES>(sc, k); }
  __device__ __forceinline__ decltype(auto) mesh(int i) const { return meshAt<RES>(sc, i); }
};

// ---------------------------------------------------------------------------------------------
// Per-lane path state
// ---------------------------------------------------------------------------------------------
struct Path {
  Ray ray;          // next ray to trace (world space)
  f3 T;             // throughput
  f3 L;             // radiance gathered by this sample so far
  int absorbMtl;    // material the current ray was spawned from: its absorption applies on a
                    // back-face exit (Beer's law, ComputeSecondaryRay :244-248); -1 for camera rays
  int bounce;       // bounceCount the next hit is shaded with
  bool fromDiffuse; // hInfo.c.hasDiffuseHit of the next hit
  bool primary;     // camera ray
};

// ---------------------------------------------------------------------------------------------
// The kernel.  Dynamic LDS: [resident scene image (RES) | traversal stacks (stackDepth x 256) | per-lane columns | tile lists (RES, RenderParams::tile_lists)]
// ---------------------------------------------------------------------------------------------
// Area lights draw random numbers, and the reference evaluates a hit's lights only AFTER the whole
// recursive subtree below it (MtlBlinn_PhotonMap.cpp:374-479 precede :484-498).  AREA variants
// therefore log one record per hit (19 floats, SoA in a global scratch slab) and replay the lights
// deepest hit first when the path ends, continuing the same xorshift32 stream.
#define QA_MAX_PATH 8           /* hits per path an AREA variant can log (maxBounce <= 7) */
#define QA_REC_FLOATS 19

// PHOTON variants (Scene::usePhotonMap, -use-photon-map): a DIFFUSE selection gathers from the
// caustics map, and from the photon map instead of bouncing when the ray already comes from a
// diffuse bounce (MtlBlinn_PhotonMap.cpp:349-359,426-458).  The gathers draw no random numbers, so
// they are evaluated at the hit (also by AREA variants).
// Waves per SIMD the register allocator must leave room for.  The LDS-resident kernel without lights
// (the Cornell box class: VALU-issue bound, smallest register footprint) gains from a fifth wave (+5 %);
// every other variant loses more to the extra spills than the added latency hiding returns
// (resident glass-sphere room -36 %, project7_object -8 %, glossy caustics -10 %); 6 loses everywhere.
#ifndef QA_C2_EXTRA_WAVE
#define QA_C2_EXTRA_WAVE 1   /* 0: four waves per SIMD for that variant too - spill-free and 6 % slower (profiles/round02/c2_register_variants.txt) */
#endif
#define QA_WAVES_FOR(RES, LIGHTS) (((RES) && !(LIGHTS)) ? QA_MIN_WAVES + QA_C2_EXTRA_WAVE : QA_MIN_WAVES)
// qa_integrate_lastcast has a macro of its own: four against five waves per SIMD were measured again on its straight-line body
// (profiles/lastcast_straight_cost.txt); -DQA_LASTCAST_WAVES=4 for the A/B
#ifndef QA_LASTCAST_WAVES
#define QA_LASTCAST_WAVES (QA_MIN_WAVES + QA_C2_EXTRA_WAVE)
#endif

template <bool RES, bool LIGHTS, bool TEX, bool AREA, bool STATS, bool PHOTON = false>
__global__ __launch_bounds__(QA_BLOCK, QA_WAVES_FOR(RES, LIGHTS)) void qa_integrate(const DScene sc, const RenderParams rp)
{
  constexpr bool RAYS = false, POINTS = false;
  const RayBatch rb = {};
#include "qa_kernel_body.h"
}

// qa_integrate<RES, LIGHTS=0, TEX=0, AREA=0> for scenes whose plan has lastCastQuery (qa_frame.hip SelectKernel; kernel_name():
// "qa_integrate<RES=1,LIGHTS=0,TEX=0,AREA=0,LASTCAST=1>").  A kernel of its own name, so that every qa_integrate instance keeps its own.
// Its paths are camera ray, diffuse hit, one bounce ray: one turn of the loop per sample (qa_kernel_lastcast_body.h).
template <bool RES>
__global__ __launch_bounds__(QA_BLOCK, QA_LASTCAST_WAVES) void qa_integrate_lastcast(const DScene sc, const RenderParams rp)
{
#include "qa_kernel_lastcast_body.h"
}

// qa_integrate<RES, LIGHTS, TEX, AREA> whose paths start from rays of the caller's (qa_radiance_rays*; the opening comment of
// qa_radiance.hip is the specification): the second entry point over the body.  The ray arrays are a third kernel argument, so that
// RenderParams and the kernel arguments of every shipped kernel stay as they are.  Instances: qa_radiance.hip.
template <bool RES, bool LIGHTS, bool TEX, bool AREA>
__global__ __launch_bounds__(QA_BLOCK, QA_WAVES_FOR(RES, LIGHTS)) void qa_integrate_rays(const DScene sc, const RenderParams rp, const RayBatch rb)
{
  constexpr bool STATS = false, PHOTON = false;
  constexpr bool RAYS = true, POINTS = false;
#include "qa_kernel_body.h"
}

// qa_integrate_rays whose batch holds surface points and normals (rb.o, rb.d) in place of rays: a sample starts by shading its point
// as a white diffuse surface and traces from there (qa_irradiance_points*; the opening comment of qa_irradiance.hip is the
// specification): the third entry point over the body.  Instances: qa_irradiance.hip.
template <bool RES, bool LIGHTS, bool TEX, bool AREA>
__global__ __launch_bounds__(QA_BLOCK, QA_WAVES_FOR(RES, LIGHTS)) void qa_integrate_points(const DScene sc, const RenderParams rp, const RayBatch rb)
{
  constexpr bool STATS = false, PHOTON = false;
  constexpr bool RAYS = true, POINTS = true;
#include "qa_kernel_body.h"
}

// The gathering siblings of the two batch kernels (QA_RADIANCE_PHOTON_MAPS: Scene::usePhotonMap for a batch, as qa_integrate's
// PHOTON variants for a frame): kernels of their own names, so that every instance above keeps its symbol and its code.  A map
// needs a point light, so LIGHTS is true; rp.pm and rp.heap are filled as for a frame (qa_ctx.h SetPhotonParams).  Instances:
// qa_radiance_pm.hip, qa_irradiance_pm.hip (whose opening comment specifies the gather at the point itself).
template <bool RES, bool TEX, bool AREA>
__global__ __launch_bounds__(QA_BLOCK, QA_WAVES_FOR(RES, true)) void qa_integrate_rays_pm(const DScene sc, const RenderParams rp, const RayBatch rb)
{
  constexpr bool LIGHTS = true, STATS = false, PHOTON = true;
  constexpr bool RAYS = true, POINTS = false;
#include "qa_kernel_body.h"
}

template <bool RES, bool TEX, bool AREA>
__global__ __launch_bounds__(QA_BLOCK, QA_WAVES_FOR(RES, true)) void qa_integrate_points_pm(const DScene sc, const RenderParams rp, const RayBatch rb)
{
  constexpr bool LIGHTS = true, STATS = false, PHOTON = true;
  constexpr bool RAYS = true, POINTS = true;
#include "qa_kernel_body.h"
}

}  // namespace qa
