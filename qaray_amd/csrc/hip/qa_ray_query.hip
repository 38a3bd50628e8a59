// qa_ray_query.hip — rays of the caller's against the resident scene (qa_cast_rays*, qa_occluded*) and the renderer's own camera
// rays handed out (qa_camera_rays_device).  The walks are the integrators': traceClosest and shadow of qa_kernel.h (the reference's
// Scene::TraceNodeNormal and TraceNodeShadow), compiled here into kernels of their own; no integrator kernel, slab, progressive
// frame, counter or kernel-time record is touched.  No reference counterpart (the reference casts only the rays of its own paths).
//
// SEMANTICS
// A ray is an origin o and a direction d, both world space, fp32.  d is used as given and is NOT normalised; t is the parameter
// along d (the hit is at o + t d), as Hit::z is for a path segment.  A query answers exactly what a path segment of the integrator
// with that ray would meet: the same intersectors, the same bias (a hit with t <= QA_BIAS is not seen), the same near-zero-direction
// rule in the box tests, the same tie rules between trees and the same node order (pre-order, a later node wins only with a
// smaller t).
//   Void rays: a ray is void if any component of o or d is not finite, or if d == (0, 0, 0).  A void ray is not walked; it answers
//   as a miss, or as not occluded.
//   Closest hit, per ray; every output is optional, at least one must be given:
//     t       1 float    1e30 (QA_BIGFLOAT) on a miss
//     ids     2 int32    node and material word in the encoding of the guide planes' ids (qa_gbuffer.hip): -1, -1 on a miss;
//                        material -1: the node has none, -2: a multi-material mesh whose face names none; bit 30 of a word >= 0:
//                        the hit is on a back face (a negative word has the bit anyway and stays as it is)
//     normal  3 floats   Hit::N as traceClosest returns it (world space, unit, geometric side); 0 on a miss
//     point   3 floats   Hit::p in world space; 0 on a miss
//   Occlusion, per ray with a tmax of its own: a uint8 that is 1 iff shadow(ray, tmax) returns 0, that is iff some surface is met
//   at QA_BIAS < t < tmax.  A tmax that is NaN or <= QA_BIAS gives 0; one above 1e30, +inf included, is taken as 1e30 (what a
//   closest-hit cast can see).
//   Camera rays: origin and direction of sample 0's camera ray of every pixel of a region, region-local and row-major, exactly as
//   qa_kernel.h section B builds them from (seed, pixel): halton[0..1], the pixel's stream and the two depth-of-field draws when
//   dof > 0.1.  Cast, they meet what the frame's first sample meets.
//
// Shape: lane = ray, a wave takes 64 consecutive rays, wave w of the grid takes batches w, w + waves, ...  The grid is persistent
// (what is resident at once) because a workgroup of a resident scene first copies the scene image into LDS, as qa_integrate does.
// Padding lanes of the last batch and void rays skip the walk.  Only the untextured instance of traceClosest is compiled: no
// texture output is asked for, and the local ray of localRayDiff (TEX) and of localRayInGroup (!TEX) is the same chain of toNode
// calls on the same operands, so the hits of a textured scene come out the same (tests/test_gpu_ray_query.py holds both to the
// guide planes and the CPU restatement bit for bit on textured scenes).
#include <algorithm>

#include "qa_firsthit.h"
#include "qa_ctx.h"
#include "qa_stage.h"

namespace qa {

struct CastParams {
  uint64_t n;
  const float *o, *d;       // [n][3] each
  float *t;                 // outputs; any may be null
  int32_t *ids;
  float *normal, *point;
};
struct OccludedParams {
  uint64_t n;
  const float *o, *d, *tmax;
  uint8_t *out;
};
struct CamRayParams {
  int32_t x0, y0, x1, y1;
  uint32_t seed;
  float *o, *d;             // [(y1 - y0) * (x1 - x0)][3] each
};

__device__ __forceinline__ bool loadRay(const float *o, const float *d, uint64_t i, Ray &ray)
{
  ray.p = F3(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
  ray.d = F3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
  const bool finite = isfinite(ray.p.x) && isfinite(ray.p.y) && isfinite(ray.p.z) && isfinite(ray.d.x) && isfinite(ray.d.y) && isfinite(ray.d.z);
  return finite && !(ray.d.x == 0.f && ray.d.y == 0.f && ray.d.z == 0.f);   // false: a void ray
}

template <bool RES>
__global__ __launch_bounds__(QA_BLOCK) void qa_cast_rays(const DScene sc, const CastParams cp)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  DCounters cnt = {};   // (traceClosest tallies into it; never written out)

  const uint64_t stride = (uint64_t) gridDim.x * QA_BLOCK;
  for (uint64_t i = (uint64_t) blockIdx.x * QA_BLOCK + threadIdx.x; i < cp.n; i += stride) {   // (i >= n: padding lane of the last batch)
    Ray ray;
    const bool walk = loadRay(cp.o, cp.d, i, ray);
    Hit h;
    hitInit(h);
    bool found = false;
    if (walk) {
      RayDiff diff;   // (read by the TEX instance only)
      diff.dx = diff.dy = ray.d;
      TexHit th;
      texHitInit(th);
      found = traceClosest<RES, false, false>(mem, sc, ray, diff, h, th, stack, cnt);
    }
    int node = -1, mword = -1;
    f3 N = F3(0, 0, 0), P = F3(0, 0, 0);
    if (found) {
      N = h.N;
      P = h.p;
      node = h.node;
      bool white;
      const int mi = hitMaterial(sc.mtlset, instAt<RES>(sc, h.node).mtlset, h.mtlID, white);
      mword = materialWord(mi, white, h.front);
    }
    if (cp.t) cp.t[i] = found ? h.z : QA_BIGFLOAT;
    if (cp.ids) { cp.ids[2 * i] = node; cp.ids[2 * i + 1] = mword; }
    if (cp.normal) { cp.normal[3 * i] = N.x; cp.normal[3 * i + 1] = N.y; cp.normal[3 * i + 2] = N.z; }
    if (cp.point) { cp.point[3 * i] = P.x; cp.point[3 * i + 1] = P.y; cp.point[3 * i + 2] = P.z; }
  }
}

template <bool RES>
__global__ __launch_bounds__(QA_BLOCK) void qa_occluded(const DScene sc, const OccludedParams op)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  DCounters cnt = {};

  const uint64_t stride = (uint64_t) gridDim.x * QA_BLOCK;
  for (uint64_t i = (uint64_t) blockIdx.x * QA_BLOCK + threadIdx.x; i < op.n; i += stride) {
    Ray ray;
    bool walk = loadRay(op.o, op.d, i, ray);
    float tmax = op.tmax[i];
    if (!(tmax > QA_BIAS)) walk = false;   // NaN as well: nothing lies between the bias and such a tmax
    tmax = qmin(tmax, QA_BIGFLOAT);
    uint8_t occ = 0;
    if (walk) occ = shadow<RES, false>(mem, sc, ray, tmax, stack, cnt) == 0.0f;
    op.out[i] = occ;
  }
}

// One thread per pixel; reads the camera record and halton[0..1] only
__global__ __launch_bounds__(QA_BLOCK) void qa_camera_rays(const DCamera cam, const float *halton, const CamRayParams cr)
{
  const uint64_t rw = (uint64_t) (cr.x1 - cr.x0), npix = rw * (uint64_t) (cr.y1 - cr.y0);
  const uint64_t q = (uint64_t) blockIdx.x * QA_BLOCK + threadIdx.x;
  if (q >= npix) return;
  const int px = cr.x0 + (int) (q % rw), py = cr.y0 + (int) (q / rw);
  uint32_t rng = qa_pixel_seed(cr.seed, (uint32_t) py * (uint32_t) cam.width + (uint32_t) px);

  const f3 texpos = camTexpos(halton, 0, px, py);
  const f3 cpt = camPoint(cam, texpos.x, texpos.y);
  const f3 campos = camLensPos(cam, rng);
  const f3 dir = normalize(cpt - campos);
  cr.o[3 * q] = campos.x; cr.o[3 * q + 1] = campos.y; cr.o[3 * q + 2] = campos.z;
  cr.d[3 * q] = dir.x; cr.d[3 * q + 1] = dir.y; cr.d[3 * q + 2] = dir.z;
}

}  // namespace qa

// What both queries refuse alike, before anything is sized by n.  n == 0 comes first: an empty batch has no arrays
#define QA_MAX_RAYS 0x7FFFFFFFull
static int QueryChecks(qa_ctx *c, uint64_t n, bool arraysGiven, bool outputGiven)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 rays");
  if (!arraysGiven) return Fail(QA_EINVAL, "null ray array");
  if (!outputGiven) return Fail(QA_EINVAL, "no output");
  return QA_OK;
}
static long long RayBlocks(uint64_t n) { return (long long) ((n + QA_BLOCK - 1) / QA_BLOCK); }   // lane = ray

// the <RES> instance by the frame launcher's predicate (SelectKernel: plan.resident), as PickGBuffer picks
typedef void (*CastFn)(const DScene, const CastParams);
typedef void (*OccludedFn)(const DScene, const OccludedParams);
static CastFn PickCast(bool resident) { return resident ? (CastFn) qa_cast_rays<true> : (CastFn) qa_cast_rays<false>; }
static OccludedFn PickOccluded(bool resident) { return resident ? (OccludedFn) qa_occluded<true> : (OccludedFn) qa_occluded<false>; }

static int CastRays(qa_ctx *c, uint64_t n, const float *o, const float *d, float *t, int32_t *ids, float *normal, float *point, hipStream_t s)
{
  if (int rc = QueryChecks(c, n, o && d, t || ids || normal || point)) return rc;
  if (n == 0) return QA_OK;
  const CastParams cp = {n, o, d, t, ids, normal, point};
  return LaunchSceneKernel(c, PickCast(c->plan.resident), cp, RayBlocks(n), s);
}

static int Occluded(qa_ctx *c, uint64_t n, const float *o, const float *d, const float *tmax, uint8_t *out, hipStream_t s)
{
  if (int rc = QueryChecks(c, n, o && d && tmax, out != nullptr)) return rc;
  if (n == 0) return QA_OK;
  const OccludedParams op = {n, o, d, tmax, out};
  return LaunchSceneKernel(c, PickOccluded(c->plan.resident), op, RayBlocks(n), s);
}

extern "C" {

int qa_cast_rays_device(qa_ctx *c, uint64_t n, const float *d_origins, const float *d_dirs, float *d_t, int32_t *d_ids, float *d_normal,
                        float *d_point, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  return CastRays(c, n, d_origins, d_dirs, d_t, d_ids, d_normal, d_point, StreamOf(c, hip_stream));
}

int qa_cast_rays(qa_ctx *c, uint64_t n, const float *origins, const float *dirs, float *t, int32_t *ids, float *normal, float *point)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = QueryChecks(c, n, origins && dirs, t || ids || normal || point)) return rc;   // before anything is sized by n
  if (n == 0) return QA_OK;
  QueryStage st(c);
  const auto dO = st.In(origins, 3 * n), dD = st.In(dirs, 3 * n);
  const auto dT = st.Out(t, n), dN = st.Out(normal, 3 * n), dP = st.Out(point, 3 * n);
  const auto dI = st.Out(ids, 2 * n);
  if (int rc = st.Begin()) return rc;
  if (int rc = CastRays(c, n, st(dO), st(dD), st(dT), st(dI), st(dN), st(dP), c->stream)) return rc;
  return st.End();
}

int qa_occluded_device(qa_ctx *c, uint64_t n, const float *d_origins, const float *d_dirs, const float *d_tmax, uint8_t *d_out, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  return Occluded(c, n, d_origins, d_dirs, d_tmax, d_out, StreamOf(c, hip_stream));
}

int qa_occluded(qa_ctx *c, uint64_t n, const float *origins, const float *dirs, const float *tmax, uint8_t *out)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = QueryChecks(c, n, origins && dirs && tmax, out != nullptr)) return rc;
  if (n == 0) return QA_OK;
  QueryStage st(c);
  const auto dO = st.In(origins, 3 * n), dD = st.In(dirs, 3 * n), dT = st.In(tmax, n);
  const auto dOut = st.Out(out, n);
  if (int rc = st.Begin()) return rc;
  if (int rc = Occluded(c, n, st(dO), st(dD), st(dT), st(dOut), c->stream)) return rc;
  return st.End();
}

int qa_camera_rays_device(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t seed, float *d_origins, float *d_dirs, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;
  if (!d_origins || !d_dirs) return Fail(QA_EINVAL, "null ray array");
  if (int rc = EnsureHalton(c, 1)) return rc;
  const hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(c->lastFrame.WaitOn(s));
  HIP_TRY(c->lastEdit.WaitOn(s));
  const CamRayParams cr = {x0, y0, x1, y1, seed, d_origins, d_dirs};
  const uint64_t npix = (uint64_t) (x1 - x0) * (uint64_t) (y1 - y0);
  hipLaunchKernelGGL(qa_camera_rays, dim3((unsigned) ((npix + QA_BLOCK - 1) / QA_BLOCK)), dim3(QA_BLOCK), 0, s, c->ds.cam, c->ds.halton, cr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(c->lastFrame.Record(s));
  return QA_OK;
}

}  // extern "C"
