// qa_ao.hip — ambient occlusion on the resident scene: the planes of a region (qa_ao_region*, qa_progressive_ao_device) and the
// answer at points of the caller's (qa_ao_points*).  Per pixel the camera rays of its samples are cast as qa_matte.hip builds them
// and as qa_cast_rays casts them (untextured), and from every hit K short rays go out over the facing side, each tested by the
// integrators' shadow walk exactly as qa_occluded tests a ray.  The hit stays in registers; nothing but the planes is written.
// qa_ao_dev.h is the specification and holds the direction generator for both sides.  The kernels only read the scene; no
// integrator kernel, slab, counter of qa_get_counters, kernel-time record or progressive frame is touched.  No reference
// counterpart (the reference has no occlusion output).
//
// Shape, region: qa_matte's - 8x8 pixel tiles, one wave per tile, lane = pixel, tiles taken from a counter with one atomic.  A lane
// keeps two integers.  The result is a count of open rays and does not depend on the order in which rays are cast.
// Shape, points: qa_occluded's - lane = point, a persistent grid striding over the points.
// A second region form that packed the hit lanes' (record, k) items densely over the wave through an LDS list gave the same bits,
// was no faster on the Cornell box at 1080p and 28 % slower on the tower at 4K, and was removed (profiles/ao_cost.txt).
// qa_ao_grey_device turns the float plane into its 8-bit grey picture (one pixel per lane; no state of the context).
// Only the untextured walks are compiled (<RES> alone), for the reason qa_ray_query.hip gives.
#include <algorithm>

#include "qa_firsthit.h"
#include "qa_ctx.h"
#include "qa_ao_dev.h"
#include "qa_display_dev.h"
#include "qa_stage.h"

namespace qa {

struct AoParams {
  int32_t x0, y0, x1, y1;   // region
  uint32_t first, spp, K;
  uint32_t seed;
  float tmax;               // min(radius, 1e30)
  const uint32_t *ns;       // region-local sample counts, or null: first + spp everywhere
  const uint32_t *state;    // a progressive frame's state slab, or null (as MatteParams::state)
  uint32_t *open, *rays;    // region-local, row-major; any may be null
  float *ao;
  unsigned int *work;       // the next tile (zero before the launch)
};
struct AoPointParams {
  uint64_t n;
  const float *p, *nrm;     // [n][3] each
  const int32_t *stream;    // [n], or null: the point's index
  uint32_t first, K, seed;
  float tmax;
  uint32_t *open;           // either may be null
  float *ao;
};

__device__ __forceinline__ AoVec aoVec(f3 v) { const AoVec a = {v.x, v.y, v.z}; return a; }

// the K rays of one surface point -> the open ones among them
template <bool RES>
__device__ __forceinline__ uint32_t aoOpenRays(const SceneMem<RES> mem, const DScene &sc, f3 p, AoVec n, uint32_t key, uint32_t c0, uint32_t K, float tmax,
                                               uint32_t *stack, DCounters &cnt)
{
  uint32_t open = 0;
  for (uint32_t k = 0; k < K; ++k) {
    const AoVec d = aoDirection(key, c0 + k, n);
    Ray ray;
    ray.p = p;
    ray.d = F3(d.x, d.y, d.z);
    open += shadow<RES, false>(mem, sc, ray, tmax, stack, cnt) != 0.0f;
  }
  return open;
}

template <bool RES>
__global__ __launch_bounds__(QA_BLOCK) void qa_ao_region(const DScene sc, const AoParams ap)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  DCounters cnt = {};   // (the walks tally into it; never written out)

  const int rw = ap.x1 - ap.x0, rh = ap.y1 - ap.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8, tilesY = (unsigned) (rh + 7) / 8;
  const unsigned numTiles = tilesX * tilesY;
  const unsigned lane = __lane_id();
  const f3 campos = ld3(sc.cam.pos);   // (pinhole: a camera with dof > 0.1 is refused by the host)

  for (;;) {
    unsigned tile = 0;
    if (lane == 0) tile = atomicAdd(ap.work, 1u);
    tile = __shfl(tile, 0);
    if (tile >= numTiles) break;
    const unsigned tx = (tile % tilesX) * 8 + (lane % 8), ty = (tile / tilesX) * 8 + (lane / 8);
    const bool inside = tx < (unsigned) rw && ty < (unsigned) rh;   // else: padding slot of a ragged tile
    const int px = ap.x0 + (int) tx, py = ap.y0 + (int) ty;
    const size_t q = inside ? (size_t) ty * (size_t) rw + tx : 0;
    uint32_t n = 0;
    if (inside) {
      uint32_t have = ap.first + ap.spp;
      if (ap.ns) {
        have = ap.ns[q];
        if (ap.state) {
          const uint32_t w = ap.state[8 * q + 1];
          if (!(w & 0x80000000u)) have = w;
        }
      }
      n = aoSamples(have, ap.first, ap.spp);
    }
    const uint32_t key = aoKey(ap.seed, (uint32_t) py * (uint32_t) sc.cam.width + (uint32_t) px);

    uint32_t open = 0, hits = 0;
    uint32_t nmax = n;   // the wave runs to the largest n of its lanes
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, (uint32_t) __shfl_xor(nmax, off));
    for (uint32_t j = 0; j < nmax; ++j) {
      if (j >= n) continue;
      // the camera ray of sample first + j, and its cast
      const uint32_t s = ap.first + j;
      const f3 texpos = camTexpos(sc.halton, (int) s, px, py);
      Ray ray;
      ray.p = campos;
      ray.d = normalize(camPoint(sc.cam, texpos.x, texpos.y) - campos);
      RayDiff diff;   // (read by the TEX instance only)
      diff.dx = diff.dy = ray.d;
      Hit h;
      hitInit(h);
      TexHit th;
      texHitInit(th);
      if (!traceClosest<RES, false, false>(mem, sc, ray, diff, h, th, stack, cnt)) continue;
      hits += 1u;
      open += aoOpenRays<RES>(mem, sc, h.p, aoFaceNormal(aoVec(h.N), aoVec(ray.d)), key, s * ap.K, ap.K, ap.tmax, stack, cnt);
    }

    if (!inside) continue;
    const uint32_t rays = hits * ap.K;
    if (ap.open) ap.open[q] = open;
    if (ap.rays) ap.rays[q] = rays;
    if (ap.ao) ap.ao[q] = aoValue(open, rays);
  }
}

template <bool RES>
__global__ __launch_bounds__(QA_BLOCK) void qa_ao_points(const DScene sc, const AoPointParams pp)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  DCounters cnt = {};

  const uint64_t stride = (uint64_t) gridDim.x * QA_BLOCK;
  for (uint64_t i = (uint64_t) blockIdx.x * QA_BLOCK + threadIdx.x; i < pp.n; i += stride) {   // (i >= n: padding lane of the last batch)
    const f3 p = F3(pp.p[3 * i], pp.p[3 * i + 1], pp.p[3 * i + 2]);
    const AoVec n = {pp.nrm[3 * i], pp.nrm[3 * i + 1], pp.nrm[3 * i + 2]};
    uint32_t open = pp.K;   // a void point: not walked, nothing occludes it
    if (!aoVoidPoint(aoVec(p), n)) {
      const uint32_t key = aoKey(pp.seed, pp.stream ? (uint32_t) pp.stream[i] : (uint32_t) i);
      open = aoOpenRays<RES>(mem, sc, p, n, key, pp.first, pp.K, pp.tmax, stack, cnt);
    }
    if (pp.open) pp.open[i] = open;
    if (pp.ao) pp.ao[i] = aoValue(open, pp.K);
  }
}

// One pixel per lane: the plane's 8-bit grey picture, the byte qa_display_device makes of a value without sRGB
__global__ __launch_bounds__(256) void qa_ao_grey(const float *ao, uint32_t npix, uint8_t *bytes)
{
  const uint32_t total = gridDim.x * 256u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < npix; q += total) bytes[q] = displayColorByte(ao[q], false);
}

}  // namespace qa

// the <RES> instance by the frame launcher's predicate (SelectKernel: plan.resident), as PickCast picks
typedef void (*AoRegionFn)(const DScene, const AoParams);
typedef void (*AoPointsFn)(const DScene, const AoPointParams);
static AoRegionFn PickAoRegion(bool resident) { return resident ? (AoRegionFn) qa_ao_region<true> : (AoRegionFn) qa_ao_region<false>; }
static AoPointsFn PickAoPoints(bool resident) { return resident ? (AoPointsFn) qa_ao_points<true> : (AoPointsFn) qa_ao_points<false>; }

struct AoPlanes { uint32_t *open, *rays; float *ao; };

// what both forms refuse alike: K, and a radius that leaves nothing between the bias and itself
static int CheckAoRays(uint32_t K, float radius)
{
  if (K == 0 || K > QA_AO_MAX_RAYS) return Fail(QA_EINVAL, "bad K: 1 .. 256 rays per hit");
  if (!(radius > QA_BIAS)) return Fail(QA_EINVAL, "bad radius: it must exceed the bias (0.005); +inf is unbounded");
  return QA_OK;
}

// What every region entry refuses, before anything is written or sized: the region as a frame's is checked (CheckRegion), then the call's own
static int CheckAo(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t first, uint32_t spp, uint32_t K, float radius, const AoPlanes &o)
{
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;
  if (spp == 0 || spp > 0x7FFFFFFFu || first > 0x7FFFFFFFu || (uint64_t) first + spp > 0x7FFFFFFFull) return Fail(QA_EINVAL, "bad sample range");
  if (int rc = CheckAoRays(K, radius)) return rc;
  if (((uint64_t) first + spp) * K > 0xFFFFFFFFull) return Fail(QA_EINVAL, "(first + spp) * K does not fit 32 bits");
  if (!o.open && !o.rays && !o.ao) return Fail(QA_EINVAL, "no output plane");
  if (c->ds.cam.dof > 0.1f)
    return Fail(QA_EUNSUPPORTED, "depth of field: the lens draws sit in the middle of the pixel's random stream; the samples' camera rays cannot be rebuilt");
  return QA_OK;
}

// One launch, as Matte's: the tile counter is one of the context's ring of work counters, cleared on s ahead of the launch
static int AoRegion(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t first, uint32_t spp, const uint32_t *ns, const uint32_t *state, uint32_t K,
                    float radius, uint32_t seed, const AoPlanes &o, hipStream_t s)
{
  if (int rc = CheckAo(c, x0, y0, x1, y1, first, spp, K, radius, o)) return rc;
  if (int rc = EnsureHalton(c, (int) (first + spp))) return rc;
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned int), s));
  const AoParams ap = {x0, y0, x1, y1, first, spp, K, seed, aoTmax(radius), ns, state, o.open, o.rays, o.ao, work};
  return LaunchSceneKernel(c, PickAoRegion(c->plan.resident), ap, TileBlocks(x0, y0, x1, y1), s);
}

// the points form's checks are the ray queries' (QueryChecks of qa_ray_query.hip), then the call's own.  n == 0 comes first: an
// empty batch has no arrays
#define QA_AO_MAX_POINTS 0x7FFFFFFFull
static int CheckAoPoints(qa_ctx *c, uint64_t n, bool arraysGiven, bool outputGiven, uint32_t first, uint32_t K, float radius)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (n == 0) return QA_OK;
  if (n > QA_AO_MAX_POINTS) return Fail(QA_EINVAL, "more than 2^31 - 1 points");
  if (!arraysGiven) return Fail(QA_EINVAL, "null point array");
  if (!outputGiven) return Fail(QA_EINVAL, "no output");
  if (int rc = CheckAoRays(K, radius)) return rc;
  if ((uint64_t) first + K > 0x100000000ull) return Fail(QA_EINVAL, "first + K does not fit 32 bits");
  return QA_OK;
}

static int AoPoints(qa_ctx *c, uint64_t n, const float *p, const float *nrm, const int32_t *stream, uint32_t first, uint32_t K, float radius,
                    uint32_t seed, uint32_t *open, float *ao, hipStream_t s)
{
  if (int rc = CheckAoPoints(c, n, p && nrm, open || ao, first, K, radius)) return rc;
  if (n == 0) return QA_OK;
  const AoPointParams pp = {n, p, nrm, stream, first, K, seed, aoTmax(radius), open, ao};
  return LaunchSceneKernel(c, PickAoPoints(c->plan.resident), pp, (long long) ((n + QA_BLOCK - 1) / QA_BLOCK), s);
}

extern "C" {

int qa_ao_region_device(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t first, uint32_t spp, const uint32_t *d_ns, uint32_t K, float radius,
                        uint32_t seed, uint32_t *d_open, uint32_t *d_rays, float *d_ao, void *stream)
{
  if (int rc = Enter(c)) return rc;
  const AoPlanes o = {d_open, d_rays, d_ao};
  return AoRegion(c, x0, y0, x1, y1, first, spp, d_ns, nullptr, K, radius, seed, o, StreamOf(c, stream));
}

int qa_ao_region(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t first, uint32_t spp, const uint32_t *ns, uint32_t K, float radius, uint32_t seed,
                 uint32_t *open, uint32_t *rays, float *ao)
{
  if (int rc = Enter(c)) return rc;
  const AoPlanes host = {open, rays, ao};
  if (int rc = CheckAo(c, x0, y0, x1, y1, first, spp, K, radius, host)) return rc;   // before anything is sized by the region
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  QueryStage st(c);
  const auto dS = st.In(ns, npix);
  const auto dO = st.Out(open, npix), dR = st.Out(rays, npix);
  const auto dA = st.Out(ao, npix);
  if (int rc = st.Begin()) return rc;
  const AoPlanes dev = {st(dO), st(dR), st(dA)};
  if (int rc = AoRegion(c, x0, y0, x1, y1, first, spp, st(dS), nullptr, K, radius, seed, dev, c->stream)) return rc;
  return st.End();
}

int qa_progressive_ao_device(qa_ctx *c, uint32_t K, float radius, uint32_t *d_open, uint32_t *d_rays, float *d_ao, void *stream)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const qa_ctx::Progressive &f = c->prog;
  const FrameArgs &a = f.args;   // the frame's own region and seed; the scene as it now stands (computed afresh, no cache)
  const AoPlanes o = {d_open, d_rays, d_ao};
  if (int rc = CheckAo(c, a.x0, a.y0, a.x1, a.y1, 0, (uint32_t) a.sppMax, K, radius, o)) return rc;
  const hipStream_t s = StreamOf(c, stream);
  HIP_TRY(f.done.WaitOn(s));   // the counts are read from the slabs the last pass wrote
  return AoRegion(c, a.x0, a.y0, a.x1, a.y1, 0, (uint32_t) a.sppMax, a.ns, f.dState, K, radius, a.seed, o, s);
}

int qa_ao_points_device(qa_ctx *c, uint64_t n, const float *d_points, const float *d_normals, const int32_t *d_stream_ids, uint32_t first, uint32_t K,
                        float radius, uint32_t seed, uint32_t *d_open, float *d_ao, void *stream)
{
  if (int rc = Enter(c)) return rc;
  return AoPoints(c, n, d_points, d_normals, d_stream_ids, first, K, radius, seed, d_open, d_ao, StreamOf(c, stream));
}

int qa_ao_points(qa_ctx *c, uint64_t n, const float *points, const float *normals, const int32_t *stream_ids, uint32_t first, uint32_t K, float radius,
                 uint32_t seed, uint32_t *open, float *ao)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = CheckAoPoints(c, n, points && normals, open || ao, first, K, radius)) return rc;   // before anything is sized by n
  if (n == 0) return QA_OK;
  QueryStage st(c);
  const auto dP = st.In(points, 3 * n), dN = st.In(normals, 3 * n);
  const auto dS = st.In(stream_ids, n);
  const auto dO = st.Out(open, n);
  const auto dA = st.Out(ao, n);
  if (int rc = st.Begin()) return rc;
  if (int rc = AoPoints(c, n, st(dP), st(dN), st(dS), first, K, radius, seed, st(dO), st(dA), c->stream)) return rc;
  return st.End();
}

int qa_ao_grey_device(qa_ctx *c, const float *d_ao, uint64_t npix, uint8_t *d_bytes, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (npix == 0) return Fail(QA_EINVAL, "no pixels");
  if (npix > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");   // (32-bit pixel indices in the kernel's grid-stride loop)
  if (!d_ao || !d_bytes) return Fail(QA_EINVAL, "null buffer");
  const uint32_t n = (uint32_t) npix;
  const uint32_t blocks = std::max(1u, std::min((n + 255u) / 256u, (uint32_t) c->numCUs * 8u));
  hipLaunchKernelGGL(qa::qa_ao_grey, dim3(blocks), dim3(256), 0, StreamOf(c, stream), d_ao, n, d_bytes);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// the same source on the CPU (no GPU, no context).  directions: `count` rays - stream [count], c [count], n [count][3] -> d [count][3]
int qa_test_ao_directions_host(uint32_t seed, const uint32_t *stream, const uint32_t *cs, const float *n, uint64_t count, float *d)
{
  if (count && (!stream || !cs || !n || !d)) return QA_EINVAL;
  for (uint64_t i = 0; i < count; ++i) {
    const AoVec nn = {n[3 * i], n[3 * i + 1], n[3 * i + 2]};
    const AoVec v = aoDirection(aoKey(seed, stream[i]), cs[i], nn);
    d[3 * i] = v.x; d[3 * i + 1] = v.y; d[3 * i + 2] = v.z;
  }
  return QA_OK;
}

// the inner steps: the sphere points s [count][3] of the same keys and whether the fallback was taken [count] (either may be null)
int qa_test_ao_sphere_host(uint32_t seed, const uint32_t *stream, const uint32_t *cs, uint64_t count, float *s, uint8_t *fallback)
{
  if (count && (!stream || !cs || (!s && !fallback))) return QA_EINVAL;
  for (uint64_t i = 0; i < count; ++i) {
    bool fb;
    const AoVec v = aoSphere(aoRayKey(aoKey(seed, stream[i]), cs[i]), fb);
    if (s) { s[3 * i] = v.x; s[3 * i + 1] = v.y; s[3 * i + 2] = v.z; }
    if (fallback) fallback[i] = fb;
  }
  return QA_OK;
}

// and the direction from sphere points given directly: n [count][3], s [count][3] -> d [count][3]
int qa_test_ao_direction_from_host(const float *n, const float *s, uint64_t count, float *d)
{
  if (count && (!n || !s || !d)) return QA_EINVAL;
  for (uint64_t i = 0; i < count; ++i) {
    const AoVec nn = {n[3 * i], n[3 * i + 1], n[3 * i + 2]}, ss = {s[3 * i], s[3 * i + 1], s[3 * i + 2]};
    const AoVec v = aoDirectionFrom(nn, ss);
    d[3 * i] = v.x; d[3 * i + 1] = v.y; d[3 * i + 2] = v.z;
  }
  return QA_OK;
}

int qa_test_ao_face_normal_host(const float *N, const float *d, uint64_t count, float *n)
{
  if (count && (!N || !d || !n)) return QA_EINVAL;
  for (uint64_t i = 0; i < count; ++i) {
    const AoVec NN = {N[3 * i], N[3 * i + 1], N[3 * i + 2]}, dd = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    const AoVec v = aoFaceNormal(NN, dd);
    n[3 * i] = v.x; n[3 * i + 1] = v.y; n[3 * i + 2] = v.z;
  }
  return QA_OK;
}

}  // extern "C"
