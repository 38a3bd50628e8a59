// qa_gbuffer.hip — the first-hit guide planes of a region (qa_gbuffer_region*, qa_progressive_gbuffer_device): per pixel ONE cast,
// the camera ray of sample 0 exactly as qa_integrate builds it (qa_kernel.h section B), through the integrators' own traceClosest and
// texture path.  Planes: depth (the integrators' depth plane, by construction), world-space normal, the diffuse colour the
// integrator would shade the hit with (the backdrop on a miss), node / material ids.  The kernel only reads the scene; no integrator
// kernel, slab or counter is touched.  No reference counterpart (the reference has no pick or guide buffer).
//
// Shape: 8x8 pixel tiles, one wave per tile, lane = pixel, as section A hands them out - here without the work counter: a frame of
// one cast per pixel has no long tiles to balance, so wave w of the grid takes tiles w, w + waves, ...  The grid is persistent
// (what is resident at once) because a workgroup of a resident scene first copies the scene image into LDS, as qa_integrate does.
#include <algorithm>

#include "qa_kernel.h"
#include "qa_ctx.h"

namespace qa {

struct GBufParams {
  int32_t x0, y0, x1, y1;   // region
  uint32_t seed;
  float *normal, *albedo, *depth;   // region-local, row-major; any may be null
  int32_t *ids;
};

#define QA_GBUF_BACK 0x40000000   /* bit 30 of the material word: the hit is on a back face */

template <bool RES, bool TEX>
__global__ __launch_bounds__(QA_BLOCK) void qa_gbuffer(const DScene sc, const GBufParams gp)
{
  // dynamic LDS as qa_integrate lays it out: [resident scene image (RES) | traversal stacks (stackDepth x 256)]
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  if (RES) {
    for (uint32_t i = threadIdx.x; i < sc.residentVec4; i += QA_BLOCK) s_dyn[i] = sc.resident[i];
    __syncthreads();
  }
  uint32_t *stack = reinterpret_cast<uint32_t *>(s_dyn + (RES ? sc.residentVec4 : 0)) + threadIdx.x;
  const uint4 *mtlTable = RES ? s_dyn + sc.resMaterials : reinterpret_cast<const uint4 *>(sc.mtl);
  TexTables tt;
  tt.blob = sc.blob;
  tt.texels = sc.texels;
  tt.texOff = sc.texOff;
  tt.texmap = sc.texmap;
  tt.tex = sc.tex;
  tt.filter = sc.texFilter;
  DCounters cnt = {};   // (traceClosest tallies into it; never written out)

  const int rw = gp.x1 - gp.x0, rh = gp.y1 - gp.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8, tilesY = (unsigned) (rh + 7) / 8;
  const unsigned numTiles = tilesX * tilesY;
  const unsigned lane = __lane_id(), wavesPerBlock = QA_BLOCK / 64;
  for (unsigned tile = blockIdx.x * wavesPerBlock + threadIdx.x / 64; tile < numTiles; tile += gridDim.x * wavesPerBlock) {
    const unsigned tx = (tile % tilesX) * 8 + (lane % 8), ty = (tile / tilesX) * 8 + (lane / 8);
    if (tx >= (unsigned) rw || ty >= (unsigned) rh) continue;   // padding slot of a ragged tile
    const int px = gp.x0 + (int) tx, py = gp.y0 + (int) ty;
    const size_t q = (size_t) ty * (size_t) rw + tx;
    uint32_t rng = qa_pixel_seed(gp.seed, (uint32_t) py * (uint32_t) sc.cam.width + (uint32_t) px);

    // ---- the camera ray of sample 0: qa_kernel.h section B (:1551-1577), the same operations in the same order
    const float hx = sc.halton[0], hy = sc.halton[1];
    const f3 texpos = F3(hx, hy, 0.f) + F3((float) px, (float) py, 0.f);
    const f3 A = ld3(sc.cam.screenA), U = ld3(sc.cam.screenU), V = ld3(sc.cam.screenV);
    const f3 cpt = (A + U * texpos.x) + V * texpos.y;
    f3 campos = ld3(sc.cam.pos);
    if (sc.cam.dof > 0.1f) {
      const float r1 = rng1(rng), r2 = rng1(rng);
      const float r = sc.cam.dof * qsqrt(r1);
      const float t = r2 * 2.f * QA_PI;
      campos = campos + (ld3(sc.cam.screenX) * (r * qcosf(t)) + ld3(sc.cam.screenY) * (r * qsinf(t)));
    }
    Ray ray;
    ray.p = campos;
    ray.d = normalize(cpt - campos);
    RayDiff diff;
    diff.dx = diff.dy = F3(0, 0, 1);
    if (TEX) {
      const f3 xpt = (A + U * (texpos.x + QA_DX)) + V * texpos.y;
      const f3 ypt = (A + U * texpos.x) + V * (texpos.y + QA_DX);
      diff.dx = normalize(xpt - campos);
      diff.dy = normalize(ypt - campos);
    }

    // ---- the cast: section C (:1593-1605)
    Hit h;
    h.z = QA_BIGFLOAT;
    h.node = -1;
    h.mtlID = 0;
    h.front = true;
    h.p = F3(0, 0, 0);
    h.N = F3(0, 0, 0);
    TexHit th;
    th.uvw = F3(0.5f, 0.5f, 0.5f);
    th.duvw0 = th.duvw1 = F3(0, 0, 0);
    th.hasTexture = false;
    const bool found = traceClosest<RES, TEX, false>(mem, sc, ray, diff, h, th, stack, cnt);

    f3 N = F3(0, 0, 0), kd;
    int node = -1, mword = -1;
    if (!found) {
      // the background a camera ray returns (:1613-1616)
      kd = ld3(sc.background);
      if (TEX) kd = texColorSample(tt, kd, sc.bgTexmap, F3(texpos.x / (float) sc.cam.width, texpos.y / (float) sc.cam.height, 0.f));
    } else {
      N = h.N;
      node = h.node;
      // the hit's material: section D (:1632-1641)
      const qa_instance &in = instAt<RES>(sc, h.node);
      int mi = -1;
      bool white = false;
      if (in.mtlset >= 0) {
        const qa_mtlset ms = sc.mtlset[in.mtlset];
        if (ms.multi) {
          if (h.mtlID >= 0 && h.mtlID < ms.count) mi = ms.first + h.mtlID;
          else white = true;
        } else mi = ms.first;
      }
      if (mi < 0) {
        kd = white ? F3(1, 1, 1) : F3(0, 0, 0);
        mword = white ? -2 : -1;
      } else {
        // the sampled diffuse colour: shadeSurface (:1219-1221) and, textured, shadeSurfaceTexFirst (:1111-1112, :1120)
        const uint4 m0 = mtlTable[6 * (size_t) mi];
        kd = F3(asF(m0.x), asF(m0.y), asF(m0.z));
        if (TEX) kd = mtlSample(tt, th, kd, sc.mtlTex[8 * (size_t) mi]);
        mword = mi;
      }
      if (!h.front) mword = (int) ((uint32_t) mword | (uint32_t) QA_GBUF_BACK);
    }
    if (gp.depth) gp.depth[q] = found ? h.z : QA_BIGFLOAT;
    if (gp.normal) { gp.normal[3 * q] = N.x; gp.normal[3 * q + 1] = N.y; gp.normal[3 * q + 2] = N.z; }
    if (gp.albedo) { gp.albedo[3 * q] = kd.x; gp.albedo[3 * q + 1] = kd.y; gp.albedo[3 * q + 2] = kd.z; }
    if (gp.ids) { gp.ids[2 * q] = node; gp.ids[2 * q + 1] = mword; }
  }
}

}  // namespace qa

typedef void (*GBufFn)(const DScene, const GBufParams);
static GBufFn PickGBuffer(bool resident, bool tex)
{
  if (resident) return tex ? (GBufFn) qa_gbuffer<true, true> : (GBufFn) qa_gbuffer<true, false>;
  return tex ? (GBufFn) qa_gbuffer<false, true> : (GBufFn) qa_gbuffer<false, false>;
}

// One launch.  Validates as a frame of one sample and no bounce does (CheckFrame); ordered as a frame is: behind the context's last
// frame and last edit, and the next edit waits for it (it reads the tables an edit rewrites)
static int GBuffer(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t seed, float *normal, float *albedo, float *depth, int32_t *ids, hipStream_t s)
{
  FrameArgs a;
  a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
  if (int rc = CheckFrame(c, a)) return rc;
  if (!normal && !albedo && !depth && !ids) return Fail(QA_EINVAL, "no output plane");
  if (int rc = EnsureHalton(c, 1)) return rc;
  HIP_TRY(c->lastFrame.WaitOn(s));
  HIP_TRY(c->lastEdit.WaitOn(s));
  // the <RES, TEX> instance by the frame launcher's predicate (SelectKernel: plan.resident, plan.textured), with the megakernel's
  // LDS size and stack depth: the layout above is a prefix of qa_integrate's
  const ScenePlan &p = c->plan;
  const GBufFn fn = PickGBuffer(p.resident, p.textured);
  const size_t lds = c->integ[kMega].ldsBytes;
  DScene ds = c->ds;
  ds.stackDepth = c->integ[kMega].stackDepth;
  const GBufParams gp = {x0, y0, x1, y1, seed, normal, albedo, depth, ids};
  const long long tiles = (long long) ((x1 - x0 + 7) / 8) * ((y1 - y0 + 7) / 8);
  const long long needBlocks = (tiles + QA_BLOCK / 64 - 1) / (QA_BLOCK / 64);
  int perCU = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, (const void *) fn, QA_BLOCK, lds) != hipSuccess || perCU < 1) perCU = 2;
  long long blocks = std::min<long long>(needBlocks, (long long) c->numCUs * std::min(perCU, 8));
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(fn, dim3((unsigned) blocks), dim3(QA_BLOCK), (unsigned) lds, s, ds, gp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(c->lastFrame.Record(s));
  return QA_OK;
}

extern "C" {

int qa_gbuffer_region_device(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t seed, float *d_normal, float *d_albedo, float *d_depth,
                             int32_t *d_ids, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  return GBuffer(c, x0, y0, x1, y1, seed, d_normal, d_albedo, d_depth, d_ids, StreamOf(c, hip_stream));
}

int qa_gbuffer_region(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t seed, float *normal, float *albedo, float *depth, int32_t *ids)
{
  if (int rc = Enter(c)) return rc;
  FrameArgs a;   // the region is checked against the image (as GBuffer does) before anything is sized by it
  a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
  if (int rc = CheckFrame(c, a)) return rc;
  if (!normal && !albedo && !depth && !ids) return Fail(QA_EINVAL, "no output plane");
  // staging [normal 12 | albedo 12 | depth 4 | ids 8] bytes per pixel: only grows, and is only used synchronously
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  HIP_TRY(c->stageGbuffer.Reserve(npix * 36));
  float *dN = (float *) c->stageGbuffer.p, *dA = dN + 3 * npix, *dZ = dA + 3 * npix;
  int32_t *dI = (int32_t *) (dZ + npix);
  if (int rc = GBuffer(c, x0, y0, x1, y1, seed, normal ? dN : nullptr, albedo ? dA : nullptr, depth ? dZ : nullptr, ids ? dI : nullptr, c->stream))
    return rc;
  if (normal) HIP_TRY(hipMemcpyAsync(normal, dN, npix * 12, hipMemcpyDeviceToHost, c->stream));
  if (albedo) HIP_TRY(hipMemcpyAsync(albedo, dA, npix * 12, hipMemcpyDeviceToHost, c->stream));
  if (depth) HIP_TRY(hipMemcpyAsync(depth, dZ, npix * 4, hipMemcpyDeviceToHost, c->stream));
  if (ids) HIP_TRY(hipMemcpyAsync(ids, dI, npix * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

int qa_progressive_gbuffer_device(qa_ctx *c, float *d_normal, float *d_albedo, float *d_depth, int32_t *d_ids, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const FrameArgs &a = c->prog.args;   // the frame's own region and seed; the scene as it now stands (computed afresh, no cache)
  return GBuffer(c, a.x0, a.y0, a.x1, a.y1, a.seed, d_normal, d_albedo, d_depth, d_ids, StreamOf(c, hip_stream));
}

}  // extern "C"
