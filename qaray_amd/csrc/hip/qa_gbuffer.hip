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

#include "qa_firsthit.h"
#include "qa_ctx.h"
#include "qa_stage.h"

namespace qa {

struct GBufParams {
  int32_t x0, y0, x1, y1;   // region
  uint32_t seed;
  float *normal, *albedo, *depth;   // region-local, row-major; any may be null
  int32_t *ids;
};

template <bool RES, bool TEX>
__global__ __launch_bounds__(QA_BLOCK) void qa_gbuffer(const DScene sc, const GBufParams gp)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  const uint4 *mtlTable = materialTable<RES>(sc, s_dyn);
  const TexTables tt = texTables(sc);
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

    // the camera ray of sample 0, and its cast
    const f3 texpos = camTexpos(sc.halton, 0, px, py);
    const f3 cpt = camPoint(sc.cam, texpos.x, texpos.y);
    const f3 campos = camLensPos(sc.cam, rng);
    Ray ray;
    ray.p = campos;
    ray.d = normalize(cpt - campos);
    RayDiff diff;
    diff.dx = diff.dy = F3(0, 0, 1);
    if (TEX) {
      diff.dx = normalize(camPoint(sc.cam, texpos.x + QA_DX, texpos.y) - campos);
      diff.dy = normalize(camPoint(sc.cam, texpos.x, texpos.y + QA_DX) - campos);
    }
    Hit h;
    hitInit(h);
    TexHit th;
    texHitInit(th);
    const bool found = traceClosest<RES, TEX, false>(mem, sc, ray, diff, h, th, stack, cnt);

    f3 N = F3(0, 0, 0), kd;
    int node = -1, mword = -1;
    if (!found) {
      kd = missColor<TEX>(sc, tt, texpos);
    } else {
      N = h.N;
      node = h.node;
      bool white;
      const int mi = hitMaterial(sc.mtlset, instAt<RES>(sc, h.node).mtlset, h.mtlID, white);
      mword = materialWord(mi, white, h.front);
      kd = hitColor<TEX>(sc, tt, mtlTable, th, mi, white);
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

// One launch.  Validates as a frame of one sample and no bounce does (CheckRegion).  The <RES, TEX> instance by the frame
// launcher's predicate (SelectKernel: plan.resident, plan.textured)
static int GBuffer(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t seed, float *normal, float *albedo, float *depth, int32_t *ids, hipStream_t s)
{
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;
  if (!normal && !albedo && !depth && !ids) return Fail(QA_EINVAL, "no output plane");
  if (int rc = EnsureHalton(c, 1)) return rc;
  const GBufParams gp = {x0, y0, x1, y1, seed, normal, albedo, depth, ids};
  return LaunchSceneKernel(c, PickGBuffer(c->plan.resident, c->plan.textured), gp, TileBlocks(x0, y0, x1, y1), s);
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
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;   // (as GBuffer does) before anything is sized by the region
  if (!normal && !albedo && !depth && !ids) return Fail(QA_EINVAL, "no output plane");
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  QueryStage st(c);
  const auto dN = st.Out(normal, 3 * npix), dA = st.Out(albedo, 3 * npix), dZ = st.Out(depth, npix);
  const auto dI = st.Out(ids, 2 * npix);
  if (int rc = st.Begin()) return rc;
  if (int rc = GBuffer(c, x0, y0, x1, y1, seed, st(dN), st(dA), st(dZ), st(dI), c->stream)) return rc;
  return st.End();
}

int qa_progressive_gbuffer_device(qa_ctx *c, float *d_normal, float *d_albedo, float *d_depth, int32_t *d_ids, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const FrameArgs &a = c->prog.args;   // the frame's own region and seed; the scene as it now stands (computed afresh, no cache)
  return GBuffer(c, a.x0, a.y0, a.x1, a.y1, a.seed, d_normal, d_albedo, d_depth, d_ids, StreamOf(c, hip_stream));
}

}  // extern "C"
