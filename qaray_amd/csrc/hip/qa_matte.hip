// qa_matte.hip — the matte planes of a region (qa_matte_region*, qa_progressive_matte_device) and the straight-alpha RGBA made from
// them (qa_matte_rgba_device).  Per pixel the camera rays of ALL its samples are cast, each exactly as qa_integrate builds it
// (qa_kernel.h section B) and as qa_gbuffer.hip casts sample 0, and reduced in registers: coverage, the running means of the
// albedo, the backdrop and the hit normals.  qa_matte_dev.h is the specification and holds the per-sample step, the coverage and
// the byte encode for both sides.  The kernels only read the scene; no integrator kernel, slab, counter of qa_get_counters or
// progressive frame is touched.  No reference counterpart (the reference has no alpha or AOV output).
//
// Shape: 8x8 pixel tiles, one wave per tile, lane = pixel, the LDS layout of qa_gbuffer (a prefix of qa_integrate's).  A tile
// costs as many casts as its busiest pixel has samples, and tiles differ (an ns plane, silhouettes whose lanes walk further), so a
// wave takes its next tile from a counter with one atomic, as section A does, not by stride as qa_gbuffer's one-cast frames do.
#include <algorithm>

#include "qa_firsthit.h"
#include "qa_ctx.h"
#include "qa_matte_dev.h"
#include "qa_stage.h"

namespace qa {

struct MatteParams {
  int32_t x0, y0, x1, y1;   // region
  uint32_t spp;
  const uint32_t *ns;       // region-local sample counts, or null: spp everywhere
  const uint32_t *state;    // a progressive frame's state slab, or null: word 1 of a pixel's 8 = samples taken | bit 31 finished (then ns holds the count)
  float *coverage, *albedo, *normal, *backdrop;   // region-local, row-major; any may be null
  unsigned int *work;       // the next tile (zero before the launch)
};

template <bool RES, bool TEX>
__global__ __launch_bounds__(QA_BLOCK) void qa_matte(const DScene sc, const MatteParams mp)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  const uint4 *mtlTable = materialTable<RES>(sc, s_dyn);
  const TexTables tt = texTables(sc);
  DCounters cnt = {};   // (traceClosest tallies into it; never written out)

  const int rw = mp.x1 - mp.x0, rh = mp.y1 - mp.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8, tilesY = (unsigned) (rh + 7) / 8;
  const unsigned numTiles = tilesX * tilesY;
  const unsigned lane = __lane_id();
  // the colour of a sample feeds albedo and backdrop alone: a call for coverage and / or normals looks no material or texture up
  const bool wantColor = mp.albedo || mp.backdrop;
  const f3 campos = ld3(sc.cam.pos);   // (pinhole: a camera with dof > 0.1 is refused by the host)

  for (;;) {
    unsigned tile = 0;
    if (lane == 0) tile = atomicAdd(mp.work, 1u);
    tile = __shfl(tile, 0);
    if (tile >= numTiles) break;
    const unsigned tx = (tile % tilesX) * 8 + (lane % 8), ty = (tile / tilesX) * 8 + (lane / 8);
    const bool inside = tx < (unsigned) rw && ty < (unsigned) rh;   // else: padding slot of a ragged tile
    const int px = mp.x0 + (int) tx, py = mp.y0 + (int) ty;
    const size_t q = inside ? (size_t) ty * (size_t) rw + tx : 0;
    uint32_t n = 0;
    if (inside) {
      uint32_t have = mp.spp;
      if (mp.ns) {
        have = mp.ns[q];
        if (mp.state) {
          const uint32_t w = mp.state[8 * q + 1];
          if (!(w & 0x80000000u)) have = w;
        }
      }
      n = matteSamples(have, mp.spp);
    }

    MatteAcc acc = matteAccInit();
    uint32_t nmax = n;   // the wave runs to the largest n of its lanes
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, (uint32_t) __shfl_xor(nmax, off));
    for (uint32_t s = 0; s < nmax; ++s) {
      if (s >= n) continue;
      // the camera ray of sample s, and its cast
      const f3 texpos = camTexpos(sc.halton, (int) s, px, py);
      Ray ray;
      ray.p = campos;
      ray.d = normalize(camPoint(sc.cam, texpos.x, texpos.y) - campos);
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

      // x_s: what qa_gbuffer writes to its albedo plane for this ray
      f3 kd = F3(0, 0, 0);
      if (wantColor) {
        if (!found) {
          kd = missColor<TEX>(sc, tt, texpos);
        } else {
          bool white;
          const int mi = hitMaterial(sc.mtlset, instAt<RES>(sc, h.node).mtlset, h.mtlID, white);
          kd = hitColor<TEX>(sc, tt, mtlTable, th, mi, white);
        }
      }
      matteAccSample(acc, s, found, kd.x, kd.y, kd.z, h.N.x, h.N.y, h.N.z);
    }

    if (!inside) continue;
    if (mp.coverage) mp.coverage[q] = matteCoverage(acc.hits, n);
    if (mp.albedo) { mp.albedo[3 * q] = acc.albedo[0]; mp.albedo[3 * q + 1] = acc.albedo[1]; mp.albedo[3 * q + 2] = acc.albedo[2]; }
    if (mp.normal) { mp.normal[3 * q] = acc.normal[0]; mp.normal[3 * q + 1] = acc.normal[1]; mp.normal[3 * q + 2] = acc.normal[2]; }
    if (mp.backdrop) { mp.backdrop[3 * q] = acc.backdrop[0]; mp.backdrop[3 * q + 1] = acc.backdrop[1]; mp.backdrop[3 * q + 2] = acc.backdrop[2]; }
  }
}

// One pixel per lane: 28 or 32 bytes read (rgb 12, backdrop 12, coverage 4, ns 4), 4 written - as one dword where rgba is aligned
__global__ __launch_bounds__(256) void qa_matte_rgba(const float *rgb, const float *backdrop, const float *coverage, const uint32_t *ns, uint32_t npix,
                                                     int useSRGB, int dwords, uint8_t *rgba)
{
  const uint32_t total = gridDim.x * 256u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < npix; q += total) {
    const size_t i = 3 * (size_t) q;
    const MatteRgba o = matteRgbaEncode(rgb[i], rgb[i + 1], rgb[i + 2], backdrop[i], backdrop[i + 1], backdrop[i + 2], coverage[q], ns[q], useSRGB != 0);
    if (dwords) reinterpret_cast<uint32_t *>(rgba)[q] = o.r | (uint32_t) o.g << 8 | (uint32_t) o.b << 16 | (uint32_t) o.a << 24;
    else { rgba[4 * (size_t) q] = o.r; rgba[4 * (size_t) q + 1] = o.g; rgba[4 * (size_t) q + 2] = o.b; rgba[4 * (size_t) q + 3] = o.a; }
  }
}

}  // namespace qa

typedef void (*MatteFn)(const DScene, const MatteParams);
static MatteFn PickMatte(bool resident, bool tex)
{
  if (resident) return tex ? (MatteFn) qa_matte<true, true> : (MatteFn) qa_matte<true, false>;
  return tex ? (MatteFn) qa_matte<false, true> : (MatteFn) qa_matte<false, false>;
}

struct MattePlanes { float *coverage, *albedo, *normal, *backdrop; };

// What every entry refuses, before anything is written or sized: the region as a frame's is checked (CheckRegion), then the call's own
static int CheckMatte(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const MattePlanes &o)
{
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;
  if (spp == 0 || spp > 0x7FFFFFFFu) return Fail(QA_EINVAL, "bad spp");
  if (!o.coverage && !o.albedo && !o.normal && !o.backdrop) return Fail(QA_EINVAL, "no output plane");
  if (c->ds.cam.dof > 0.1f)
    return Fail(QA_EUNSUPPORTED, "depth of field: the lens draws sit in the middle of the pixel's random stream; the samples' camera rays cannot be rebuilt");
  return QA_OK;
}

// One launch, as GBuffer's.  The tile counter is one of the context's ring of work counters, cleared on s ahead of the launch
static int Matte(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *ns, const uint32_t *state, const MattePlanes &o, hipStream_t s)
{
  if (int rc = CheckMatte(c, x0, y0, x1, y1, spp, o)) return rc;
  if (int rc = EnsureHalton(c, (int) spp)) return rc;
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned int), s));
  const MatteParams mp = {x0, y0, x1, y1, spp, ns, state, o.coverage, o.albedo, o.normal, o.backdrop, work};
  return LaunchSceneKernel(c, PickMatte(c->plan.resident, c->plan.textured), mp, TileBlocks(x0, y0, x1, y1), s);
}

extern "C" {

int qa_matte_region_device(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *d_ns, float *d_coverage, float *d_albedo,
                           float *d_normal, float *d_backdrop, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  const MattePlanes o = {d_coverage, d_albedo, d_normal, d_backdrop};
  return Matte(c, x0, y0, x1, y1, spp, d_ns, nullptr, o, StreamOf(c, hip_stream));
}

int qa_matte_region(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *ns, float *coverage, float *albedo, float *normal,
                    float *backdrop)
{
  if (int rc = Enter(c)) return rc;
  const MattePlanes host = {coverage, albedo, normal, backdrop};
  if (int rc = CheckMatte(c, x0, y0, x1, y1, spp, host)) return rc;   // before anything is sized by the region
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  QueryStage st(c);
  const auto dS = st.In(ns, npix);
  const auto dC = st.Out(coverage, npix), dA = st.Out(albedo, 3 * npix), dN = st.Out(normal, 3 * npix), dB = st.Out(backdrop, 3 * npix);
  if (int rc = st.Begin()) return rc;
  const MattePlanes dev = {st(dC), st(dA), st(dN), st(dB)};
  if (int rc = Matte(c, x0, y0, x1, y1, spp, st(dS), nullptr, dev, c->stream)) return rc;
  return st.End();
}

int qa_progressive_matte_device(qa_ctx *c, float *d_coverage, float *d_albedo, float *d_normal, float *d_backdrop, void *hip_stream)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const qa_ctx::Progressive &f = c->prog;
  const FrameArgs &a = f.args;   // the frame's own region; the scene as it now stands (computed afresh, no cache)
  const MattePlanes o = {d_coverage, d_albedo, d_normal, d_backdrop};
  if (int rc = CheckMatte(c, a.x0, a.y0, a.x1, a.y1, (uint32_t) a.sppMax, o)) return rc;
  const hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(f.done.WaitOn(s));   // the counts are read from the slabs the last pass wrote
  return Matte(c, a.x0, a.y0, a.x1, a.y1, (uint32_t) a.sppMax, a.ns, f.dState, o, s);
}

int qa_matte_rgba_device(qa_ctx *c, const float *d_rgb, const float *d_backdrop, const float *d_coverage, const uint32_t *d_ns, uint64_t npix, int srgb,
                         uint8_t *d_rgba, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (npix == 0) return Fail(QA_EINVAL, "no pixels");
  if (npix > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");   // (32-bit pixel indices in the kernel's grid-stride loop)
  if (!d_rgb || !d_backdrop || !d_coverage || !d_ns || !d_rgba) return Fail(QA_EINVAL, "null buffer");
  const uint32_t n = (uint32_t) npix;
  const uint32_t blocks = std::max(1u, std::min((n + 255u) / 256u, (uint32_t) c->numCUs * 8u));
  const int dwords = (reinterpret_cast<uintptr_t>(d_rgba) & 3u) == 0;
  hipLaunchKernelGGL(qa::qa_matte_rgba, dim3(blocks), dim3(256), 0, StreamOf(c, hip_stream), d_rgb, d_backdrop, d_coverage, d_ns, n, srgb, dwords, d_rgba);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// the same source on the CPU (no GPU, no context).  One pixel: n samples' values x_s [n][3], the hits' normals [n][3] (read where
// hit[s] != 0) and hit flags [n] -> coverage [1], albedo [3], normal [3], backdrop [3]; any output may be null
int qa_test_matte_accumulate_host(const float *values, const float *normals, const uint8_t *hit, uint32_t n, float *coverage, float *albedo, float *normal,
                                  float *backdrop)
{
  if (n && (!values || !normals || !hit)) return QA_EINVAL;
  MatteAcc acc = matteAccInit();
  for (uint32_t s = 0; s < n; ++s)
    matteAccSample(acc, s, hit[s] != 0, values[3 * s], values[3 * s + 1], values[3 * s + 2], normals[3 * s], normals[3 * s + 1], normals[3 * s + 2]);
  if (coverage) *coverage = matteCoverage(acc.hits, n);
  for (int k = 0; k < 3; ++k) {
    if (albedo) albedo[k] = acc.albedo[k];
    if (normal) normal[k] = acc.normal[k];
    if (backdrop) backdrop[k] = acc.backdrop[k];
  }
  return QA_OK;
}

int qa_test_matte_rgba_host(const float *rgb, const float *backdrop, const float *coverage, const uint32_t *ns, uint64_t npix, int srgb, uint8_t *rgba)
{
  if (!rgb || !backdrop || !coverage || !ns || !rgba || npix == 0) return QA_EINVAL;
  for (uint64_t q = 0; q < npix; ++q) {
    const MatteRgba o = matteRgbaEncode(rgb[3 * q], rgb[3 * q + 1], rgb[3 * q + 2], backdrop[3 * q], backdrop[3 * q + 1], backdrop[3 * q + 2], coverage[q],
                                        ns[q], srgb != 0);
    rgba[4 * q] = o.r; rgba[4 * q + 1] = o.g; rgba[4 * q + 2] = o.b; rgba[4 * q + 3] = o.a;
  }
  return QA_OK;
}

}  // extern "C"
