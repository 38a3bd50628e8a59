// qa_idmatte.hip — the id matte of a region (qa_idmatte_region*, qa_progressive_idmatte_device) and the coverage plane of a set of
// ids made from it (qa_idmatte_select_device).  Per pixel the camera rays of ALL its samples are cast, exactly as qa_matte.hip
// casts them, and the key of each hit - its node or its material - is counted into a table of eight slots that the lane keeps in
// registers; the table is ranked by a fixed network of exchanges and written once.  qa_idmatte_dev.h is the specification and holds
// the table's step, the ranking and the select product for both sides.  The kernels only read the scene; no integrator kernel,
// slab, counter of qa_get_counters or progressive frame is touched.  No reference counterpart (the reference has no id output).
//
// Shape: qa_matte's - 8x8 pixel tiles, one wave per tile, lane = pixel, tiles taken from a counter with one atomic.  The table is
// 17 registers of a lane (8 ids, 8 counts, other) and is only ever indexed by constants: nothing of it lives in LDS or scratch.
#include <algorithm>

#include "qa_firsthit.h"
#include "qa_ctx.h"
#include "qa_idmatte_dev.h"
#include "qa_matte_dev.h"
#include "qa_stage.h"

namespace qa {

struct IdMatteParams {
  int32_t x0, y0, x1, y1;   // region
  uint32_t spp;
  int32_t key;              // QA_IDMATTE_NODE / QA_IDMATTE_MATERIAL
  const uint32_t *ns;       // region-local sample counts, or null: spp everywhere
  const uint32_t *state;    // a progressive frame's state slab, or null (as MatteParams::state)
  int32_t *ids;             // region-local, row-major; any may be null
  uint32_t *counts, *other, *samples;
  unsigned int *work;       // the next tile (zero before the launch)
};

template <bool RES, bool TEX>
__global__ __launch_bounds__(QA_BLOCK) void qa_idmatte(const DScene sc, const IdMatteParams mp)
{
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  uint32_t *stack = sceneToLds<RES>(sc, s_dyn);
  DCounters cnt = {};   // (traceClosest tallies into it; never written out)

  const int rw = mp.x1 - mp.x0, rh = mp.y1 - mp.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8, tilesY = (unsigned) (rh + 7) / 8;
  const unsigned numTiles = tilesX * tilesY;
  const unsigned lane = __lane_id();
  const bool byMaterial = mp.key == QA_IDMATTE_MATERIAL;
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

    IdMatteAcc acc = idMatteInit();
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

      // the key: what qa_gbuffer writes to its ids plane for this ray
      int32_t key = h.node;
      if (found && byMaterial) {
        bool white;
        const int mi = hitMaterial(sc.mtlset, instAt<RES>(sc, h.node).mtlset, h.mtlID, white);
        key = idMatteMaterialKey(materialWord(mi, white, h.front));
      }
      idMatteSample(acc, found, key);
    }

    if (!inside) continue;
    idMatteRank(acc);
    if (mp.ids) {
      int4 *o = reinterpret_cast<int4 *>(mp.ids + 8 * q);
      o[0] = make_int4(acc.id[0], acc.id[1], acc.id[2], acc.id[3]);
      o[1] = make_int4(acc.id[4], acc.id[5], acc.id[6], acc.id[7]);
    }
    if (mp.counts) {
      uint4 *o = reinterpret_cast<uint4 *>(mp.counts + 8 * q);
      o[0] = make_uint4(acc.count[0], acc.count[1], acc.count[2], acc.count[3]);
      o[1] = make_uint4(acc.count[4], acc.count[5], acc.count[6], acc.count[7]);
    }
    if (mp.other) mp.other[q] = acc.other;
    if (mp.samples) mp.samples[q] = n;
  }
}

// The list travels in the kernel's arguments, as every small argument of the read-only passes does: the lanes of a wave read entry
// j together (a scalar load), there is no buffer of the context's whose reuse a call on another stream would have to wait for
struct IdSelectParams {
  const int32_t *ids;
  const uint32_t *counts, *samples;
  float *out;       // either may be null
  uint8_t *bytes;
  uint32_t npix, m;
  int32_t select[QA_IDMATTE_MAX_SELECT];
};

// One pixel per lane: 68 bytes read (ids 32 as two 16-byte loads, counts 32 likewise, samples 4), 4 and / or 1 written
__global__ __launch_bounds__(256) void qa_idmatte_select(const IdSelectParams sp)
{
  const uint32_t total = gridDim.x * 256u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < sp.npix; q += total) {
    const int4 *pi = reinterpret_cast<const int4 *>(sp.ids + 8 * (size_t) q);
    const uint4 *pc = reinterpret_cast<const uint4 *>(sp.counts + 8 * (size_t) q);
    const int4 i0 = pi[0], i1 = pi[1];
    const uint4 c0 = pc[0], c1 = pc[1];
    const int32_t id[QA_IDMATTE_SLOTS] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
    const uint32_t count[QA_IDMATTE_SLOTS] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float v = idMatteSelect(id, count, sp.samples[q], sp.select, sp.m);
    if (sp.out) sp.out[q] = v;
    if (sp.bytes) sp.bytes[q] = displayColorByte(v, false);
  }
}

}  // namespace qa

typedef void (*IdMatteFn)(const DScene, const IdMatteParams);
static IdMatteFn PickIdMatte(bool resident, bool tex)
{
  if (resident) return tex ? (IdMatteFn) qa_idmatte<true, true> : (IdMatteFn) qa_idmatte<true, false>;
  return tex ? (IdMatteFn) qa_idmatte<false, true> : (IdMatteFn) qa_idmatte<false, false>;
}

struct IdMattePlanes { int32_t *ids; uint32_t *counts, *other, *samples; };

static bool Aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What every entry refuses, before anything is written or sized: CheckMatte's list, then the key and the alignment of the two planes
// that are written 16 bytes at a time
static int CheckIdMatte(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, int key, const IdMattePlanes &o, bool device)
{
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;
  if (spp == 0 || spp > 0x7FFFFFFFu) return Fail(QA_EINVAL, "bad spp");
  if (key != QA_IDMATTE_NODE && key != QA_IDMATTE_MATERIAL) return Fail(QA_EINVAL, "bad key: QA_IDMATTE_NODE or QA_IDMATTE_MATERIAL");
  if (!o.ids && !o.counts && !o.other && !o.samples) return Fail(QA_EINVAL, "no output plane");
  if (device && (!Aligned16(o.ids) || !Aligned16(o.counts))) return Fail(QA_EINVAL, "ids and counts must be 16-byte aligned");
  if (c->ds.cam.dof > 0.1f)
    return Fail(QA_EUNSUPPORTED, "depth of field: the lens draws sit in the middle of the pixel's random stream; the samples' camera rays cannot be rebuilt");
  return QA_OK;
}

// One launch, as Matte's: the tile counter is one of the context's ring of work counters, cleared on s ahead of the launch
static int IdMatte(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *ns, const uint32_t *state, int key, const IdMattePlanes &o,
                   hipStream_t s)
{
  if (int rc = CheckIdMatte(c, x0, y0, x1, y1, spp, key, o, true)) return rc;
  if (int rc = EnsureHalton(c, (int) spp)) return rc;
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned int), s));
  const IdMatteParams mp = {x0, y0, x1, y1, spp, key, ns, state, o.ids, o.counts, o.other, o.samples, work};
  return LaunchSceneKernel(c, PickIdMatte(c->plan.resident, c->plan.textured), mp, TileBlocks(x0, y0, x1, y1), s);
}

extern "C" {

int qa_idmatte_region_device(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *d_ns, int key, int32_t *d_ids, uint32_t *d_counts,
                             uint32_t *d_other, uint32_t *d_samples, void *stream)
{
  if (int rc = Enter(c)) return rc;
  const IdMattePlanes o = {d_ids, d_counts, d_other, d_samples};
  return IdMatte(c, x0, y0, x1, y1, spp, d_ns, nullptr, key, o, StreamOf(c, stream));
}

int qa_idmatte_region(qa_ctx *c, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *ns, int key, int32_t *ids, uint32_t *counts, uint32_t *other,
                      uint32_t *samples)
{
  if (int rc = Enter(c)) return rc;
  const IdMattePlanes host = {ids, counts, other, samples};
  if (int rc = CheckIdMatte(c, x0, y0, x1, y1, spp, key, host, false)) return rc;   // before anything is sized by the region
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  QueryStage st(c);   // (every plane starts on a multiple of 16 bytes: what IdMatte asks of ids and counts)
  const auto dS = st.In(ns, npix);
  const auto dI = st.Out(ids, 8 * npix);
  const auto dC = st.Out(counts, 8 * npix), dO = st.Out(other, npix), dN = st.Out(samples, npix);
  if (int rc = st.Begin()) return rc;
  const IdMattePlanes dev = {st(dI), st(dC), st(dO), st(dN)};
  if (int rc = IdMatte(c, x0, y0, x1, y1, spp, st(dS), nullptr, key, dev, c->stream)) return rc;
  return st.End();
}

int qa_progressive_idmatte_device(qa_ctx *c, int key, int32_t *d_ids, uint32_t *d_counts, uint32_t *d_other, uint32_t *d_samples, void *stream)
{
  if (int rc = ProgActive(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const qa_ctx::Progressive &f = c->prog;
  const FrameArgs &a = f.args;   // the frame's own region; the scene as it now stands (computed afresh, no cache)
  const IdMattePlanes o = {d_ids, d_counts, d_other, d_samples};
  if (int rc = CheckIdMatte(c, a.x0, a.y0, a.x1, a.y1, (uint32_t) a.sppMax, key, o, true)) return rc;
  const hipStream_t s = StreamOf(c, stream);
  HIP_TRY(f.done.WaitOn(s));   // the counts are read from the slabs the last pass wrote
  return IdMatte(c, a.x0, a.y0, a.x1, a.y1, (uint32_t) a.sppMax, a.ns, f.dState, key, o, s);
}

int qa_idmatte_select_device(qa_ctx *c, const int32_t *d_ids, const uint32_t *d_counts, const uint32_t *d_samples, uint64_t npix, const int32_t *select,
                             uint32_t m, float *d_out, uint8_t *d_bytes, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (npix == 0) return Fail(QA_EINVAL, "no pixels");
  if (npix > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");   // (32-bit pixel indices in the kernel's grid-stride loop)
  if (!d_ids || !d_counts || !d_samples || (!d_out && !d_bytes)) return Fail(QA_EINVAL, "null buffer");
  if (!Aligned16(d_ids) || !Aligned16(d_counts)) return Fail(QA_EINVAL, "ids and counts must be 16-byte aligned");
  if (m > QA_IDMATTE_MAX_SELECT) return Fail(QA_EINVAL, "more ids than QA_IDMATTE_MAX_SELECT");
  if (m && !select) return Fail(QA_EINVAL, "null id list");
  IdSelectParams sp;
  sp.ids = d_ids; sp.counts = d_counts; sp.samples = d_samples; sp.out = d_out; sp.bytes = d_bytes;
  sp.npix = (uint32_t) npix; sp.m = m;
  for (uint32_t j = 0; j < QA_IDMATTE_MAX_SELECT; ++j) sp.select[j] = j < m ? select[j] : QA_IDMATTE_EMPTY;
  const uint32_t blocks = std::max(1u, std::min((sp.npix + 255u) / 256u, (uint32_t) c->numCUs * 8u));
  hipLaunchKernelGGL(qa::qa_idmatte_select, dim3(blocks), dim3(256), 0, StreamOf(c, stream), sp);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// the same source on the CPU (no GPU, no context).  One pixel: n samples' hit flags [n] and keys [n] (read where hit[s] != 0) -> the
// ranked table ids [8], counts [8], other [1]; any output may be null
int qa_test_idmatte_accumulate_host(const uint8_t *hit, const int32_t *keys, uint32_t n, int32_t *ids, uint32_t *counts, uint32_t *other)
{
  if (n && (!hit || !keys)) return QA_EINVAL;
  IdMatteAcc acc = idMatteInit();
  for (uint32_t s = 0; s < n; ++s) {
    if (hit[s] && keys[s] == QA_IDMATTE_EMPTY) return QA_EINVAL;   // (no key has the value of a free slot)
    idMatteSample(acc, hit[s] != 0, keys[s]);
  }
  idMatteRank(acc);
  for (int k = 0; k < QA_IDMATTE_SLOTS; ++k) {
    if (ids) ids[k] = acc.id[k];
    if (counts) counts[k] = acc.count[k];
  }
  if (other) *other = acc.other;
  return QA_OK;
}

int qa_test_idmatte_select_host(const int32_t *ids, const uint32_t *counts, const uint32_t *samples, uint64_t npix, const int32_t *select, uint32_t m,
                                float *out)
{
  if (!ids || !counts || !samples || !out || npix == 0 || m > QA_IDMATTE_MAX_SELECT || (m && !select)) return QA_EINVAL;
  for (uint64_t q = 0; q < npix; ++q) out[q] = idMatteSelect(ids + 8 * q, counts + 8 * q, samples[q], select, m);
  return QA_OK;
}

}  // extern "C"
