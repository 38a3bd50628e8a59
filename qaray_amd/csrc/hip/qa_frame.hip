// qa_frame.hip — which integrator the uploaded scene runs on, the launch all frames share (one-shot frames here, the passes of
// qa_progressive.hip), and the one-shot frames of the C ABI (qa_render_*)
#include <algorithm>
#include <cstring>

#include "qa_ctx.h"
#include "qa_emptytile.h"

// The Halton table of at least `count` samples, made or grown as needed, and the scene record's pointer to it
int EnsureHalton(qa_ctx *c, int count)
{
  if (count > c->haltonCount) {
    int n = 64;
    while (n < count) n *= 2;
    std::vector<float> t(2 * (size_t) n);
    for (int s = 0; s < n; ++s) { t[2 * s] = HaltonF(s, 11); t[2 * s + 1] = HaltonF(s, 13); }
    // a frame or a pass on a stream of the caller's may still read the old table (its launch holds the old pointer)
    if (c->dHalton) { HIP_TRY(hipDeviceSynchronize()); (void) hipFree(c->dHalton); }
    c->dHalton = nullptr;
    HIP_TRY(hipMalloc((void **) &c->dHalton, t.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(c->dHalton, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    c->haltonCount = n;
  }
  c->ds.halton = c->dHalton;
  c->ds.halton_count = c->haltonCount;
  return QA_OK;
}

// The cooperative kernel's MANY variant (more shadow-casting lights than one batch; it always tests the nodes' bounds), and whether
// the variant chosen tests the nodes' bounds first (qa_kernel_cs.h): the textured variants always (it pays from a handful of nodes
// on: C3, 9 nodes, + 4 %), the untextured ones on scenes of more than 12 nodes (their register budget: see the kernel's comment).
// Both read the live plan: they agree with the kernels SelectKernel picked because every edit that changes the plan runs it again
static bool CsManyVariant(const qa_ctx *c) { return c->plan.shadowLights.size() > QA_CS_LIGHT_BATCH && !c->plan.area; }
// The resident variant whose bounce rays ask which emitter they meet (qa_kernel.h lastCastQuery)
static bool LastCastVariant(const qa_ctx *c) { return c->plan.resident && c->plan.lastCastQuery && c->ds.num_lights == 0; }
// Do one-shot frames finish empty tiles in closed form (qa_emptytile.h)?  The kernel that carries the shortcut, the option, and what the
// kernel itself asks for: tile lists (their LDS row holds the test's pyramid) and no depth of field
static int TileListLimit(const qa_ctx *c) { return c->plan.tileListBytes ? (c->optTileLists < 0 ? QA_TILE_LISTS_AUTO : c->optTileLists) : 0; }
static bool EmptyTilesOn(const qa_ctx *c)
{
  return LastCastVariant(c) && c->optEmptyTiles != 0 && TileListLimit(c) > 0 && !(c->ds.cam.dof > 0.1f);
}
static bool CsCullVariant(const qa_ctx *c) { return c->plan.csCullOk && (CsManyVariant(c) || c->plan.area || c->plan.textured || c->ds.num_inst > 12); }

// The name of a slot's integrator for the uploaded scene (qa_get_kernel_name)
static std::string IntegratorName(const qa_ctx *c, Slot s)
{
  const ScenePlan &p = c->plan;
  const int lights = c->ds.num_lights > 0;
  char name[160];
  if (s == kCs || s == kCsResume)
    snprintf(name, sizeof(name), "qa_integrate_cs%s<LIGHTS=%d,TEX=%d,CULL=%d%s%s>", s == kCsResume ? "_resume" : "", lights, (int) p.textured, (int) CsCullVariant(c),
             CsManyVariant(c) ? ",MANY=1" : "", p.area ? ",AREA=1" : "");
  else snprintf(name, sizeof(name), "qa_integrate<RES=%d,LIGHTS=%d,TEX=%d,AREA=%d%s>", (int) p.resident, lights, (int) p.textured, (int) p.area,
                s == kMega && LastCastVariant(c) ? ",LASTCAST=1" : "");
  std::string out = name;
  if (s == kPm || s == kPmStats) out += " + photon-map gathers (PHOTON=1)";
  if (s == kMegaStats || s == kPmStats) out += " counting variant (STATS=1, reference tree)";
  return out;
}
// The integrator the next plain frame is planned to run on.  What a frame really ran on (photon-map variants, counting
// kernels, frames the staged integrator refused) is recorded at launch: qa_get_kernel_name returns that once a frame has run.
void SetKernelName(qa_ctx *c)
{
  const WfHost &w = c->wf;
  if (w.eligible && w.mode == QA_PIPE_STAGED) {
    char buf[64];
    snprintf(buf, sizeof(buf), " (%d tile group%s)", w.numGroups, w.numGroups == 1 ? "" : "s");
    c->kernelName = std::string("staged: wf_logic + wf_cull + wf_trace + wf_redo") + buf;
  } else c->kernelName = IntegratorName(c, c->integ[kCs].fn ? kCs : kMega);
  c->launchedName.clear();
}

// Choose the kernel variants for the uploaded scene and size the persistent grid to what is
// resident at once (VGPR / LDS-limited workgroups per CU x CUs).
int SelectKernel(qa_ctx *c)
{
  const ScenePlan &p = c->plan;
  const bool lights = c->ds.num_lights > 0;
  Integrator &mega = c->integ[kMega], &cs = c->integ[kCs], &resume = c->integ[kCsResume];
  mega.fn = LastCastVariant(c) ? PickLastCastKernel() : PickKernel(p.resident, lights, p.textured, p.area, false);
  mega.ldsBytes = p.ldsBytes + p.tileListBytes;
  mega.blocksPerCU = OccupancyBlocks(mega.fn, mega.ldsBytes);
  mega.stackDepth = c->ds.stackDepth;
  c->integ[kMegaStats] = mega;
  c->integ[kMegaStats].fn = PickKernel(p.resident, lights, p.textured, p.area, true);
  // Cooperative mesh walks (qa_kernel_cs.h): scenes in global memory.  QA_COOP=0: off.
  // (any number of lights: their shadow queries are pooled QA_CS_LIGHT_BATCH = 4 lights at a time; with more than one batch the
  // surface waits in the slab DScene::csSurf between batches, qa_kernel_cs.h; area lights: the AREA variants, where every light is
  // evaluated when the path has ended, by the whole wave)
  cs.fn = nullptr;
  cs.stackDepth = c->ds.stackDepth;
  resume = cs;
  const char *e = DevEnv("QA_COOP");
  if (!p.resident && p.csFits && (p.shadowLights.size() <= QA_CS_LIGHT_BATCH || c->ds.csSurf) && cs.ldsBytes <= kMaxLdsPerBlock && c->optCoop && !(e && !strcmp(e, "0"))) {
    cs.fn = PickCs(lights, p.textured, CsCullVariant(c), CsManyVariant(c), p.area);
    cs.blocksPerCU = OccupancyBlocks(cs.fn, cs.ldsBytes);
    if (!p.textured) {
      resume.fn = PickCsResume(lights, CsCullVariant(c), CsManyVariant(c), p.area);
      resume.blocksPerCU = OccupancyBlocks(resume.fn, resume.ldsBytes);
    }
  }
  SetKernelName(c);
  if (FILE *report = Report(c))
    fprintf(report, "kernel %s: dynamic LDS per workgroup: megakernel %zu B (stack depth %u), cooperative %zu B (%u pool items, %u ray slots per wave); workgroups per CU: megakernel %d, cooperative %d\n",
            c->kernelName.c_str(), p.ldsBytes, c->ds.stackDepth, cs.ldsBytes, c->ds.csItems, c->ds.csSlots, mega.blocksPerCU, cs.fn ? cs.blocksPerCU : 0);
  return QA_OK;
}

static int OwnTileRows(int y0, int y1, int tile_row0, int tile_row_step)
{
  const int tilesY = (y1 - y0 + 7) / 8;
  if (tile_row0 >= tilesY) return 0;
  return (tilesY - tile_row0 + tile_row_step - 1) / tile_row_step;
}

// What qa_render_* and qa_progressive_begin refuse alike
int CheckFrame(qa_ctx *c, const FrameArgs &a)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (a.x0 < 0 || a.y0 < 0 || a.x1 > c->ds.cam.width || a.y1 > c->ds.cam.height || a.x1 <= a.x0 || a.y1 <= a.y0)
    return Fail(QA_EINVAL, "region outside the image");
  // sppMin = 0 would mean "no sample at all" (SuperSamplerHalton::Loop, src/scene/scene.cpp:92-97): refused
  if (a.sppMin < 1 || a.sppMax < a.sppMin || a.maxBounce < 0) return Fail(QA_EINVAL, "bad spp / bounce");
  if (c->plan.area && a.maxBounce + 1 > kMaxPath) return Fail(QA_EUNSUPPORTED, "area lights: maxBounce must be <= " + std::to_string(kMaxPath - 1));
  return QA_OK;
}

// The part of a launch one-shot frames and progressive passes share: the wait for the context's last frame, the render parameters
// (without the chunk fields), the tile order, the photon maps, the kernel variant and the grid.  resume: a progressive pass - every
// work item resumes a pixel, so the cooperative kernel's untextured variants run as their chunk-capable instances
int LaunchSetup(qa_ctx *c, Launch &L, const FrameArgs &a, int ownRows, unsigned int *work, bool resume)
{
  const hipStream_t s = a.stream;
  const int x0 = a.x0, y0 = a.y0, x1 = a.x1, y1 = a.y1;
  // one frame at a time per context (its device slabs are one per context): a frame on another stream than the last one waits for it
  HIP_TRY(c->lastFrame.WaitOn(s));
  HIP_TRY(c->lastEdit.WaitOn(s));   // a scene edit's copies run on the context's stream

  RenderParams &rp = L.rp;
  rp.x0 = x0; rp.y0 = y0; rp.x1 = x1; rp.y1 = y1;
  rp.spp_min = a.sppMin; rp.spp_max = a.sppMax; rp.max_bounce = a.maxBounce;
  rp.seed = a.seed;
  rp.tile_row0 = a.tileRow0; rp.tile_row_step = a.tileRowStep; rp.own_tile_rows = ownRows;
  // camera rays on per-tile leaf lists (qa_tilecull.h): where the scene's LDS plan has room for the lists (PlanScene)
  rp.tile_lists = TileListLimit(c);
  rp.sync_samples = c->syncSamples < 0 ? c->plan.syncAuto : c->syncSamples;
  rp.rgb = a.rgb; rp.depth = a.depth; rp.ns = a.ns;
  rp.work_counter = work;
  rp.tile_order = nullptr;
  {
    // Tiles are handed out centre-first: the cheap ones (rays that leave the scene at the image
    // border) end up last, so the end-of-frame tail is made of short tiles instead of long ones.
    const int tx = (x1 - x0 + 7) / 8;
    const uint64_t key = ((uint64_t) tx << 40) ^ ((uint64_t) ownRows << 20) ^ ((uint64_t) a.tileRow0 << 8) ^ (uint64_t) a.tileRowStep ^
                         ((uint64_t) (y1 - y0) << 50);
    if (key != c->orderKey || !c->dOrder) {
      const size_t n = (size_t) tx * ownRows;
      std::vector<std::pair<float, uint32_t>> v(n);
      const float cx = 0.5f * (x1 - x0), cy = 0.5f * (y1 - y0);
      for (int r = 0; r < ownRows; ++r)
        for (int i = 0; i < tx; ++i) {
          const float px = i * 8 + 4 - cx, py = (a.tileRow0 + r * a.tileRowStep) * 8 + 4 - cy;
          v[(size_t) r * tx + i] = {px * px + py * py, (uint32_t) (r * tx + i)};
        }
      std::stable_sort(v.begin(), v.end(), [](const std::pair<float, uint32_t> &a, const std::pair<float, uint32_t> &b) { return a.first < b.first; });
      std::vector<uint32_t> order(n);
      for (size_t i = 0; i < n; ++i) order[i] = v[i].second;
      if (c->dOrder) { HIP_TRY(hipStreamSynchronize(s)); (void) hipFree(c->dOrder); c->dOrder = nullptr; }
      HIP_TRY(hipMalloc((void **) &c->dOrder, n * sizeof(uint32_t)));
      HIP_TRY(hipMemcpyAsync(c->dOrder, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      HIP_TRY(hipStreamSynchronize(s));
      c->orderKey = key;
    }
    if (c->tileOrder) rp.tile_order = c->dOrder;
  }
  rp.stop_flag = c->dStopAlias;
  rp.counters = c->dCounters;
  // Scene::usePhotonMap: once qa_photon_maps_build has run, frames gather from the maps
  const bool pmOn = c->photonReady;
  memset(rp.pm, 0, sizeof(rp.pm));
  rp.heap = nullptr;
  if (pmOn) SetPhotonParams(c, rp);
  const bool stats = a.flags & QA_RENDER_STATS, cs = c->integ[kCs].fn && !pmOn && !stats;
  // (the textured cooperative variants carry the chunk code already: a progressive pass runs them as they are)
  L.slot = PickSlot(pmOn, stats, cs, resume && !c->plan.textured);
  DScene &ds = L.ds;
  ds = c->ds;
  ds.stackDepth = c->integ[L.slot].stackDepth;   // (the photon maps' kd-tree gather may need a deeper LDS stack than the scene)
  // the cooperative kernel's third way between "a lane starts its next sample at once" (0) and "when the whole wave is between samples"
  // (1): a finished path waits until 32 of the wave's have gathered, then those lanes finish and start samples together.  Where 1 was
  // the per-scene choice, and on scenes of many lights (an iteration is mostly their shadow batches), it beats both (experiments.txt 22)
  if (cs && c->syncSamples < 0 && ((c->plan.syncAuto && c->plan.textured) || CsManyVariant(c))) rp.sync_samples = 32;   // (the variants that carry the code)
  if (cs && c->plan.area) rp.sync_samples = 1;   // the cooperative AREA variants evaluate a wave's lights between its samples
  ds.csCullOn = (c->optCsCull && c->plan.csCullOk) ? 1u : 0u;
  ds.csForceExact = c->optCsForceExact;
  ds.walkZeroTerms = c->optWalkZeroTerms;
  ds.lastCast = (LastCastVariant(c) && c->optLastCast != 0) ? (c->optLeafSweep != 0 ? 2u : 1u) : 0u;   // (2: with the leaf sweep; inert where the query is off)
  ds.lastCastGlow = c->plan.lastCastGlow;
  ds.csPoolLimit = DevEnv("QA_CS_POOL") ? (uint32_t) std::max(64, atoi(DevEnv("QA_CS_POOL"))) : c->optCsPool;

  L.tiles = (unsigned) ((x1 - x0 + 7) / 8) * (unsigned) ownRows;
  const long long needBlocks = ((long long) L.tiles * 64 + QA_BLOCK - 1) / QA_BLOCK;
  L.blocks = (long long) c->numCUs * (c->optBlocksPerCU > 0 ? c->optBlocksPerCU : c->integ[L.slot].blocksPerCU);
  if (pmOn && L.blocks > (long long) c->numCUs * 8) L.blocks = (long long) c->numCUs * 8;   // the heap scratch is sized for this
  if (L.blocks > needBlocks) L.blocks = needBlocks;
  if (L.blocks < 1) L.blocks = 1;
  rp.chunk_spp = 0; rp.chunk_tail = 0; rp.num_chunks = 1; rp.tile_progress = nullptr; rp.pix_state = nullptr;
  rp.empty_tiles = (!resume && EmptyTilesOn(c)) ? 1u : 0u;
  return QA_OK;
}

// Launch what LaunchSetup planned (or the staged integrator), time it and record what ran
int LaunchFrame(qa_ctx *c, Launch &L, bool staged, hipStream_t s)
{
  EventPair ev;
  if (!c->freeEvents.empty()) { ev = c->freeEvents.back(); c->freeEvents.pop_back(); }
  else { HIP_TRY(hipEventCreate(&ev.a)); HIP_TRY(hipEventCreate(&ev.b)); }
  HIP_TRY(hipEventRecord(ev.a, s));
  if (staged) {
    // one event pair around the whole frame of the staged integrator (qa_wf.h)
    const int rc = RenderStaged(c, L.ds, L.rp, s, L.rp.counters);
    if (rc != QA_OK) { c->freeEvents.push_back(ev); return rc; }
  } else {
    hipLaunchKernelGGL(c->integ[L.slot].fn, dim3((unsigned) L.blocks), dim3(QA_BLOCK), (unsigned) c->integ[L.slot].ldsBytes, s, L.ds, L.rp);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(c->lastFrame.Record(s));
  HIP_TRY(hipEventRecord(ev.b, s));
  c->launchedName = staged ? c->kernelName : IntegratorName(c, L.slot);   // the kernel this frame really ran on
  c->pending.push_back(ev);
  c->launches++;
  // a caller that never asks for timers or counters must not grow the event list without bound
  if (c->pending.size() > 256) return DrainEvents(c);
  return QA_OK;
}

// One one-shot frame
static int Render(qa_ctx *c, const FrameArgs &a)
{
  if (int rc = CheckFrame(c, a)) return rc;
  if (!a.rgb || !a.depth || !a.ns) return Fail(QA_EINVAL, "null output buffer");
  if (int rc = EnsureHalton(c, a.sppMax)) return rc;
  if (a.tileRow0 < 0 || a.tileRowStep < 1) return Fail(QA_EINVAL, "bad strip partition");
  const int ownRows = OwnTileRows(a.y0, a.y1, a.tileRow0, a.tileRowStep);
  if (ownRows == 0) return QA_OK;  // nothing to do for this rank
  const hipStream_t s = a.stream;
  const bool whole = (a.tileRow0 == 0 && a.tileRowStep == 1);
  const size_t npix = (size_t) (a.x1 - a.x0) * (whole ? (size_t) (a.y1 - a.y0) : (size_t) ownRows * 8);
  // pixels skipped by a stop request (and the padding rows of a ragged last strip) read as "not rendered"
  HIP_TRY(hipMemsetAsync(a.ns, 0, npix * sizeof(uint32_t), s));
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned int), s));

  Launch L;
  if (int rc = LaunchSetup(c, L, a, ownRows, work, false)) return rc;
  RenderParams &rp = L.rp;
  const bool cs = L.slot == kCs;
  const int spp_max = a.sppMax;

  // ---- tiles in sample chunks (qa_kernel.h, section A): the per-lane kernels and the cooperative kernel's textured variants (in the
  // untextured ones the code costs more than their 4K frames' tails: 31 tiles per wave).  Per frame: when a wave gets fewer than 16 tiles, a tile's samples are handed out in chunks, so that
  // the frame ends on work items an eighth the size: half of them first, then eighths, where a wave's lanes start their samples
  // together (they also reach a chunk's end together); three quarters first where they do not (every hand-over then waits for the
  // tile's slowest pixel).  Cornell box 1080p @ 512 spp: 81.3 -> 72.5 ms (profiles/round03/chunk_sweep.txt).
  if ((!cs || c->plan.textured) && !(c->wf.mode == QA_PIPE_STAGED) && c->optChunkSpp != 0) {   // (cooperative kernel: the textured variants carry the code)
    uint32_t chunk = 0, tail = 0;
    if (c->optChunkSpp > 0) chunk = (uint32_t) c->optChunkSpp;
    else if ((long long) L.tiles < 16 * L.blocks * (QA_BLOCK / 64) && (long long) L.tiles >= L.blocks * (QA_BLOCK / 64) && spp_max >= 64)
      chunk = rp.sync_samples ? (uint32_t) spp_max / 2u : (uint32_t) spp_max - (uint32_t) spp_max / 4u;
    tail = c->optChunkTail > 0 ? (uint32_t) c->optChunkTail : std::max(16u, (uint32_t) spp_max / 8u);
    if (chunk > 0 && chunk < (uint32_t) spp_max) {
      const uint32_t nChunks = 1u + ((uint32_t) spp_max - chunk + tail - 1) / tail;
      if ((unsigned long long) L.tiles * 64ull * nChunks < 0xF0000000ull) {   // (the work counter is 32 bits; every exiting wave adds 64 more)
        // (8 words of state per pixel, one of progress per tile; a frame on any stream may still use the old slabs)
        HIP_TRY(c->pixState.Reserve((size_t) L.tiles * 64 * 8 * sizeof(uint32_t), true));
        HIP_TRY(c->tileProgress.Reserve(L.tiles * sizeof(uint32_t), true));
        HIP_TRY(hipMemsetAsync(c->tileProgress.p, 0, L.tiles * sizeof(uint32_t), s));
        rp.chunk_spp = chunk; rp.chunk_tail = tail; rp.num_chunks = nChunks; rp.tile_progress = (uint32_t *) c->tileProgress.p; rp.pix_state = (uint32_t *) c->pixState.p;
      }
    }
  }

  // ---- which integrator: both return the same bits.  The staged one (qa_wf.h) runs on request only (QA_PIPE_STAGED): since
  // the cooperative walks the megakernel is the faster one on every scene measured, and round 2's timed probe between the
  // two is gone.
  const bool staged = c->wf.mode == QA_PIPE_STAGED && StagedTakes(c, a.flags, spp_max, a.maxBounce, (size_t) L.tiles * 64);
  return LaunchFrame(c, L, staged, s);
}

int DrainEvents(qa_ctx *c)
{
  for (EventPair &ev : c->pending) {
    HIP_TRY(hipEventSynchronize(ev.b));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    c->totalMs += ms;
    c->freeEvents.push_back(ev);
  }
  c->pending.clear();
  return QA_OK;
}

extern "C" {

int qa_render_region_device(qa_ctx *c, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce,
                            uint32_t seed, uint32_t flags, float *d_rgb, float *d_depth, uint32_t *d_ns, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  return Render(c, {x0, y0, x1, y1, 0, 1, spp_min, spp_max, max_bounce, seed, flags, d_rgb, d_depth, d_ns, StreamOf(c, hip_stream)});
}

int qa_render_strips_device(qa_ctx *c, int x0, int y0, int x1, int y1, int first_strip, int strip_step, int spp_min,
                            int spp_max, int max_bounce, uint32_t seed, uint32_t flags, float *d_rgb, float *d_depth,
                            uint32_t *d_ns, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  return Render(c, {x0, y0, x1, y1, first_strip, strip_step, spp_min, spp_max, max_bounce, seed, flags, d_rgb, d_depth, d_ns, StreamOf(c, hip_stream)});
}

int qa_empty_tiles_device(qa_ctx *c, int x0, int y0, int x1, int y1, int first_strip, int strip_step, uint8_t *d_mask, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (x0 < 0 || y0 < 0 || x1 > c->ds.cam.width || y1 > c->ds.cam.height || x1 <= x0 || y1 <= y0) return Fail(QA_EINVAL, "region outside the image");
  if (!d_mask || first_strip < 0 || strip_step < 1) return Fail(QA_EINVAL, "bad argument");
  const int ownRows = OwnTileRows(y0, y1, first_strip, strip_step);
  if (ownRows == 0) return QA_OK;
  const hipStream_t s = StreamOf(c, hip_stream);
  const unsigned tiles = (unsigned) ((x1 - x0 + 7) / 8) * (unsigned) ownRows;
  HIP_TRY(c->lastEdit.WaitOn(s));   // a scene edit's copies run on the context's stream
  if (!EmptyTilesOn(c)) {           // a frame of this context finishes no tile in closed form
    HIP_TRY(hipMemsetAsync(d_mask, 0, tiles, s));
    return QA_OK;
  }
  RenderParams rp = {};
  rp.x0 = x0; rp.y0 = y0; rp.x1 = x1; rp.y1 = y1;
  rp.tile_row0 = first_strip; rp.tile_row_step = strip_step; rp.own_tile_rows = ownRows;
  // the kernel reads the instance and mesh tables an edit rewrites: ordered as the other read-only passes are (LaunchSceneKernel),
  // so that the next edit waits for it
  HIP_TRY(c->lastFrame.WaitOn(s));
  if (int rc = LaunchEmptyTileMask(c->ds, rp, tiles, d_mask, s)) return rc;
  HIP_TRY(c->lastFrame.Record(s));
  return QA_OK;
}

int qa_strip_count(int y0, int y1, int first_strip, int strip_step)
{
  if (y1 <= y0 || first_strip < 0 || strip_step < 1) return 0;
  return OwnTileRows(y0, y1, first_strip, strip_step);
}

int qa_render_region(qa_ctx *c, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce,
                     uint32_t seed, uint32_t flags, float *rgb, float *depth, uint32_t *ns)
{
  if (!c || !rgb || !depth || !ns) return Fail(QA_EINVAL, "null argument");
  if (x1 <= x0 || y1 <= y0) return Fail(QA_EINVAL, "empty region");
  HIP_TRY(hipSetDevice(c->device));
  // the staging only grows, and is only used synchronously: nothing to wait for before it is freed
  const size_t npix = (size_t) (x1 - x0) * (y1 - y0);
  HIP_TRY(c->stageRgb.Reserve(npix * 3 * sizeof(float)));
  HIP_TRY(c->stageDepth.Reserve(npix * sizeof(float)));
  HIP_TRY(c->stageNs.Reserve(npix * sizeof(uint32_t)));
  float *dRgb = (float *) c->stageRgb.p, *dDepth = (float *) c->stageDepth.p;
  uint32_t *dNs = (uint32_t *) c->stageNs.p;
  const int rc = Render(c, {x0, y0, x1, y1, 0, 1, spp_min, spp_max, max_bounce, seed, flags, dRgb, dDepth, dNs, c->stream});
  if (rc != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, dRgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(depth, dDepth, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(ns, dNs, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DrainEvents(c);   // the frame is complete: fold its event pair into the kernel time
}

}  // extern "C"
