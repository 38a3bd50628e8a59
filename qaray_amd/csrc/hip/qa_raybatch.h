// qa_raybatch.h - what the entry points over a RayBatch share on the host (qa_radiance.hip: qa_integrate_rays; qa_irradiance.hip:
// qa_integrate_points): the picker of a kernel family's ten instances, the checks both refuse by, and the launch - a frame's
// (qa_frame.hip LaunchSetup / LaunchFrame) without tiles, chunks, tile lists and photon maps.  Host code only: each unit
// instantiates its own kernels.
#pragma once
#include <algorithm>
#include <cstring>

#include "qa_ctx.h"

typedef void (*RaysFn)(const DScene, const RenderParams, const RayBatch);

// The ten instances of kernel family K<RES, LIGHTS, TEX, AREA>: the five shadings PickShading lists (qa_mega.hip), for scenes in LDS
// and in global memory, by the predicates SelectKernel hands to PickKernel: plan.resident, num_lights > 0, plan.textured, plan.area
#define QA_PICK_RAYS_SHADING(K, RES)                                                                                      \
  (area ? (tex ? (RaysFn) K<RES, true, true, true> : (RaysFn) K<RES, true, false, true>)                                \
        : tex ? (RaysFn) K<RES, true, true, false> : lights ? (RaysFn) K<RES, true, false, false> : (RaysFn) K<RES, false, false, false>)
#define QA_DEFINE_RAYS_PICKER(NAME, K)                                                          \
  static RaysFn NAME(const qa_ctx *c)                                                           \
  {                                                                                             \
    const bool lights = c->ds.num_lights > 0, tex = c->plan.textured, area = c->plan.area;      \
    return c->plan.resident ? QA_PICK_RAYS_SHADING(K, true) : QA_PICK_RAYS_SHADING(K, false);   \
  }

#define QA_MAX_RAYS 0x7FFFFFFFull

// What the device and the host forms refuse alike, before anything is sized by n.  QA_OK with n == 0: nothing to do.
// flagsAllowed: the bits of qa_radiance_params::flags the entry knows; firstSegment: the batch's first segments are traced and may
// miss into the background
inline int RayBatchChecks(qa_ctx *c, uint64_t n, bool rays, bool dx, bool dy, bool screen, const qa_radiance_params *p, bool rgb, uint32_t flagsAllowed,
                          bool firstSegment)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (n == 0) return QA_OK;
  if (n > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 rays");
  if ((n + 63) / 64 * 64 >= 0xF0000000ull) return Fail(QA_EINVAL, "too many rays for the 32-bit work counter");   // (every exiting wave adds 64 more)
  if (!rays) return Fail(QA_EINVAL, "null ray array");
  if (!rgb) return Fail(QA_EINVAL, "null rgb output");
  if (!p) return Fail(QA_EINVAL, "null params");
  if (p->spp < 1 || p->max_bounce < 0) return Fail(QA_EINVAL, "bad spp / bounce");
  if (p->flags & ~flagsAllowed) return Fail(QA_EINVAL, "unknown flag bits");
  if (dx != dy) return Fail(QA_EINVAL, "one differential array without the other");
  if (c->plan.area && p->max_bounce + 1 > kMaxPath) return Fail(QA_EUNSUPPORTED, "area lights: maxBounce must be <= " + std::to_string(kMaxPath - 1));
  if (c->photonReady) return Fail(QA_EUNSUPPORTED, "photon maps are built: no gathering instance of the batch kernels is compiled (qa_photon_maps_clear first)");
  if (firstSegment && c->plan.textured && c->ds.bgTexmap >= 0 && !screen && !(p->flags & QA_RADIANCE_MISS_ENVIRONMENT))
    return Fail(QA_EINVAL, "the background has a texmap: give screen positions or QA_RADIANCE_MISS_ENVIRONMENT");
  return QA_OK;
}

// One batch on kernel `fn` (an instance of the unit's family, by its picker)
inline int LaunchRayBatch(qa_ctx *c, RaysFn fn, uint64_t n, const RayBatch &rb, const qa_radiance_params &p, float *rgb, float *t, uint32_t *ns, hipStream_t s)
{
  HIP_TRY(c->lastFrame.WaitOn(s));
  HIP_TRY(c->lastEdit.WaitOn(s));
  if (ns) HIP_TRY(hipMemsetAsync(ns, 0, n * sizeof(uint32_t), s));   // rays skipped by a stop request read as "not finished"
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned int), s));

  RenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.spp_min = rp.spp_max = p.spp;
  rp.max_bounce = p.max_bounce;
  rp.seed = p.seed;
  rp.tile_row_step = 1;
  rp.sync_samples = c->syncSamples < 0 ? c->plan.syncAuto : c->syncSamples;
  rp.rgb = rgb; rp.depth = t; rp.ns = ns;
  rp.work_counter = work;
  rp.stop_flag = c->dStopAlias;
  rp.counters = c->dCounters;
  rp.num_chunks = 1;

  const Integrator &mega = c->integ[kMega];   // the frames' LDS layout and stack depth (the tile lists' room stays unused)
  DScene ds = c->ds;
  ds.stackDepth = mega.stackDepth;
  ds.walkZeroTerms = c->optWalkZeroTerms;
  ds.lastCast = 0;
  ds.lastCastGlow = c->plan.lastCastGlow;

  // persistent grid of what is resident at once, at most 8 workgroups per CU: the area-light log is sized for that (EnsurePlanSlab)
  const long long needBlocks = (long long) ((n + QA_BLOCK - 1) / QA_BLOCK);
  const long long blocks = std::max<long long>(1, std::min<long long>(needBlocks, (long long) c->numCUs * OccupancyBlocks((KernelFn) fn, mega.ldsBytes)));

  EventPair ev;
  if (!c->freeEvents.empty()) { ev = c->freeEvents.back(); c->freeEvents.pop_back(); }
  else { HIP_TRY(hipEventCreate(&ev.a)); HIP_TRY(hipEventCreate(&ev.b)); }
  HIP_TRY(hipEventRecord(ev.a, s));
  hipLaunchKernelGGL(fn, dim3((unsigned) blocks), dim3(QA_BLOCK), (unsigned) mega.ldsBytes, s, ds, rp, rb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(c->lastFrame.Record(s));
  HIP_TRY(hipEventRecord(ev.b, s));
  c->pending.push_back(ev);
  c->launches++;
  if (c->pending.size() > 256) return DrainEvents(c);
  return QA_OK;
}
