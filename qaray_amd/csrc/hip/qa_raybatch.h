// qa_raybatch.h - what the entry points over a RayBatch share on the host (qa_radiance.hip: qa_integrate_rays; qa_irradiance.hip:
// qa_integrate_points; qa_radiance_pm.hip and qa_irradiance_pm.hip: their gathering siblings): the picker of a kernel family's ten
// instances and of a gathering family's eight, the checks both refuse by, and the launch - a frame's (qa_frame.hip LaunchSetup /
// LaunchFrame) without tiles, chunks and tile lists.  Host code only: each unit instantiates its own kernels.
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

// The eight instances of a gathering family K<RES, TEX, AREA> (QA_RADIANCE_PHOTON_MAPS; LIGHTS is true: a map needs a point light),
// by PickPmKernel's predicates (qa_photon.hip): plan.resident, plan.textured, plan.area.  Every one is reached by a committed scene
// (tests/test_gpu_radiance_photon.py, tests/test_gpu_irradiance_photon.py): none is left out
#define QA_PICK_PM_SHADING(K, RES) \
  (area ? (tex ? (RaysFn) K<RES, true, true> : (RaysFn) K<RES, false, true>) : (tex ? (RaysFn) K<RES, true, false> : (RaysFn) K<RES, false, false>))
#define QA_DEFINE_PM_PICKER(NAME, K)                                                        \
  RaysFn NAME(const qa_ctx *c)                                                              \
  {                                                                                         \
    const bool tex = c->plan.textured, area = c->plan.area;                                 \
    return c->plan.resident ? QA_PICK_PM_SHADING(K, true) : QA_PICK_PM_SHADING(K, false);   \
  }
// the gathering families' pickers: each is defined by the unit that holds the instances (qa_radiance_pm.hip, qa_irradiance_pm.hip)
// and called by the unit of the entry points
RaysFn PickRaysPm(const qa_ctx *c);
RaysFn PickPointsPm(const qa_ctx *c);
// does the batch gather from the photon maps?  (behind RayBatchChecks: p is not null there)
inline bool WantsPhotonMaps(const qa_radiance_params *p) { return (p->flags & QA_RADIANCE_PHOTON_MAPS) != 0; }

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
  // the maps are opt-in: a batch says what it wants (a frame changes silently once they are built)
  if (p->flags & QA_RADIANCE_PHOTON_MAPS) {
    if (!c->photonReady) return Fail(QA_ENOSCENE, "no photon maps built");
  } else if (c->photonReady)
    return Fail(QA_EUNSUPPORTED, "photon maps are built: a batch gathers from them with QA_RADIANCE_PHOTON_MAPS only (or qa_photon_maps_clear first)");
  if (firstSegment && c->plan.textured && c->ds.bgTexmap >= 0 && !screen && !(p->flags & QA_RADIANCE_MISS_ENVIRONMENT))
    return Fail(QA_EINVAL, "the background has a texmap: give screen positions or QA_RADIANCE_MISS_ENVIRONMENT");
  return QA_OK;
}

// One batch on kernel `fn` (an instance of the unit's family, by its picker; with QA_RADIANCE_PHOTON_MAPS of its gathering family).
// The wait for lastFrame and its record serialise a batch against the frames and batches of its context: that is also what keeps two
// users of the one heap slab of the photon gathers apart
inline int LaunchRayBatch(qa_ctx *c, RaysFn fn, uint64_t n, const RayBatch &rb, const qa_radiance_params &p, float *rgb, float *t, uint32_t *ns, hipStream_t s)
{
  const bool pm = WantsPhotonMaps(&p);
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
  if (pm) SetPhotonParams(c, rp);   // Scene::usePhotonMap = true, exactly as a frame would (memset above: null tables otherwise)

  // the frames' LDS layout and stack depth (the tile lists' room stays unused); gathering: the photon variants' (the kd-tree gather
  // may need a deeper stack than the scene)
  const Integrator &mega = c->integ[pm ? kPm : kMega];
  DScene ds = c->ds;
  ds.stackDepth = mega.stackDepth;
  ds.walkZeroTerms = c->optWalkZeroTerms;
  ds.lastCast = 0;
  ds.lastCastGlow = c->plan.lastCastGlow;

  // persistent grid of what is resident at once, at most 8 workgroups per CU: the area-light log is sized for that (EnsurePlanSlab),
  // and so is the heap slab of the gathers (qa_photon_maps_build: numCUs * 8 * QA_BLOCK lanes, indexed by blockIdx.x * QA_BLOCK + threadIdx.x)
  const long long needBlocks = (long long) ((n + QA_BLOCK - 1) / QA_BLOCK);
  const long long blocks = std::max<long long>(1, std::min<long long>(needBlocks, (long long) c->numCUs * std::min(8, OccupancyBlocks((KernelFn) fn, mega.ldsBytes))));

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
