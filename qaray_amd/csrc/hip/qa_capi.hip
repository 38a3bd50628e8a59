// qa_capi.hip — extern "C" surface of libqaray_hip.so (include/qaray_hip.h): context, scene
// upload (blob -> device tables), launches of the integrator kernel, counters and timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "qa_kernel_cs.h"
#include "qa_ctx.h"
#include "qa_scene_build.h"

static int EnsureHalton(qa_ctx *c, int count)
{
  if (count <= c->haltonCount) return QA_OK;
  int n = 64;
  while (n < count) n *= 2;
  std::vector<float> t(2 * (size_t) n);
  for (int s = 0; s < n; ++s) { t[2 * s] = HaltonF(s, 11); t[2 * s + 1] = HaltonF(s, 13); }
  if (c->dHalton) (void) hipFree(c->dHalton);
  c->dHalton = nullptr;
  HIP_TRY(hipMalloc((void **) &c->dHalton, t.size() * sizeof(float)));
  HIP_TRY(hipMemcpy(c->dHalton, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  c->haltonCount = n;
  return QA_OK;
}

// variants: scene memory (LDS-resident | global) x shading (no lights | lights | + textures | + area
// lights | + both) x stats
template <bool RES, bool STATS>
static KernelFn PickShading(bool lights, bool tex, bool area)
{
  if (area) return tex ? (KernelFn) qa_integrate<RES, true, true, true, STATS> : (KernelFn) qa_integrate<RES, true, false, true, STATS>;
  if (tex) return (KernelFn) qa_integrate<RES, true, true, false, STATS>;
  if (lights) return (KernelFn) qa_integrate<RES, true, false, false, STATS>;
  return (KernelFn) qa_integrate<RES, false, false, false, STATS>;
}
static KernelFn PickKernel(bool resident, bool lights, bool tex, bool area, bool stats)
{
  if (resident) return stats ? PickShading<true, true>(lights, tex, area) : PickShading<true, false>(lights, tex, area);
  return stats ? PickShading<false, true>(lights, tex, area) : PickShading<false, false>(lights, tex, area);
}

namespace qa {
// qa_debug_scrub_scratch: every lane fills its private segment (2 KB here, more than any kernel of this library uses) with one
// pattern and lingers, so that all wave slots of the chip are taken at once.  A frame that depends on the pattern reads scratch it
// never wrote (the compiler's spill-before-mask-restore hazard).
__global__ __launch_bounds__(256, 8) void qa_scrub_scratch(uint32_t pattern, uint32_t *never)
{
  volatile uint32_t a[512];
  for (int i = 0; i < 512; ++i) a[i] = pattern;
  for (int i = 0; i < 300; ++i) __builtin_amdgcn_s_sleep(127);
  if (a[threadIdx.x] == 0x12345u && pattern != 0x12345u) never[0] = 1;
}

// ---- progressive frames (qa_progressive_*): the pixel state slab is RenderParams::pix_state's layout, 8 words per pixel at its output
// index q (row-major in the region): [0] RNG state, [1] samples taken | bit 31 finished, [2..4] running mean, [5..7] running variance
// qa_progressive_begin: every pixel's fresh state (what qa_integrate's section A sets up for a pixel's first sample), nothing rendered
__global__ __launch_bounds__(256) void qa_prog_init(uint32_t *state, float *rgb, float *depth, uint32_t *ns, int x0, int y0, uint32_t rw, uint32_t npix,
                                                    uint32_t width, uint32_t seed)
{
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= npix) return;
  const uint32_t px = (uint32_t) x0 + q % rw, py = (uint32_t) y0 + q / rw;
  uint4 *st = reinterpret_cast<uint4 *>(state) + 2 * (size_t) q;
  st[0] = make_uint4(qa_pixel_seed(seed, py * width + px), 0u, 0u, 0u);
  st[1] = make_uint4(0u, 0u, 0u, 0u);
  rgb[3 * (size_t) q] = 0.f; rgb[3 * (size_t) q + 1] = 0.f; rgb[3 * (size_t) q + 2] = 0.f;
  depth[q] = QA_BIGFLOAT;
  ns[q] = 0u;
}
// after a pass to `target` samples: the tiles whose pass is complete are at the target now.  tile_progress is indexed by the work item's
// place in the pass's tile order (qa_integrate, section A: 2 once the item is complete); every word is 1 again for the next pass (its
// work items are all "chunk 1": the wait for chunk 0 ends at once)
__global__ __launch_bounds__(256) void qa_prog_levels(uint32_t *progress, const uint32_t *order, uint32_t *level, uint32_t tiles, uint32_t target)
{
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= tiles) return;
  if (progress[p] >= 2u) {
    const uint32_t t = order ? order[p] : p;
    if (level[t] < target) level[t] = target;
  }
  progress[p] = 1u;
}
// a pass to a target some tiles already reached (the same target again after a stop): only the tiles below it are handed out, so that
// no pixel takes a sample beyond the target.  They go, in launch order, to the END of list[tiles], and the pass's work counter starts
// so that its items are the last min(count, limit) of them.  One wave walks the order (a rare path; the order decides the schedule only)
__global__ __launch_bounds__(64) void qa_prog_select(const uint32_t *order, const uint32_t *level, uint32_t tiles, uint32_t target, uint32_t limit,
                                                     uint32_t *list, unsigned int *work)
{
  const uint32_t lane = threadIdx.x;
  uint32_t k = 0;   // tiles selected so far
  for (uint32_t b = 0; b < tiles; b += 64) {
    const bool valid = b + lane < tiles;
    const uint32_t p = valid ? tiles - 1u - (b + lane) : 0u;   // (backwards from the order's end)
    const uint32_t t = valid ? (order ? order[p] : p) : 0u;
    const bool need = valid && level[t] < target;
    const unsigned long long m = __ballot(need);
    if (need) list[tiles - 1u - (k + (uint32_t) __popcll(m & ((1ull << lane) - 1ull)))] = t;
    k += (uint32_t) __popcll(m);
  }
  if (lane == 0) *work = (2u * tiles - ((limit && limit < k) ? limit : k)) * 64u;
}
// the preview: finished pixels' final mean and sample count, the running mean and the samples so far of the others (rgb 0, ns 0 where
// nothing was taken yet); depth is sample 0's hit distance (1e30 before it)
__global__ __launch_bounds__(256) void qa_prog_resolve(const uint32_t *state, const float *rgb, const float *depth, const uint32_t *ns, uint32_t npix,
                                                       float *outRgb, float *outDepth, uint32_t *outNs)
{
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= npix) return;
  const uint4 a = reinterpret_cast<const uint4 *>(state)[2 * (size_t) q];
  const uint32_t mz = state[8 * (size_t) q + 4];
  if (a.y & 0x80000000u) {
    outRgb[3 * (size_t) q] = rgb[3 * (size_t) q]; outRgb[3 * (size_t) q + 1] = rgb[3 * (size_t) q + 1]; outRgb[3 * (size_t) q + 2] = rgb[3 * (size_t) q + 2];
    outNs[q] = ns[q];
  } else {
    outRgb[3 * (size_t) q] = __uint_as_float(a.z); outRgb[3 * (size_t) q + 1] = __uint_as_float(a.w); outRgb[3 * (size_t) q + 2] = __uint_as_float(mz);
    outNs[q] = a.y;
  }
  outDepth[q] = depth[q];
}
// qa_progressive_status: out[0] finished pixels, out[1] tiles below `target`, out[2] the lowest tile level (zeroed / set to ~0 before)
__global__ __launch_bounds__(256) void qa_prog_status(const uint32_t *state, uint32_t npix, const uint32_t *level, uint32_t tiles, uint32_t target,
                                                      unsigned long long *out)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool fin = i < npix && (state[8 * (size_t) i + 1] & 0x80000000u);
  const bool behind = i < tiles && level[i] < target;
  const unsigned long long mf = __ballot(fin), mb = __ballot(behind);
  if (__lane_id() == 0) {
    if (mf) atomicAdd(&out[0], (unsigned long long) __popcll(mf));
    if (mb) atomicAdd(&out[1], (unsigned long long) __popcll(mb));
  }
  if (i < tiles) atomicMin(&out[2], (unsigned long long) level[i]);
}
}  // namespace qa

static const char *kStagedName = "staged: wf_logic + wf_cull + wf_trace + wf_redo";
static std::string MegaName(const qa_ctx *c, bool cs)
{
  char name[160];
  if (cs) snprintf(name, sizeof(name), "qa_integrate_cs<LIGHTS=%d,TEX=%d,CULL=%d%s%s>", (int) (c->ds.num_lights > 0), (int) c->plan.textured, (int) c->csCullVariant,
                   c->csMany ? ",MANY=1" : "", c->plan.area ? ",AREA=1" : "");
  else snprintf(name, sizeof(name), "qa_integrate<RES=%d,LIGHTS=%d,TEX=%d,AREA=%d>", (int) c->plan.resident, (int) (c->ds.num_lights > 0), (int) c->plan.textured, (int) c->plan.area);
  return name;
}
// The integrator the next plain frame is planned to run on.  What a frame really ran on (photon-map variants, counting
// kernels, frames the staged integrator refused) is recorded at launch: qa_get_kernel_name returns that once a frame has run.
static void SetKernelName(qa_ctx *c)
{
  const WfHost &w = c->wf;
  if (w.eligible && w.mode == QA_PIPE_STAGED) {
    char buf[64];
    snprintf(buf, sizeof(buf), " (%d tile group%s)", w.numGroups, w.numGroups == 1 ? "" : "s");
    c->kernelName = std::string(kStagedName) + buf;
  } else c->kernelName = MegaName(c, c->kernelCs != nullptr);
  c->launchedName.clear();
}

// qa_integrate_cs variants; rows: no lights, lights, instance culling without / with lights, MANY, AREA; columns: textures
static KernelFn PickCs(bool lights, bool tex, bool cull, bool many, bool area)
{
  static const KernelFn k[6][2] = {
      {(KernelFn) qa_integrate_cs<false, false, false, false>, (KernelFn) qa_integrate_cs<false, true, false, false>},
      {(KernelFn) qa_integrate_cs<true, false, false, false>, (KernelFn) qa_integrate_cs<true, true, false, false>},
      {(KernelFn) qa_integrate_cs<false, false, true, false>, (KernelFn) qa_integrate_cs<false, true, true, false>},
      {(KernelFn) qa_integrate_cs<true, false, true, false>, (KernelFn) qa_integrate_cs<true, true, true, false>},
      {(KernelFn) qa_integrate_cs<true, false, true, true>, (KernelFn) qa_integrate_cs<true, true, true, true>},
      {(KernelFn) qa_integrate_cs<true, false, true, false, true>, (KernelFn) qa_integrate_cs<true, true, true, false, true>}};
  return k[area ? 5 : many ? 4 : 2 * cull + lights][tex];
}
// ... their untextured rows as chunk-capable instances (qa_integrate_cs_resume): the passes of progressive frames
static KernelFn PickCsResume(bool lights, bool cull, bool many, bool area)
{
  static const KernelFn k[6] = {(KernelFn) qa_integrate_cs_resume<false, false, false, false>, (KernelFn) qa_integrate_cs_resume<true, false, false, false>,
                                (KernelFn) qa_integrate_cs_resume<false, false, true, false>, (KernelFn) qa_integrate_cs_resume<true, false, true, false>,
                                (KernelFn) qa_integrate_cs_resume<true, false, true, true>, (KernelFn) qa_integrate_cs_resume<true, false, true, false, true>};
  return k[area ? 5 : many ? 4 : 2 * cull + lights];
}

// where the upload report goes ("verbose", QA_FAST_VERBOSE), else null
static FILE *Report(const qa_ctx *c) { return (c->optVerbose || DevEnv("QA_FAST_VERBOSE")) ? stderr : nullptr; }

// Choose the kernel variant for the uploaded scene and size the persistent grid to what is
// resident at once (VGPR / LDS-limited workgroups per CU x CUs).
static int SelectKernel(qa_ctx *c)
{
  const ScenePlan &p = c->plan;
  const bool lights = c->ds.num_lights > 0;
  c->kernel = PickKernel(p.resident, lights, p.textured, p.area, false);
  c->kernelStats = PickKernel(p.resident, lights, p.textured, p.area, true);
  int resident = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, (const void *) c->kernel, QA_BLOCK, p.ldsBytes) != hipSuccess || resident < 1)
    resident = 2;
  c->blocksPerCUAuto = resident > 8 ? 8 : resident;
  // Cooperative mesh walks (qa_kernel_cs.h): scenes in global memory without area lights.  QA_COOP=0: off.
  // (any number of lights: their shadow queries are pooled QA_CS_LIGHT_BATCH = 4 lights at a time; with more than one batch the
  // surface waits in the slab DScene::csSurf between batches, qa_kernel_cs.h; area lights: the AREA variants)
  c->kernelCs = nullptr;
  c->kernelCsResume = nullptr;
  c->csMany = false;
  const char *e = DevEnv("QA_COOP");
  const size_t shadowLights = p.shadowLights.size();
  if (!p.resident && p.csFits && (shadowLights <= QA_CS_LIGHT_BATCH || c->ds.csSurf) && c->ldsBytesCs <= kMaxLdsPerBlock && c->optCoop && !(e && !strcmp(e, "0"))) {
    // instance culling (qa_kernel_cs.h): the textured variants always (it pays from a handful of nodes on: C3, 9 nodes, + 4 %), the
    // untextured ones on scenes of more than 12 nodes (their register budget: see the kernel's comment)
    c->csCullVariant = p.csCullOk && (p.textured || c->ds.num_inst > 12);
    c->csMany = shadowLights > QA_CS_LIGHT_BATCH && !p.area;   // (those variants always test the nodes' bounds)
    if (c->csMany || p.area) c->csCullVariant = p.csCullOk;
    // AREA: every light is evaluated when the path has ended, by the whole wave (qa_kernel_cs.h)
    c->kernelCs = PickCs(lights, p.textured, c->csCullVariant, c->csMany, p.area);
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *) c->kernelCs, QA_BLOCK, c->ldsBytesCs) != hipSuccess || n < 1) n = 2;
    c->blocksPerCUCs = n > 8 ? 8 : n;
    if (!p.textured) {
      c->kernelCsResume = PickCsResume(lights, c->csCullVariant, c->csMany, p.area);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *) c->kernelCsResume, QA_BLOCK, c->ldsBytesCs) != hipSuccess || n < 1) n = 2;
      c->blocksPerCUCsResume = n > 8 ? 8 : n;
    }
  }
  SetKernelName(c);
  if (FILE *report = Report(c))
    fprintf(report, "kernel %s: dynamic LDS per workgroup: megakernel %zu B (stack depth %u), cooperative %zu B (%u pool items, %u ray slots per wave); workgroups per CU: megakernel %d, cooperative %d\n",
            c->kernelName.c_str(), p.ldsBytes, c->ds.stackDepth, c->ldsBytesCs, c->ds.csItems, c->ds.csSlots, c->blocksPerCUAuto, c->kernelCs ? c->blocksPerCUCs : 0);
  return QA_OK;
}

// The per-thread slab c->plan needs, if any, made on first need and kept with the scene; c->ds points at the one the plan uses
static int EnsurePlanSlab(qa_ctx *c)
{
  const size_t threads = (size_t) c->numCUs * 8 * QA_BLOCK;
  const bool area = c->plan.area, many = !area && c->plan.shadowLights.size() > QA_CS_LIGHT_BATCH;
  float **slab = area ? &c->dAreaSlab : many ? &c->dSurfSlab : nullptr;
  if (slab && !*slab) {
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, threads * (area ? QA_MAX_PATH * QA_REC_FLOATS : 13) * sizeof(float)));
    c->sceneAllocs.push_back(p);
    c->statSceneAllocs++;
    *slab = static_cast<float *>(p);
  }
  c->ds.areaScratch = area ? c->dAreaSlab : nullptr;
  c->ds.csSurf = many ? c->dSurfSlab : nullptr;
  return QA_OK;
}

// Copy the built tables to the device: the only place a scene allocates device memory (but for the slab of a plan an edit brings)
static int UploadScene(qa_ctx *c, const SceneTables &t)
{
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  DScene &ds = c->ds;
  ds = t.ds;
  c->plan = t.plan;
  ds.blob = c->dBlob;
  ds.inst = QA_BLOB_PTR(qa_instance, c->dBlob, h->off_instances);
  ds.mtlset = QA_BLOB_PTR(qa_mtlset, c->dBlob, h->off_mtlsets);
  ds.light = QA_BLOB_PTR(qa_light, c->dBlob, h->off_lights);
  ds.texmap = QA_BLOB_PTR(qa_texmap, c->dBlob, h->off_texmaps);
  ds.tex = QA_BLOB_PTR(qa_texture, c->dBlob, h->off_textures);
  int rc;
  for (size_t mi = 0; mi < t.mesh.size(); ++mi) {
    const MeshTables &m = t.mesh[mi];
    DMesh &dm = c->plan.meshes[mi];
    if ((rc = DeviceCopy(c, m.vt, &dm.vt)) || (rc = DeviceCopy(c, m.nodes, &dm.nodes)) || (rc = DeviceCopy(c, m.tris, &dm.tris)) ||
        (rc = DeviceCopy(c, m.shade, &dm.shade)) || (rc = DeviceCopy(c, m.fnodes, &dm.fnodes)) || (rc = DeviceCopy(c, m.ftris, &dm.ftris)) ||
        (rc = DeviceCopy(c, m.fmap, &dm.fmap)) || (rc = DeviceCopy(c, m.wide.nodes, &dm.wnodes)) || (rc = DeviceCopy(c, m.wtris, &dm.wtris)))
      return rc;
  }
  if ((rc = DeviceCopy(c, t.csNodes, &ds.csNodes)) || (rc = DeviceCopy(c, t.csTris, &ds.csTris)) || (rc = DeviceCopy(c, t.csLeafBox, &ds.csLeafBox)) ||
      (rc = DeviceCopy(c, t.csCull, &ds.csCull)) || (rc = DeviceCopy(c, t.csInst, &ds.csInst)) ||
      (rc = DeviceCopy(c, c->plan.meshes, &ds.mesh)) || (rc = DeviceCopy(c, t.materials, &ds.mtl)))
    return rc;
  // per-thread slabs of the largest grid: the AREA variants' hit log (QA_MAX_PATH x 19 floats), and the surface qa_integrate_cs
  // parks between batches when there are more shadow-casting lights than one batch
  if ((rc = EnsurePlanSlab(c)) != QA_OK) return rc;
  if ((rc = DeviceCopy(c, t.mtlTex, &ds.mtlTex)) || (rc = DeviceCopy(c, t.texels, &ds.texels)) || (rc = DeviceCopy(c, t.texOff, &ds.texOff)) ||
      (rc = DeviceCopy(c, t.taps, &ds.texFilter)))
    return rc;
  if (t.plan.resident) {
    if ((rc = DeviceCopy(c, t.image, &ds.resident))) return rc;
    std::copy(c->plan.meshes.begin(), c->plan.meshes.end(), ds.meshv);
  }
  // qa_integrate_cs: per wave [ray slots | results | flags | pool items | accumulators]; four workgroups per CU (160 KB LDS)
  c->ldsBytesCs = (size_t) CsLdsWords(ds.csItems, ds.csSlots) * (QA_BLOCK / 64) * sizeof(uint32_t);
  return QA_OK;
}

// Validate the blob, build the tables and upload them, then choose the integrator
static int PrepareScene(qa_ctx *c)
{
  auto env = [](const char *name, uint32_t dflt) { const char *e = DevEnv(name); return e ? (uint32_t) atoi(e) : dflt; };
  BuildKnobs k;
  k.wide = env("QA_WIDE", 1) != 0;
  k.wideLeaf = env("QA_WIDE_LEAF", k.wideLeaf);
  k.fastLeaf = env("QA_FAST_LEAF", k.fastLeaf);
  k.fastMaxFaces = env("QA_FAST_MAXFACES", k.fastMaxFaces);
  k.csItems = env("QA_CS_ITEMS", k.csItems);
  k.csSlots = env("QA_CS_SLOTS", k.csSlots);
  k.report = Report(c);
  SceneTables &t = c->tables;
  std::string err;
  int rc = BuildScene(c->hostBlob.data(), c->hostBlob.size(), k, t, &err);
  c->statMeshBuilds += t.meshBuilds;
  if (rc != QA_OK) return Fail(rc, err);
  if ((rc = UploadScene(c, t)) != QA_OK) return rc;
  // scene edits build the scene-side tables again from these (qa_scene_edit_*): the mesh side is on the device now
  DropMeshSide(t);
  c->knobs = k;
  c->knobs.report = nullptr;
  c->statEdits = 0;
  c->haveScene = true;
  SelectStaged(c);
  return SelectKernel(c);
}

static int DrainEvents(qa_ctx *c);

static int OwnTileRows(int y0, int y1, int tile_row0, int tile_row_step)
{
  const int tilesY = (y1 - y0 + 7) / 8;
  if (tile_row0 >= tilesY) return 0;
  return (tilesY - tile_row0 + tile_row_step - 1) / tile_row_step;
}

// What qa_render_* and qa_progressive_begin refuse alike
static int CheckFrame(qa_ctx *c, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (x0 < 0 || y0 < 0 || x1 > c->ds.cam.width || y1 > c->ds.cam.height || x1 <= x0 || y1 <= y0)
    return Fail(QA_EINVAL, "region outside the image");
  // sppMin = 0 would mean "no sample at all" (SuperSamplerHalton::Loop, src/scene/scene.cpp:92-97): refused
  if (spp_min < 1 || spp_max < spp_min || max_bounce < 0) return Fail(QA_EINVAL, "bad spp / bounce");
  if (c->plan.area && max_bounce + 1 > QA_MAX_PATH) return Fail(QA_EUNSUPPORTED, "area lights: maxBounce must be <= 7");
  return QA_OK;
}

// One launch of the megakernel as LaunchSetup plans it
struct Launch {
  RenderParams rp;
  DScene ds;
  KernelFn kernel = nullptr;
  size_t ldsBytes = 0;
  long long blocks = 1;
  unsigned tiles = 0;
  bool cs = false, pmOn = false, csResume = false;
};

// The part of a launch one-shot frames and progressive passes share: the wait for the context's last frame, the render parameters
// (without the chunk fields), the tile order, the photon maps, the kernel variant and the grid.  resume: a progressive pass - every
// work item resumes a pixel, so the cooperative kernel's untextured variants run as their chunk-capable instances
static int LaunchSetup(qa_ctx *c, Launch &L, int x0, int y0, int x1, int y1, int tile_row0, int tile_row_step, int ownRows, int spp_min,
                       int spp_max, int max_bounce, uint32_t seed, uint32_t flags, float *d_rgb, float *d_depth, uint32_t *d_ns,
                       unsigned int *work, hipStream_t s, bool resume)
{
  // one frame at a time per context (its device slabs are one per context): a frame on another stream than the last one waits for it
  if (!c->chunkEv) HIP_TRY(hipEventCreateWithFlags(&c->chunkEv, hipEventDisableTiming));
  if (c->chunkEvSet && s != c->lastStream) HIP_TRY(hipStreamWaitEvent(s, c->chunkEv, 0));
  if (c->editEvSet && s != c->stream) HIP_TRY(hipStreamWaitEvent(s, c->editEv, 0));   // a scene edit's copies run on the context's stream

  RenderParams &rp = L.rp;
  rp.x0 = x0; rp.y0 = y0; rp.x1 = x1; rp.y1 = y1;
  rp.spp_min = spp_min; rp.spp_max = spp_max; rp.max_bounce = max_bounce;
  rp.seed = seed;
  rp.tile_row0 = tile_row0; rp.tile_row_step = tile_row_step; rp.own_tile_rows = ownRows; rp.pad = 0;
  rp.sync_samples = c->syncSamples < 0 ? c->plan.syncAuto : c->syncSamples;
  rp.rgb = d_rgb; rp.depth = d_depth; rp.ns = d_ns;
  rp.work_counter = work;
  rp.tile_order = nullptr;
  {
    // Tiles are handed out centre-first: the cheap ones (rays that leave the scene at the image
    // border) end up last, so the end-of-frame tail is made of short tiles instead of long ones.
    const int tx = (x1 - x0 + 7) / 8;
    const uint64_t key = ((uint64_t) tx << 40) ^ ((uint64_t) ownRows << 20) ^ ((uint64_t) tile_row0 << 8) ^ (uint64_t) tile_row_step ^
                         ((uint64_t) (y1 - y0) << 50);
    if (key != c->orderKey || !c->dOrder) {
      const size_t n = (size_t) tx * ownRows;
      std::vector<std::pair<float, uint32_t>> v(n);
      const float cx = 0.5f * (x1 - x0), cy = 0.5f * (y1 - y0);
      for (int r = 0; r < ownRows; ++r)
        for (int i = 0; i < tx; ++i) {
          const float px = i * 8 + 4 - cx, py = (tile_row0 + r * tile_row_step) * 8 + 4 - cy;
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
  if (pmOn) {
    for (int k = 0; k < 2; ++k) {
      const qa_photon_map_params &mp = k ? c->photonParams.caustics : c->photonParams.photon;
      rp.pm[k].node = static_cast<const uint4 *>(c->dPmTables[k][0]);
      rp.pm[k].dir = static_cast<const float4 *>(c->dPmTables[k][1]);
      rp.pm[k].power = static_cast<const float4 *>(c->dPmTables[k][2]);
      rp.pm[k].count = mp.size;
      rp.pm[k].half = (int32_t) (mp.size / 2) - 1;   // halfStoredPhotons = (photons.size() - 1) / 2 - 1, cyPhotonMap.h:291
      rp.pm[k].radius = mp.radius;
    }
    rp.heap = static_cast<uint2 *>(c->dHeap);
  }
  DScene &ds = L.ds;
  ds = c->ds;
  if (pmOn) ds.stackDepth = c->stackDepthPm;
  const bool cs = c->kernelCs && !pmOn && !(flags & QA_RENDER_STATS);
  // the cooperative kernel's third way between "a lane starts its next sample at once" (0) and "when the whole wave is between samples"
  // (1): a finished path waits until 32 of the wave's have gathered, then those lanes finish and start samples together.  Where 1 was
  // the per-scene choice, and on scenes of many lights (an iteration is mostly their shadow batches), it beats both (experiments.txt 22)
  if (cs && c->syncSamples < 0 && ((c->plan.syncAuto && c->plan.textured) || c->csMany)) rp.sync_samples = 32;   // (the variants that carry the code)
  if (cs && c->plan.area) rp.sync_samples = 1;   // the cooperative AREA variants evaluate a wave's lights between its samples
  ds.csCullOn = (c->optCsCull && c->plan.csCullOk) ? 1u : 0u;
  ds.csForceExact = c->optCsForceExact;
  ds.walkZeroTerms = c->optWalkZeroTerms;
  ds.csPoolLimit = DevEnv("QA_CS_POOL") ? (uint32_t) std::max(64, atoi(DevEnv("QA_CS_POOL"))) : c->optCsPool;
  L.ldsBytes = pmOn ? c->ldsBytesPm : (cs ? c->ldsBytesCs : c->plan.ldsBytes);
  // (the textured cooperative variants carry the chunk code already: a progressive pass runs them as they are)
  L.csResume = cs && resume && !c->plan.textured;
  const KernelFn csKernel = L.csResume ? c->kernelCsResume : c->kernelCs;
  L.kernel = pmOn ? ((flags & QA_RENDER_STATS) ? c->kernelPmStats : c->kernelPm)
                  : ((flags & QA_RENDER_STATS) ? c->kernelStats : (cs ? csKernel : c->kernel));

  L.tiles = (unsigned) ((x1 - x0 + 7) / 8) * (unsigned) ownRows;
  const long long needBlocks = ((long long) L.tiles * 64 + QA_BLOCK - 1) / QA_BLOCK;
  const int csBlocks = L.csResume ? c->blocksPerCUCsResume : c->blocksPerCUCs;
  L.blocks = (long long) c->numCUs * (c->blocksPerCU > 0 ? c->blocksPerCU : (pmOn ? c->blocksPerCUPm : (cs ? csBlocks : c->blocksPerCUAuto)));
  if (pmOn && L.blocks > (long long) c->numCUs * 8) L.blocks = (long long) c->numCUs * 8;   // the heap scratch is sized for this
  if (L.blocks > needBlocks) L.blocks = needBlocks;
  if (L.blocks < 1) L.blocks = 1;
  L.cs = cs;
  L.pmOn = pmOn;
  rp.chunk_spp = 0; rp.chunk_tail = 0; rp.num_chunks = 1; rp.chunk_pad = 0; rp.tile_progress = nullptr; rp.pix_state = nullptr;
  return QA_OK;
}

// Launch what LaunchSetup planned (or the staged integrator), time it and record what ran
static int LaunchFrame(qa_ctx *c, Launch &L, uint32_t flags, bool staged, hipStream_t s)
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
    hipLaunchKernelGGL(L.kernel, dim3((unsigned) L.blocks), dim3(QA_BLOCK), (unsigned) L.ldsBytes, s, L.ds, L.rp);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->chunkEv, s));
  c->chunkEvSet = true;
  c->lastStream = s;
  HIP_TRY(hipEventRecord(ev.b, s));
  {
    // the kernel this frame really ran on
    if (staged) c->launchedName = c->kernelName;
    else {
      c->launchedName = MegaName(c, L.cs);
      if (L.csResume) c->launchedName.replace(0, strlen("qa_integrate_cs"), "qa_integrate_cs_resume");
      if (L.pmOn) c->launchedName += " + photon-map gathers (PHOTON=1)";
      if (flags & QA_RENDER_STATS) c->launchedName += " counting variant (STATS=1, reference tree)";
    }
  }
  c->pending.push_back(ev);
  c->launches++;
  // a caller that never asks for timers or counters must not grow the event list without bound
  if (c->pending.size() > 256) return DrainEvents(c);
  return QA_OK;
}

static int Render(qa_ctx *c, int x0, int y0, int x1, int y1, int tile_row0, int tile_row_step, int spp_min, int spp_max,
                  int max_bounce, uint32_t seed, uint32_t flags, float *d_rgb, float *d_depth, uint32_t *d_ns, hipStream_t s)
{
  int rc = CheckFrame(c, x0, y0, x1, y1, spp_min, spp_max, max_bounce);
  if (rc != QA_OK) return rc;
  if (!d_rgb || !d_depth || !d_ns) return Fail(QA_EINVAL, "null output buffer");
  rc = EnsureHalton(c, spp_max);
  if (rc != QA_OK) return rc;
  c->ds.halton = c->dHalton;
  c->ds.halton_count = c->haltonCount;

  if (tile_row0 < 0 || tile_row_step < 1) return Fail(QA_EINVAL, "bad strip partition");
  const int ownRows = OwnTileRows(y0, y1, tile_row0, tile_row_step);
  if (ownRows == 0) return QA_OK;  // nothing to do for this rank
  const bool whole = (tile_row0 == 0 && tile_row_step == 1);
  const size_t npix = (size_t) (x1 - x0) * (whole ? (size_t) (y1 - y0) : (size_t) ownRows * 8);
  // pixels skipped by a stop request (and the padding rows of a ragged last strip) read as "not rendered"
  HIP_TRY(hipMemsetAsync(d_ns, 0, npix * sizeof(uint32_t), s));
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned int), s));

  Launch L;
  rc = LaunchSetup(c, L, x0, y0, x1, y1, tile_row0, tile_row_step, ownRows, spp_min, spp_max, max_bounce, seed, flags, d_rgb, d_depth, d_ns,
                   work, s, false);
  if (rc != QA_OK) return rc;
  RenderParams &rp = L.rp;
  const bool cs = L.cs;
  const unsigned tiles = L.tiles;
  const long long blocks = L.blocks;

  // ---- tiles in sample chunks (qa_kernel.h, section A): the per-lane kernels and the cooperative kernel's textured variants (in the
  // untextured ones the code costs more than their 4K frames' tails: 31 tiles per wave).  Per frame: when a wave gets fewer than 16 tiles, a tile's samples are handed out in chunks, so that
  // the frame ends on work items an eighth the size: half of them first, then eighths, where a wave's lanes start their samples
  // together (they also reach a chunk's end together); three quarters first where they do not (every hand-over then waits for the
  // tile's slowest pixel).  Cornell box 1080p @ 512 spp: 81.3 -> 72.5 ms (profiles/round03/chunk_sweep.txt).
  if ((!cs || c->plan.textured) && !(c->wf.mode == QA_PIPE_STAGED) && c->optChunkSpp != 0) {   // (cooperative kernel: the textured variants carry the code)
    uint32_t chunk = 0, tail = 0;
    if (c->optChunkSpp > 0) chunk = (uint32_t) c->optChunkSpp;
    else if ((long long) tiles < 16 * blocks * (QA_BLOCK / 64) && (long long) tiles >= blocks * (QA_BLOCK / 64) && spp_max >= 64)
      chunk = rp.sync_samples ? (uint32_t) spp_max / 2u : (uint32_t) spp_max - (uint32_t) spp_max / 4u;
    tail = c->optChunkTail > 0 ? (uint32_t) c->optChunkTail : std::max(16u, (uint32_t) spp_max / 8u);
    if (chunk > 0 && chunk < (uint32_t) spp_max) {
      const uint32_t nChunks = 1u + ((uint32_t) spp_max - chunk + tail - 1) / tail;
      if ((unsigned long long) tiles * 64ull * nChunks < 0xF0000000ull) {   // (the work counter is 32 bits; every exiting wave adds 64 more)
        const size_t needState = (size_t) tiles * 64 * 8, needProg = tiles;
        if (needState > c->pixStateWords) {
          if (c->dPixState) { HIP_TRY(hipDeviceSynchronize()); (void) hipFree(c->dPixState); c->dPixState = nullptr; c->pixStateWords = 0; }
          HIP_TRY(hipMalloc((void **) &c->dPixState, needState * sizeof(uint32_t)));
          c->pixStateWords = needState;
        }
        if (needProg > c->tileProgressWords) {
          if (c->dTileProgress) { HIP_TRY(hipDeviceSynchronize()); (void) hipFree(c->dTileProgress); c->dTileProgress = nullptr; c->tileProgressWords = 0; }
          HIP_TRY(hipMalloc((void **) &c->dTileProgress, needProg * sizeof(uint32_t)));
          c->tileProgressWords = needProg;
        }
        HIP_TRY(hipMemsetAsync(c->dTileProgress, 0, needProg * sizeof(uint32_t), s));
        rp.chunk_spp = chunk; rp.chunk_tail = tail; rp.num_chunks = nChunks; rp.tile_progress = c->dTileProgress; rp.pix_state = c->dPixState;
      }
    }
  }

  // ---- which integrator: both return the same bits.  The staged one (qa_wf.h) runs on request only (QA_PIPE_STAGED): since
  // the cooperative walks the megakernel is the faster one on every scene measured, and round 2's timed probe between the
  // two is gone.
  const bool staged = c->wf.mode == QA_PIPE_STAGED && StagedTakes(c, flags, spp_max, max_bounce, (size_t) tiles * 64);
  return LaunchFrame(c, L, flags, staged, s);
}

static int DrainEvents(qa_ctx *c)
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

__global__ void qa_sincos_probe(const float *x, int n, float *s, float *c)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { s[i] = qsinf(x[i]); c[i] = qcosf(x[i]); }
}

__global__ void qa_math_probe(int fn, const float *x, const float *y, int n, float *out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (fn) {
    case 0: out[i] = qsinf(x[i]); break;
    case 1: out[i] = qcosf(x[i]); break;
    case 2: out[i] = qpowf(x[i], y[i]); break;
    case 3: out[i] = qexpf(x[i]); break;
    case 4: out[i] = qasinf(x[i]); break;
    case 5: out[i] = sphereU(x[i], y[i]); break;
    default: out[i] = sphereV(x[i], y[i]); break;
  }
}

extern "C" {

// the device build of qa_device_math.h: fn 0 sinf, 1 cosf, 2 powf(x, y), 3 expf, 4 asinf; and of the sphere's texture
// coordinates (qa_texture_dev.h): 5 u from (p.x = x, p.y = y), 6 v from (p.z = x, rcp_l = y) (host arrays in / out)
int qa_test_math_device(int fn, const float *x, const float *y, int n, float *out)
{
  if (!x || !out || n <= 0 || fn < 0 || fn > 6 || ((fn == 2 || fn == 5 || fn == 6) && !y)) return Fail(QA_EINVAL, "bad argument");
  float *dx = nullptr, *dy = nullptr, *dout = nullptr;
  HIP_TRY(hipMalloc((void **) &dx, n * sizeof(float)));
  HIP_TRY(hipMalloc((void **) &dy, n * sizeof(float)));
  HIP_TRY(hipMalloc((void **) &dout, n * sizeof(float)));
  HIP_TRY(hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice));
  if (y) HIP_TRY(hipMemcpy(dy, y, n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qa_math_probe, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, dy, n, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, n * sizeof(float), hipMemcpyDeviceToHost));
  (void) hipFree(dx); (void) hipFree(dy); (void) hipFree(dout);
  return QA_OK;
}

// Self-test hooks: the device math next to the host libm (tests/test_gpu_parity.py, tests/test_device_math.py)
int qa_test_sincosf_device(const float *x, int n, float *s, float *c)
{
  if (!x || !s || !c || n <= 0) return Fail(QA_EINVAL, "bad argument");
  float *dx = nullptr, *dsn = nullptr, *dcs = nullptr;
  HIP_TRY(hipMalloc((void **) &dx, n * sizeof(float)));
  HIP_TRY(hipMalloc((void **) &dsn, n * sizeof(float)));
  HIP_TRY(hipMalloc((void **) &dcs, n * sizeof(float)));
  HIP_TRY(hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qa_sincos_probe, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, dsn, dcs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(s, dsn, n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(c, dcs, n * sizeof(float), hipMemcpyDeviceToHost));
  (void) hipFree(dx); (void) hipFree(dsn); (void) hipFree(dcs);
  return QA_OK;
}
// the same source compiled for the host (no GPU needed)
int qa_test_math_host(int fn, const float *x, const float *y, int n, float *out)
{
  if (!x || !out || n <= 0) return QA_EINVAL;
  for (int i = 0; i < n; ++i) {
    switch (fn) {
      case 0: out[i] = qsinf(x[i]); break;
      case 1: out[i] = qcosf(x[i]); break;
      case 2: out[i] = qpowf(x[i], y ? y[i] : 1.f); break;
      case 3: out[i] = qexpf(x[i]); break;
      case 4: out[i] = qasinf(x[i]); break;
      case 5: if (!y) return QA_EINVAL; out[i] = sphereU(x[i], y[i]); break;
      case 6: if (!y) return QA_EINVAL; out[i] = sphereV(x[i], y[i]); break;
      default: return QA_EINVAL;
    }
  }
  return QA_OK;
}

}  // extern "C"

// ---- texture probes: one query of qa_texture_dev.h per lane (device) or loop step (host), QA_TEXPROBE_IN floats in and
// QA_TEXPROBE_OUT out per query; the ops are listed in include/qaray_hip.h.  tris / vt: the record and texture vertices of the
// probed triangle (op 8), else null.
#define QA_TEXPROBE_IN 16
#define QA_TEXPROBE_OUT 9

__host__ __device__ inline void TexProbeOne(const TexTables &tt, const DTri *tris, const float *vt, int op, int index, const float *in,
                                            float *out)
{
  const f3 a = ld3(in), b = ld3(in + 3), c = ld3(in + 6), d = ld3(in + 9), e = ld3(in + 12);
  TexHit t;
  t.uvw = t.duvw0 = t.duvw1 = F3(0, 0, 0);
  t.hasTexture = false;
  switch (op) {
    case 0: t.uvw = tileClamp(a); break;
    case 1: t.uvw = textureSample(tt, index, a); break;
    case 2: t.uvw = textureSampleFiltered(tt, index, a, b, c); break;
    case 3: t.uvw = texColorSample(tt, b, index, a); break;
    case 4: {
      TexHit h;
      h.uvw = a; h.duvw0 = b; h.duvw1 = c; h.hasTexture = in[15] != 0.f;
      t.uvw = mtlSample(tt, h, d, index);
      break;
    }
    case 5: t.uvw = sampleEnvironment(tt, b, index, a); break;
    case 6: texPlane(a, b, c, d, t); break;
    case 7: texSphere(a, b, c, d, e, t); break;
    case 8: {
      const uint4 *q = reinterpret_cast<const uint4 *>(tris);
      texTriangle(q[0], q[1], q[2], vt, a, b, c, in[9], in[10], t);
      break;
    }
    default: {   // 9: the conversion helper, its int's bits in out[0]
      const int k = qa_f2i_x86(in[0]);
      __builtin_memcpy(&t.uvw.x, &k, 4);
      break;
    }
  }
  const f3 r[3] = {t.uvw, t.duvw0, t.duvw1};
  for (int k = 0; k < 3; ++k) { out[3 * k] = r[k].x; out[3 * k + 1] = r[k].y; out[3 * k + 2] = r[k].z; }
}

__global__ void qa_texture_probe(TexTables tt, const DTri *tris, const float *vt, int op, int index, int n, const float *in, float *out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) TexProbeOne(tt, tris, vt, op, index, in + (size_t) QA_TEXPROBE_IN * i, out + (size_t) QA_TEXPROBE_OUT * i);
}

// The table an op reads must exist: 1, 2 a texture; 3-5 a texmap (a negative one is the plain colour); 8 element (index & 0xFFFFF)
// of mesh (index >> 20), which must have texture vertices.  -> false when it does not
static bool TexProbeArgsOk(const qa_flat_header *h, const ScenePlan &p, int op, int index, int n, int *mesh, int *elem)
{
  if (n <= 0 || op < 0 || op > 9) return false;
  if (op == 1 || op == 2) return index >= 0 && (uint32_t) index < h->num_textures;
  if (op >= 3 && op <= 5) return index < (int) h->num_texmaps;
  if (op == 8) {
    *mesh = index >> 20;
    *elem = index & 0xFFFFF;
    return index >= 0 && (size_t) *mesh < p.meshes.size() && p.meshes[*mesh].hasVT && (uint32_t) *elem < p.meshes[*mesh].num_faces;
  }
  return true;
}

extern "C" {

int qa_test_texture_device(qa_ctx *c, int op, int index, int n, const float *in, float *out)
{
  if (!c || !in || !out || c->hostBlob.empty()) return Fail(QA_EINVAL, "bad argument");
  int mesh = 0, elem = 0;
  if (!TexProbeArgsOk(reinterpret_cast<const qa_flat_header *>(c->hostBlob.data()), c->plan, op, index, n, &mesh, &elem))
    return Fail(QA_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  TexTables tt;
  tt.blob = c->ds.blob;
  tt.texels = c->ds.texels;
  tt.texOff = c->ds.texOff;
  tt.texmap = c->ds.texmap;
  tt.tex = c->ds.tex;
  tt.filter = c->ds.texFilter;
  const DTri *tris = op == 8 ? c->plan.meshes[mesh].tris + elem : nullptr;
  const float *vt = op == 8 ? c->plan.meshes[mesh].vt + 6 * (size_t) elem : nullptr;
  float *din = nullptr, *dout = nullptr;
  HIP_TRY(hipMalloc((void **) &din, (size_t) n * QA_TEXPROBE_IN * sizeof(float)));
  HIP_TRY(hipMalloc((void **) &dout, (size_t) n * QA_TEXPROBE_OUT * sizeof(float)));
  HIP_TRY(hipMemcpy(din, in, (size_t) n * QA_TEXPROBE_IN * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qa_texture_probe, dim3((n + 255) / 256), dim3(256), 0, 0, tt, tris, vt, op, index, n, din, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, (size_t) n * QA_TEXPROBE_OUT * sizeof(float), hipMemcpyDeviceToHost));
  (void) hipFree(din); (void) hipFree(dout);
  return QA_OK;
}

int qa_test_texture_host(const void *blob, int op, int index, int n, const float *in, float *out)
{
  if (!in || !out || n <= 0) return QA_EINVAL;
  if (op == 0 || op == 9) {   // (no table: no scene needed)
    for (int i = 0; i < n; ++i) TexProbeOne(TexTables(), nullptr, nullptr, op, index, in + (size_t) QA_TEXPROBE_IN * i, out + (size_t) QA_TEXPROBE_OUT * i);
    return QA_OK;
  }
  if (!blob) return QA_EINVAL;
  const qa_flat_header *h = static_cast<const qa_flat_header *>(blob);
  if (h->magic != QA_FLAT_MAGIC || h->version != QA_FLAT_VERSION) return QA_EINVAL;
  SceneTables t;
  std::string err;
  const int rc = BuildScene(static_cast<const unsigned char *>(blob), h->total_bytes, BuildKnobs(), t, &err);
  if (rc != QA_OK) return rc;
  int mesh = 0, elem = 0;
  if (!TexProbeArgsOk(h, t.plan, op, index, n, &mesh, &elem)) return QA_EINVAL;
  TexTables tt;
  tt.blob = static_cast<const unsigned char *>(blob);
  tt.texels = reinterpret_cast<const float4 *>(t.texels.data());
  tt.texOff = t.texOff.data();
  tt.texmap = QA_BLOB_PTR(qa_texmap, blob, h->off_texmaps);
  tt.tex = QA_BLOB_PTR(qa_texture, blob, h->off_textures);
  tt.filter = t.taps.data();
  const DTri *tris = op == 8 ? t.mesh[mesh].tris.data() + elem : nullptr;
  const float *vt = op == 8 ? t.mesh[mesh].vt.data() + 6 * (size_t) elem : nullptr;
  for (int i = 0; i < n; ++i) TexProbeOne(tt, tris, vt, op, index, in + (size_t) QA_TEXPROBE_IN * i, out + (size_t) QA_TEXPROBE_OUT * i);
  return QA_OK;
}

const char *qa_last_error(void) { return g_err.c_str(); }

int qa_ctx_create(int device_id, qa_ctx **out)
{
  if (!out) return Fail(QA_EINVAL, "null argument");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return Fail(QA_EHIP, "no HIP device: the qaray HIP path has no CPU fallback");
  if (device_id < 0 || device_id >= n) return Fail(QA_EINVAL, "device id out of range");
  HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  qa_ctx *c = new (std::nothrow) qa_ctx;
  if (!c) return Fail(QA_ENOMEM, "out of memory");
  c->device = device_id;
  c->numCUs = prop.multiProcessorCount;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipMalloc((void **) &c->dWork, qa_ctx::kCounterRing * sizeof(unsigned int))) != hipSuccess ||
      (e = hipMalloc((void **) &c->dCounters, sizeof(DCounters))) != hipSuccess ||
      (e = hipMemset(c->dCounters, 0, sizeof(DCounters))) != hipSuccess ||
      (e = hipHostMalloc((void **) &c->hStop, sizeof(int), hipHostMallocMapped)) != hipSuccess) {
    qa_ctx_destroy(c);
    return Fail(QA_EHIP, std::string("context setup: ") + hipGetErrorString(e));
  }
  *c->hStop = 0;
  if (const char *e = DevEnv("QA_SYNC")) c->syncSamples = atoi(e);
  c->tileOrder = DevEnv("QA_NO_TILE_ORDER") == nullptr;
  if (const char *e = DevEnv("QA_WF_BUDGET")) c->wf.budget = atoi(e) > 0 ? (uint32_t) atoi(e) : 512u;
  if (const char *e = DevEnv("QA_WF_GATE")) c->wf.gate = (uint32_t) std::max(1, atoi(e));
  // (tile groups of the staged integrator: one unless qa_set_option("staged_groups") says otherwise - several groups only pay
  // when the process gave the HIP runtime a hardware queue per group stream, GPU_MAX_HW_QUEUES >= 8 before its first call)
  if (const char *e = DevEnv("QA_WF_REDO_ASYNC")) c->wf.redoAsync = atoi(e) != 0;
  if (const char *e = DevEnv("QA_WF_GROUPS")) c->wf.numGroups = std::max(1, std::min(atoi(e), (int) WfHost::kMaxGroups));
  if (const char *e = DevEnv("QA_WF_STACK")) c->wf.stackCap = atoi(e) > 1 ? (uint32_t) atoi(e) : 24u;
  if (const char *e = DevEnv("QA_WF_BLOCKS")) c->wf.traceBlocksPerCU = atoi(e);
  if ((e = hipHostGetDevicePointer((void **) &c->dStopAlias, c->hStop, 0)) != hipSuccess) {
    qa_ctx_destroy(c);
    return Fail(QA_EHIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
  }
  *out = c;
  return QA_OK;
}

int qa_ctx_destroy(qa_ctx *c)
{
  if (!c) return QA_OK;
  (void) hipSetDevice(c->device);
  if (c->stream) (void) hipStreamSynchronize(c->stream);
  FreeScene(c);
  FreeStaged(c);
  for (EventPair &ev : c->pending) { (void) hipEventDestroy(ev.a); (void) hipEventDestroy(ev.b); }
  for (EventPair &ev : c->freeEvents) { (void) hipEventDestroy(ev.a); (void) hipEventDestroy(ev.b); }
  if (c->dHalton) (void) hipFree(c->dHalton);
  if (c->dOrder) (void) hipFree(c->dOrder);
  if (c->dWork) (void) hipFree(c->dWork);
  if (c->dPixState) (void) hipFree(c->dPixState);
  if (c->dTileProgress) (void) hipFree(c->dTileProgress);
  if (c->chunkEv) (void) hipEventDestroy(c->chunkEv);
  if (c->editEv) (void) hipEventDestroy(c->editEv);
  if (c->hEditStage) (void) hipHostFree(c->hEditStage);
  if (c->prog.done) (void) hipEventDestroy(c->prog.done);
  if (c->dCounters) (void) hipFree(c->dCounters);
  if (c->hStop) (void) hipHostFree(c->hStop);
  if (c->dRgb) (void) hipFree(c->dRgb);
  if (c->dDepth) (void) hipFree(c->dDepth);
  if (c->dNs) (void) hipFree(c->dNs);
  if (c->dDisplay) (void) hipFree(c->dDisplay);
  if (c->dDisplayStage) (void) hipFree(c->dDisplayStage);
  if (c->displayEv) (void) hipEventDestroy(c->displayEv);
  if (c->stream) (void) hipStreamDestroy(c->stream);
  delete c;
  return QA_OK;
}

int qa_scene_upload(qa_ctx *c, const void *host_blob, uint64_t nbytes)
{
  if (!c || !host_blob || nbytes == 0) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  FreeScene(c);
  try {
    c->hostBlob.assign((const unsigned char *) host_blob, (const unsigned char *) host_blob + nbytes);
  } catch (const std::bad_alloc &) { return Fail(QA_ENOMEM, "out of memory"); }
  HIP_TRY(hipMalloc((void **) &c->dBlob, nbytes));
  c->statSceneAllocs++;
  HIP_TRY(hipMemcpy(c->dBlob, host_blob, nbytes, hipMemcpyHostToDevice));
  c->statBytesCopied = nbytes;
  const int rc = PrepareScene(c);
  if (rc != QA_OK) FreeScene(c);
  return rc;
}

int qa_scene_upload_device(qa_ctx *c, const void *device_blob, uint64_t nbytes)
{
  if (!c || !device_blob || nbytes == 0) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  FreeScene(c);
  try { c->hostBlob.resize(nbytes); } catch (const std::bad_alloc &) { return Fail(QA_ENOMEM, "out of memory"); }
  HIP_TRY(hipMalloc((void **) &c->dBlob, nbytes));
  c->statSceneAllocs++;
  HIP_TRY(hipMemcpy(c->dBlob, device_blob, nbytes, hipMemcpyDeviceToDevice));
  c->statBytesCopied = nbytes;
  HIP_TRY(hipMemcpy(c->hostBlob.data(), device_blob, nbytes, hipMemcpyDeviceToHost));
  const int rc = PrepareScene(c);
  if (rc != QA_OK) FreeScene(c);
  return rc;
}

}  // extern "C"

// ---- scene edits (qa_scene_edit_*) ----------------------------------------------------------------------------------------------
// c->tables (rebuilt from the edited host blob) -> the context's plan and scene record, device pointers kept; the slab the plan needs
static int ApplySceneSide(qa_ctx *c)
{
  const SceneTables &t = c->tables;
  std::vector<DMesh> meshes = std::move(c->plan.meshes);   // (the device copies' pointers live here; no edit changes a DMesh)
  c->plan = t.plan;
  c->plan.meshes = std::move(meshes);
  DScene &ds = c->ds;
  ds.cam = t.ds.cam;
  ds.rootIdentity = t.ds.rootIdentity;
  ds.csCullS1 = t.ds.csCullS1; ds.csCullS2 = t.ds.csCullS2; ds.csCullK3 = t.ds.csCullK3; ds.csCullK4 = t.ds.csCullK4;
  memcpy(ds.instv, t.ds.instv, sizeof(ds.instv));
  return EnsurePlanSlab(c);
}

struct EditCopy { const void *dst; const void *src; size_t bytes; };

// The copies of one edit: through the pinned ring, asynchronously on the context's stream
static int EnqueueEditCopies(qa_ctx *c, const std::vector<EditCopy> &copies)
{
  size_t need = 0;
  for (const EditCopy &k : copies) need += (k.bytes + 63) & ~(size_t) 63;
  if (!c->editEv) HIP_TRY(hipEventCreateWithFlags(&c->editEv, hipEventDisableTiming));
  if (need > c->editStageBytes) {
    if (c->editEvSet) HIP_TRY(hipEventSynchronize(c->editEv));
    if (c->hEditStage) (void) hipHostFree(c->hEditStage);
    c->hEditStage = nullptr;
    c->editStageBytes = c->editStageUsed = 0;
    const size_t bytes = std::max<size_t>(256 * 1024, 8 * need);
    HIP_TRY(hipHostMalloc((void **) &c->hEditStage, bytes, hipHostMallocDefault));
    c->editStageBytes = bytes;
  }
  if (c->editStageUsed + need > c->editStageBytes) {   // the ring wraps: the copies of the edits before this one must have left it
    if (c->editEvSet) HIP_TRY(hipEventSynchronize(c->editEv));
    c->editStageUsed = 0;
  }
  // a frame on a stream of the caller's may still read the tables
  if (c->chunkEvSet && c->lastStream != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->chunkEv, 0));
  if (c->prog.done && c->prog.active) HIP_TRY(hipStreamWaitEvent(c->stream, c->prog.done, 0));
  c->statBytesCopied = 0;
  for (const EditCopy &k : copies) {
    if (!k.bytes || !k.dst) continue;
    unsigned char *stage = c->hEditStage + c->editStageUsed;
    memcpy(stage, k.src, k.bytes);
    HIP_TRY(hipMemcpyAsync(const_cast<void *>(k.dst), stage, k.bytes, hipMemcpyHostToDevice, c->stream));
    c->editStageUsed += (k.bytes + 63) & ~(size_t) 63;
    c->statBytesCopied += k.bytes;
  }
  HIP_TRY(hipEventRecord(c->editEv, c->stream));
  c->editEvSet = true;
  return QA_OK;
}

enum EditKind { kEditCamera, kEditLights, kEditMaterials, kEditInstances };

// Writes `bytes` at `off` of the resident blob, rebuilds the scene side and brings the context to the state an upload of the
// edited blob would leave; a refusal leaves everything as it was
static int ApplyEdit(qa_ctx *c, EditKind kind, size_t off, const void *src, size_t bytes)
{
  HIP_TRY(hipSetDevice(c->device));
  unsigned char *at = c->hostBlob.data() + off;
  std::vector<unsigned char> old(at, at + bytes);
  memcpy(at, src, bytes);
  std::string err;
  int rc = RebuildSceneSide(c->hostBlob.data(), c->hostBlob.size(), c->knobs, c->tables, &err);
  if (rc != QA_OK) Fail(rc, err);
  else rc = ApplySceneSide(c);
  if (rc != QA_OK) {
    const std::string why = g_err;
    memcpy(at, old.data(), bytes);
    if (RebuildSceneSide(c->hostBlob.data(), c->hostBlob.size(), c->knobs, c->tables, &err) == QA_OK) (void) ApplySceneSide(c);
    return Fail(rc, why);
  }
  const SceneTables &t = c->tables;
  std::vector<EditCopy> copies;
  copies.push_back({c->dBlob + off, at, bytes});
  if (kind == kEditMaterials) {
    copies.push_back({c->ds.mtl, t.materials.data(), t.materials.size() * sizeof(DMaterial)});
    if (c->plan.resident) copies.push_back({c->ds.resident, t.image.data(), t.image.size() * sizeof(uint4)});
  } else if (kind == kEditInstances) {
    copies.push_back({c->ds.csInst, t.csInst.data(), t.csInst.size() * sizeof(CsInst)});
    copies.push_back({c->ds.csCull, t.csCull.data(), t.csCull.size() * sizeof(CsCull)});
  }
  if ((rc = EnqueueEditCopies(c, copies)) != QA_OK) return rc;
  if (kind == kEditCamera) SetKernelName(c);   // (the plan cannot change; the name is the plan's again, as after an upload)
  else {
    // Scene::usePhotonMap ends as with an upload; the maps' memory goes with the next upload, build, clear or the context
    // (releasing it here would wait for the device)
    c->photonReady = false;
    SelectStaged(c);
    if ((rc = SelectKernel(c)) != QA_OK) return rc;
  }
  if (c->prog.active) c->prog.stale = true;
  c->statEdits++;
  return QA_OK;
}

static int EditArgs(qa_ctx *c, const void *records, uint32_t first, uint32_t n, uint32_t count)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (!records) return Fail(QA_EINVAL, "null argument");
  if (first > count || n > count - first) return Fail(QA_EINVAL, "records beyond the scene's table");
  return QA_OK;
}

extern "C" {

int qa_scene_edit_camera(qa_ctx *c, const qa_camera *cam)
{
  int rc = EditArgs(c, cam, 0, 0, 0);
  if (rc != QA_OK) return rc;
  static_assert(offsetof(qa_flat_header, dof) + sizeof(float) - offsetof(qa_flat_header, screenA) == sizeof(qa_camera), "qa_camera is the header's camera block");
  return ApplyEdit(c, kEditCamera, offsetof(qa_flat_header, screenA), cam, sizeof(qa_camera));
}

int qa_scene_edit_lights(qa_ctx *c, uint32_t first, uint32_t n, const qa_light *lights)
{
  int rc = EditArgs(c, lights, first, n, c && c->haveScene ? reinterpret_cast<const qa_flat_header *>(c->hostBlob.data())->num_lights : 0);
  if (rc != QA_OK || n == 0) return rc;
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  return ApplyEdit(c, kEditLights, h->off_lights + (size_t) first * sizeof(qa_light), lights, (size_t) n * sizeof(qa_light));
}

int qa_scene_edit_materials(qa_ctx *c, uint32_t first, uint32_t n, const qa_material *materials)
{
  int rc = EditArgs(c, materials, first, n, c && c->haveScene ? reinterpret_cast<const qa_flat_header *>(c->hostBlob.data())->num_materials : 0);
  if (rc != QA_OK || n == 0) return rc;
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  const qa_material *cur = QA_BLOB_PTR(qa_material, c->hostBlob.data(), h->off_materials) + first;
  for (uint32_t i = 0; i < n; ++i) {
    const qa_material &a = cur[i], &b = materials[i];
    if (a.diffuse.texmap != b.diffuse.texmap || a.specular.texmap != b.specular.texmap || a.reflection.texmap != b.reflection.texmap ||
        a.refraction.texmap != b.refraction.texmap || a.emission.texmap != b.emission.texmap)
      return Fail(QA_EINVAL, "a material edit cannot change texture-map references (texture tables are not rebuilt): upload the scene instead");
  }
  return ApplyEdit(c, kEditMaterials, h->off_materials + (size_t) first * sizeof(qa_material), materials, (size_t) n * sizeof(qa_material));
}

int qa_scene_edit_instances(qa_ctx *c, uint32_t first, uint32_t n, const qa_instance *instances)
{
  int rc = EditArgs(c, instances, first, n, c && c->haveScene ? reinterpret_cast<const qa_flat_header *>(c->hostBlob.data())->num_instances : 0);
  if (rc != QA_OK || n == 0) return rc;
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  const qa_instance *cur = QA_BLOB_PTR(qa_instance, c->hostBlob.data(), h->off_instances) + first;
  for (uint32_t i = 0; i < n; ++i) {
    const qa_instance &a = cur[i], &b = instances[i];
    if (a.obj_type != b.obj_type || a.mesh != b.mesh || a.mtlset != b.mtlset || a.parent != b.parent || a.subtree_end != b.subtree_end ||
        a.depth != b.depth)
      return Fail(QA_EINVAL, "an instance edit can change tm, itm and pos only (object, mesh, material set and place in the graph stay): upload the scene instead");
  }
  return ApplyEdit(c, kEditInstances, h->off_instances + (size_t) first * sizeof(qa_instance), instances, (size_t) n * sizeof(qa_instance));
}

int qa_scene_download(qa_ctx *c, void *out, uint64_t capacity, uint64_t *nbytes)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (nbytes) *nbytes = c->hostBlob.size();
  if (!out || capacity < c->hostBlob.size()) return Fail(QA_EINVAL, "output smaller than the scene blob");
  memcpy(out, c->hostBlob.data(), c->hostBlob.size());
  return QA_OK;
}

int qa_get_scene_stats(qa_ctx *c, uint64_t out[4])
{
  if (!c || !out) return Fail(QA_EINVAL, "null argument");
  out[0] = c->statMeshBuilds; out[1] = c->statSceneAllocs; out[2] = c->statBytesCopied; out[3] = c->statEdits;
  return QA_OK;
}

int qa_render_region_device(qa_ctx *c, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce,
                            uint32_t seed, uint32_t flags, float *d_rgb, float *d_depth, uint32_t *d_ns, void *hip_stream)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t) hip_stream : c->stream;
  return Render(c, x0, y0, x1, y1, 0, 1, spp_min, spp_max, max_bounce, seed, flags, d_rgb, d_depth, d_ns, s);
}

int qa_render_strips_device(qa_ctx *c, int x0, int y0, int x1, int y1, int first_strip, int strip_step, int spp_min,
                            int spp_max, int max_bounce, uint32_t seed, uint32_t flags, float *d_rgb, float *d_depth,
                            uint32_t *d_ns, void *hip_stream)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t) hip_stream : c->stream;
  return Render(c, x0, y0, x1, y1, first_strip, strip_step, spp_min, spp_max, max_bounce, seed, flags, d_rgb, d_depth, d_ns, s);
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
  const size_t npix = (size_t) (x1 - x0) * (y1 - y0);
  if (npix > c->stagePixels) {
    if (c->dRgb) (void) hipFree(c->dRgb);
    if (c->dDepth) (void) hipFree(c->dDepth);
    if (c->dNs) (void) hipFree(c->dNs);
    c->dRgb = c->dDepth = nullptr;
    c->dNs = nullptr;
    c->stagePixels = 0;
    HIP_TRY(hipMalloc((void **) &c->dRgb, npix * 3 * sizeof(float)));
    HIP_TRY(hipMalloc((void **) &c->dDepth, npix * sizeof(float)));
    HIP_TRY(hipMalloc((void **) &c->dNs, npix * sizeof(uint32_t)));
    c->stagePixels = npix;
  }
  const int rc = Render(c, x0, y0, x1, y1, 0, 1, spp_min, spp_max, max_bounce, seed, flags, c->dRgb, c->dDepth, c->dNs, c->stream);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, c->dRgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(depth, c->dDepth, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(ns, c->dNs, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DrainEvents(c);   // the frame is complete: fold its event pair into the kernel time
}

int qa_synchronize(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DrainEvents(c);
}

int qa_request_stop(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  __atomic_store_n(c->hStop, 1, __ATOMIC_SEQ_CST);
  return QA_OK;
}
int qa_clear_stop(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  __atomic_store_n(c->hStop, 0, __ATOMIC_SEQ_CST);
  return QA_OK;
}

int qa_get_counters(qa_ctx *c, qa_counters *out)
{
  if (!c || !out) return Fail(QA_EINVAL, "null argument");
  int rc = qa_synchronize(c);
  if (rc != QA_OK) return rc;
  DCounters h;
  HIP_TRY(hipMemcpy(&h, c->dCounters, sizeof(h), hipMemcpyDeviceToHost));
  out->samples = h.samples;
  out->casts_normal = h.casts_normal;
  out->casts_shadow = h.casts_shadow;
  out->bvh_nodes = h.bvh_nodes;
  out->tri_tests = h.tri_tests;
  out->pixels = h.pixels;
#ifdef QA_STAMPS
  {
    const double w = (double) std::max<unsigned long long>(h.stamp[9], 1), k = (double) std::max<unsigned long long>(h.stamp[0], 1);
    fprintf(stderr, "[stamps] waves %llu, iterations/wave %.0f, cycles/wave %.3e | share of wave time: fetch+start %.3f, closest %.3f (mesh walks %.3f), shade %.3f, "
            "direct light %.3f (shadow mesh walks %.3f), sample end %.3f, miss branch %.3f, hit before shading %.3f, spawn %.3f\n", h.stamp[9], h.stamp[8] / w, k / w, h.stamp[1] / k, h.stamp[2] / k, h.stamp[3] / k,
            h.stamp[4] / k, h.stamp[5] / k, h.stamp[6] / k, h.stamp[7] / k, h.stamp[10] / k, h.stamp[11] / k, h.stamp[12] / k);
    if (c->kernelCs && h.stamp[11])   // qa_integrate_cs reuses slots 10 / 11: items taken from the pool / rounds of the cooperative walks
      fprintf(stderr, "[stamps] cooperative walks: %llu rounds, %.1f of 64 lanes hold an item on average (lane occupancy of the walks %.3f); %.3f of the rounds are leaf rounds; 'mesh walks' above = the rounds alone\n", h.stamp[11],
              (double) h.stamp[10] / (double) h.stamp[11], (double) h.stamp[10] / (64.0 * (double) h.stamp[11]), (double) h.stamp[12] / (double) h.stamp[11]);
    if (c->kernelCs)
      fprintf(stderr, "[stamps] closest-hit sweeps without their rounds %.3f, winners' details %.3f, shadow sweeps without their rounds %.3f; lanes sent to the exact walks: %llu closest, %llu shadow (of %llu + %llu casts)\n",
              (h.stamp[13] - (double) h.stamp[3]) / k, h.stamp[14] / k, (h.stamp[17] - (double) h.stamp[6]) / k, h.stamp[15], h.stamp[16], (unsigned long long) h.casts_normal, (unsigned long long) h.casts_shadow);
  }
#endif
  return QA_OK;
}
int qa_reset_counters(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  int rc = qa_synchronize(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipMemset(c->dCounters, 0, sizeof(DCounters)));
  if (c->wf.dStats) HIP_TRY(hipMemset(c->wf.dStats, 0, sizeof(WfStats)));
  c->wf.iterations = c->wf.raysClosest = c->wf.raysShadow = c->wf.jobs = c->wf.redo = 0;
  return QA_OK;
}

int qa_get_staged_stats(qa_ctx *c, uint64_t out[QA_STAGED_STATS])
{
  if (!c || !out) return Fail(QA_EINVAL, "null argument");
  int rc = qa_synchronize(c);
  if (rc != QA_OK) return rc;
  WfStats st;
  memset(&st, 0, sizeof(st));
  if (c->wf.dStats) HIP_TRY(hipMemcpy(&st, c->wf.dStats, sizeof(st), hipMemcpyDeviceToHost));
  const uint64_t v[QA_STAGED_STATS] = {c->wf.iterations, c->wf.raysClosest, c->wf.raysShadow, c->wf.jobs, c->wf.redo, st.jobs, st.nodeSteps,
                                       st.leafSteps, st.triTests, st.redo, st.suspended, st.laneSlots, st.waveRounds};
  memcpy(out, v, sizeof(v));
  return QA_OK;
}

int qa_set_pipeline(qa_ctx *c, int mode)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (mode < QA_PIPE_MEGA || mode > QA_PIPE_AUTO) return Fail(QA_EINVAL, "pipeline mode must be QA_PIPE_MEGA, QA_PIPE_STAGED or QA_PIPE_AUTO");
  c->wf.mode = mode;
  c->wf.modeSet = true;
  if (c->haveScene) SetKernelName(c);
  return QA_OK;
}

const char *qa_get_kernel_name(qa_ctx *c)
{
  if (!c || !c->haveScene) return "";
  return c->launchedName.empty() ? c->kernelName.c_str() : c->launchedName.c_str();
}

int qa_get_kernel_time(qa_ctx *c, double *total_ms, uint64_t *launches)
{
  if (!c || !total_ms || !launches) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  int rc = DrainEvents(c);
  if (rc != QA_OK) return rc;
  *total_ms = c->totalMs;
  *launches = c->launches;
  return QA_OK;
}
int qa_reset_kernel_time(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  int rc = DrainEvents(c);
  if (rc != QA_OK) return rc;
  c->totalMs = 0;
  c->launches = 0;
  return QA_OK;
}

int qa_set_option(qa_ctx *c, const char *name, long long value)
{
  if (!c || !name) return Fail(QA_EINVAL, "null argument");
  const std::string n(name);
  if (n == "coop") {
    c->optCoop = value != 0;
    if (c->haveScene) return SelectKernel(c);
  } else if (n == "cs_cull") c->optCsCull = value != 0;
  else if (n == "cs_force_exact") c->optCsForceExact = (uint32_t) (value & 3);
  else if (n == "walk_zero_terms") c->optWalkZeroTerms = value ? 1u : 0u;
  else if (n == "chunk_spp") c->optChunkSpp = value < 0 ? -1 : (int) (value > 65535 ? 65535 : value);
  else if (n == "chunk_tail") c->optChunkTail = value < 0 ? 0 : (int) (value > 65535 ? 65535 : value);
  else if (n == "cs_pool_limit") c->optCsPool = value > 0 ? (uint32_t) std::max<long long>(64, value) : 0u;
  else if (n == "sync_samples") c->syncSamples = value < 0 ? -1 : (value > 64 ? 64 : (int) value);
  else if (n == "tile_order") c->tileOrder = value != 0;
  else if (n == "progressive_tile_limit") c->optProgTileLimit = value > 0 ? (uint32_t) std::min<long long>(value, 0x7FFFFFFF) : 0u;
  else if (n == "staged_groups") {
    c->wf.numGroups = (int) std::max<long long>(1, std::min<long long>(value, WfHost::kMaxGroups));
    if (c->haveScene) SetKernelName(c);
  } else if (n == "verbose") c->optVerbose = value != 0;
  else return Fail(QA_EINVAL, "unknown option '" + n + "'");
  return QA_OK;
}

int qa_debug_scrub_scratch(qa_ctx *c, uint32_t pattern)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  // eight waves per SIMD on every CU: every wave slot of the chip - and with it every private segment the next launch can get -
  // holds a wave of this kernel at the same time (each lingers until the grid has been placed)
  hipLaunchKernelGGL(qa::qa_scrub_scratch, dim3((unsigned) c->numCUs * 8), dim3(256), 0, c->stream, pattern, reinterpret_cast<uint32_t *>(c->dCounters));
  HIP_TRY(hipGetLastError());
  for (int g = 0; g < c->wf.numGroups; ++g)
    if (c->wf.groups[g].stream) {
      hipLaunchKernelGGL(qa::qa_scrub_scratch, dim3((unsigned) c->numCUs * 8), dim3(256), 0, c->wf.groups[g].stream, pattern, reinterpret_cast<uint32_t *>(c->dCounters));
      HIP_TRY(hipGetLastError());
    }
  if (c->wf.redoStream) {
    hipLaunchKernelGGL(qa::qa_scrub_scratch, dim3((unsigned) c->numCUs * 8), dim3(256), 0, c->wf.redoStream, pattern, reinterpret_cast<uint32_t *>(c->dCounters));
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipDeviceSynchronize());
  return QA_OK;
}

// ---- progressive frames ---------------------------------------------------------------------------------------------------------
int qa_progressive_begin(qa_ctx *c, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce, uint32_t seed, uint32_t flags)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  int rc = CheckFrame(c, x0, y0, x1, y1, spp_min, spp_max, max_bounce);
  if (rc != QA_OK) return rc;
  if (flags & ~QA_RENDER_STATS) return Fail(QA_EINVAL, "unknown flags");
  const unsigned tiles = (unsigned) ((x1 - x0 + 7) / 8) * (unsigned) ((y1 - y0 + 7) / 8);
  // a pass's work counter runs from tiles * 64 to 2 * tiles * 64 (plus 64 per exiting wave) in 32 bits
  if ((unsigned long long) tiles * 64ull * 2ull >= 0xF0000000ull) return Fail(QA_EINVAL, "region too large for a progressive frame");
  EndProgressive(c, nullptr);
  qa_ctx::Progressive &f = c->prog;
  f.ended.clear();
  const size_t npix = (size_t) (x1 - x0) * (size_t) (y1 - y0);
  hipError_t e = hipSuccess;
  if ((e = hipMalloc((void **) &f.dState, npix * 8 * sizeof(uint32_t))) != hipSuccess || (e = hipMalloc((void **) &f.dLevel, tiles * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc((void **) &f.dProgress, tiles * sizeof(uint32_t))) != hipSuccess || (e = hipMalloc((void **) &f.dRgb, npix * 3 * sizeof(float))) != hipSuccess ||
      (e = hipMalloc((void **) &f.dDepth, npix * sizeof(float))) != hipSuccess || (e = hipMalloc((void **) &f.dNs, npix * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc((void **) &f.dStatus, 3 * sizeof(unsigned long long))) != hipSuccess || (e = hipMalloc((void **) &f.dList, tiles * sizeof(uint32_t))) != hipSuccess) {
    EndProgressive(c, nullptr);
    return Fail(e == hipErrorOutOfMemory ? QA_ENOMEM : QA_EHIP, std::string("progressive frame slabs: ") + hipGetErrorString(e));
  }
  if (!f.done) HIP_TRY(hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
  hipLaunchKernelGGL(qa::qa_prog_init, dim3((unsigned) ((npix + 255) / 256)), dim3(256), 0, c->stream, f.dState, f.dRgb, f.dDepth, f.dNs, x0, y0,
                     (uint32_t) (x1 - x0), (uint32_t) npix, (uint32_t) c->ds.cam.width, seed);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(f.dLevel, 0, tiles * sizeof(uint32_t), c->stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) f.dProgress, 1, tiles, c->stream));
  HIP_TRY(hipEventRecord(f.done, c->stream));
  f.x0 = x0; f.y0 = y0; f.x1 = x1; f.y1 = y1;
  f.sppMin = spp_min; f.sppMax = spp_max; f.maxBounce = max_bounce;
  f.seed = seed; f.flags = flags;
  f.tiles = tiles;
  f.npix = npix;
  f.target = f.top = 0;
  f.active = true;
  f.stale = false;
  return QA_OK;
}

int qa_progressive_restart(qa_ctx *c)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  if ((rc = CheckFrame(c, f.x0, f.y0, f.x1, f.y1, f.sppMin, f.sppMax, f.maxBounce)) != QA_OK) return rc;   // (the edited scene may refuse the frame: area lights, bounce > 7)
  HIP_TRY(hipStreamWaitEvent(c->stream, f.done, 0));   // the last pass, on whatever stream it ran
  hipLaunchKernelGGL(qa::qa_prog_init, dim3((unsigned) ((f.npix + 255) / 256)), dim3(256), 0, c->stream, f.dState, f.dRgb, f.dDepth, f.dNs, f.x0, f.y0,
                     (uint32_t) (f.x1 - f.x0), (uint32_t) f.npix, (uint32_t) c->ds.cam.width, f.seed);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(f.dLevel, 0, f.tiles * sizeof(uint32_t), c->stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) f.dProgress, 1, f.tiles, c->stream));
  HIP_TRY(hipEventRecord(f.done, c->stream));
  f.target = f.top = 0;
  f.stale = false;
  return QA_OK;
}

// the frame's status on the context's stream (synchronises)
static int ProgStatus(qa_ctx *c, int *reached, uint64_t *finished, uint64_t *behind)
{
  qa_ctx::Progressive &f = c->prog;
  HIP_TRY(hipStreamWaitEvent(c->stream, f.done, 0));
  HIP_TRY(hipMemsetAsync(f.dStatus, 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(hipMemsetAsync(f.dStatus + 2, 0xFF, sizeof(unsigned long long), c->stream));
  const size_t n = std::max(f.npix, (size_t) f.tiles);
  hipLaunchKernelGGL(qa::qa_prog_status, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, c->stream, f.dState, (uint32_t) f.npix, f.dLevel, f.tiles,
                     (uint32_t) f.target, f.dStatus);
  HIP_TRY(hipGetLastError());
  unsigned long long h[3];
  HIP_TRY(hipMemcpyAsync(h, f.dStatus, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (reached) *reached = (int) h[2];
  if (finished) *finished = h[0];
  if (behind) *behind = h[1];
  return QA_OK;
}

int qa_progressive_advance(qa_ctx *c, int spp_target, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (spp_target < 1) return Fail(QA_EINVAL, "bad spp target");
  qa_ctx::Progressive &f = c->prog;
  if (f.stale) return Fail(QA_EINVAL, "the scene was edited since this progressive frame began: qa_progressive_restart or qa_progressive_begin first");
  const int target = std::min(spp_target, f.sppMax);
  // Every unfinished pixel of a tile has exactly the tile's level in samples (a tile in hand always completes its pass).  Above every
  // earlier target, no pixel has the target yet; at or below the highest, some tiles may have it (a stop left others behind): the
  // pass then hands out the tiles below the target alone - or nothing happens when there are none (this asks the device)
  const bool reissue = target <= f.top;
  if (reissue) {
    int reached = 0;
    if ((rc = ProgStatus(c, &reached, nullptr, nullptr)) != QA_OK) return rc;
    if (reached >= target) return QA_OK;
  }
  hipStream_t s = hip_stream ? (hipStream_t) hip_stream : c->stream;
  rc = EnsureHalton(c, f.sppMax);   // (a one-shot frame in between may have reallocated the table)
  if (rc != QA_OK) return rc;
  c->ds.halton = c->dHalton;
  c->ds.halton_count = c->haltonCount;
  HIP_TRY(hipStreamWaitEvent(s, f.done, 0));   // the frame's setup / last pass, on whatever stream it ran
  unsigned int *work = c->dWork + c->workNext;
  c->workNext = (c->workNext + 1) % qa_ctx::kCounterRing;
  Launch L;
  rc = LaunchSetup(c, L, f.x0, f.y0, f.x1, f.y1, 0, 1, (f.y1 - f.y0 + 7) / 8, f.sppMin, f.sppMax, f.maxBounce, f.seed, f.flags, f.dRgb, f.dDepth,
                   f.dNs, work, s, true);
  if (rc != QA_OK) return rc;
  // every work item is "chunk 1" of its tile: the counter starts past chunk 0 (qa_integrate, section A), so every pixel resumes from its
  // state and ends its chunk on chunk_spp + 1 * chunk_tail = target samples.  progressive_tile_limit (tests): only the last n items are
  // left, as if stopped
  const uint32_t limit = c->optProgTileLimit;
  if (reissue) {
    hipLaunchKernelGGL(qa::qa_prog_select, dim3(1), dim3(64), 0, s, L.rp.tile_order, f.dLevel, f.tiles, (uint32_t) target, limit, f.dList, work);
    HIP_TRY(hipGetLastError());
    L.rp.tile_order = f.dList;
  } else {
    const unsigned take = (limit && limit < f.tiles) ? limit : f.tiles;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) work, (int) ((2u * f.tiles - take) * 64u), 1, s));
  }
  L.rp.chunk_spp = (uint32_t) target; L.rp.chunk_tail = 0; L.rp.num_chunks = 2;
  L.rp.tile_progress = f.dProgress; L.rp.pix_state = f.dState;
  if ((rc = LaunchFrame(c, L, f.flags, false, s)) != QA_OK) return rc;
  hipLaunchKernelGGL(qa::qa_prog_levels, dim3((f.tiles + 255) / 256), dim3(256), 0, s, f.dProgress, L.rp.tile_order, f.dLevel, f.tiles, (uint32_t) target);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(f.done, s));
  f.target = target;
  f.top = std::max(f.top, target);
  return QA_OK;
}

int qa_progressive_read_device(qa_ctx *c, float *d_rgb, float *d_depth, uint32_t *d_ns, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!d_rgb || !d_depth || !d_ns) return Fail(QA_EINVAL, "null output buffer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t) hip_stream : c->stream;
  const qa_ctx::Progressive &f = c->prog;
  HIP_TRY(hipStreamWaitEvent(s, f.done, 0));
  hipLaunchKernelGGL(qa::qa_prog_resolve, dim3((unsigned) ((f.npix + 255) / 256)), dim3(256), 0, s, f.dState, f.dRgb, f.dDepth, f.dNs, (uint32_t) f.npix,
                     d_rgb, d_depth, d_ns);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

int qa_progressive_read(qa_ctx *c, float *rgb, float *depth, uint32_t *ns)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  if (!rgb || !depth || !ns) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  qa_ctx::Progressive &f = c->prog;
  if (!f.dPrevRgb) {
    HIP_TRY(hipMalloc((void **) &f.dPrevRgb, f.npix * 3 * sizeof(float)));
    HIP_TRY(hipMalloc((void **) &f.dPrevDepth, f.npix * sizeof(float)));
    HIP_TRY(hipMalloc((void **) &f.dPrevNs, f.npix * sizeof(uint32_t)));
  }
  if ((rc = qa_progressive_read_device(c, f.dPrevRgb, f.dPrevDepth, f.dPrevNs, nullptr)) != QA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, f.dPrevRgb, f.npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(depth, f.dPrevDepth, f.npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(ns, f.dPrevNs, f.npix * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QA_OK;
}

int qa_progressive_status(qa_ctx *c, int *spp_reached, uint64_t *pixels_finished, uint64_t *tiles_behind)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return ProgStatus(c, spp_reached, pixels_finished, tiles_behind);
}

int qa_progressive_end(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  EndProgressive(c, nullptr);
  c->prog.ended.clear();
  return QA_OK;
}

int qa_set_launch_config(qa_ctx *c, int blocks_per_cu, int threads_per_block)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (threads_per_block != 0 && threads_per_block != QA_BLOCK) return Fail(QA_EINVAL, "this build supports 256-thread workgroups only");
  if (blocks_per_cu < 0 || blocks_per_cu > 8) return Fail(QA_EINVAL, "blocks_per_cu must be in 0..8");
  c->blocksPerCU = blocks_per_cu;
  return QA_OK;
}

}  // extern "C"
