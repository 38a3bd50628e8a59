// qa_ctx.h — internals shared by the translation units of libqaray_hip.so (the README's layout line says which unit holds what).
// Only qa_mega.hip, qa_coop.hip, qa_photon.hip, qa_wf.hip, qa_gbuffer.hip, qa_matte.hip and qa_idmatte.hip include the kernel headers.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qa_scene_build.h"
#include "qa_wf_types.h"
#include "qaray_hip.h"

using namespace qa;

typedef void (*KernelFn)(const DScene, const RenderParams);
// What crosses from qa_mega.hip and qa_coop.hip: the pickers, and three sizes of the kernel headers the host needs
KernelFn PickKernel(bool resident, bool lights, bool tex, bool area, bool stats);
KernelFn PickLastCastKernel();   // qa_lastcast.hip: resident scenes without lights whose plan has lastCastQuery
// qa_lastcast.hip: one byte per tile of the launch rp describes - would qa_integrate_lastcast finish it in closed form (qa_emptytile.h)?
int LaunchEmptyTileMask(const DScene &ds, const RenderParams &rp, unsigned tiles, uint8_t *d_mask, hipStream_t s);
KernelFn PickCs(bool lights, bool tex, bool cull, bool many, bool area);
KernelFn PickCsResume(bool lights, bool cull, bool many, bool area);   // (untextured rows only)
extern const int kMaxPath;             // QA_MAX_PATH: hits per path an AREA variant can log
extern const size_t kAreaLogFloats;    // ... x QA_REC_FLOATS: the floats of a thread's log
size_t CsLdsBytes(uint32_t items, uint32_t slots);   // CsLdsWords: dynamic LDS of a workgroup of the cooperative kernels

inline thread_local std::string g_err;
inline int Fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return Fail(QA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Developer knobs.  The PRODUCT library reads no environment variable of its own: what an embedding application or a test
// may change goes through qa_set_option (include/qaray_hip.h).  Builds made with -DQA_DEV_KNOBS (make hip EXTRA=-DQA_DEV_KNOBS,
// the A/B scripts under tools/) additionally read the QA_* variables named at the call sites.
inline const char *DevEnv(const char *name)
{
#ifdef QA_DEV_KNOBS
  return getenv(name);
#else
  (void) name;
  return nullptr;
#endif
}

struct EventPair { hipEvent_t a, b; };

// One integrator a frame can launch.  The STATS slots carry their plain sibling's LDS size and workgroups per CU.  stackDepth is
// the scene's at SelectKernel (the photon maps' own for kPm): whatever changes DScene::stackDepth runs SelectKernel again
struct Integrator { KernelFn fn = nullptr; size_t ldsBytes = 0; int blocksPerCU = 2; uint32_t stackDepth = 0; };
enum Slot { kMega, kMegaStats, kCs, kCsResume, kPm, kPmStats, kNumSlots };
inline Slot PickSlot(bool photon, bool stats, bool coop, bool resume)
{
  return photon ? (stats ? kPmStats : kPm) : stats ? kMegaStats : coop ? (resume ? kCsResume : kCs) : kMega;
}
// Workgroups per CU that are resident at once, at most 8; `fallback` when the runtime cannot say
inline int OccupancyBlocks(KernelFn fn, size_t ldsBytes, int fallback = 2)
{
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *) fn, QA_BLOCK, ldsBytes) != hipSuccess || n < 1) n = fallback;
  return n > 8 ? 8 : n;
}

// "The last X ended here": work on another stream that shares X's memory waits for it.  The event is made on first use.  The name is
// the member's (DESIGN.md "Streams: who waits for whom"); QA_SKIP_WAIT=<name> (developer builds only) makes that fence's waits
// no-ops, which is how tests/test_gpu_stream_order.py was shown to fail when a wait is lost (profiles/stream_order.txt)
struct StreamFence {
  const char *name = "";
  hipEvent_t ev = nullptr;
  bool set = false;
  hipStream_t stream = nullptr;
  bool Skipped() const { const char *e = DevEnv("QA_SKIP_WAIT"); return e && !strcmp(e, name); }
  hipError_t WaitOn(hipStream_t s) const { return (set && s != stream && !Skipped()) ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
  hipError_t Record(hipStream_t s)
  {
    hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess && (e = hipEventRecord(ev, s)) == hipSuccess) { set = true; stream = s; }
    return e;
  }
};

// A device buffer that only grows.  Before the old one is freed, the whole device or the given stream is waited for, if asked
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipError_t Reserve(size_t bytes, bool syncDevice = false, hipStream_t syncStream = nullptr)
  {
    if (bytes <= cap) return hipSuccess;
    hipError_t e = !p ? hipSuccess : syncDevice ? hipDeviceSynchronize() : syncStream ? hipStreamSynchronize(syncStream) : hipSuccess;
    if (e != hipSuccess) return e;
    Free();
    if ((e = hipMalloc(&p, bytes)) == hipSuccess) cap = bytes;
    return e;
  }
  void Free() { if (p) (void) hipFree(p); p = nullptr; cap = 0; }
};

// One frame as its caller describes it (qa_render_*, qa_progressive_begin)
struct FrameArgs {
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  int tileRow0 = 0, tileRowStep = 1;   // strip partition: this call's tile rows are tileRow0, + tileRowStep, ...
  int sppMin = 1, sppMax = 1, maxBounce = 0;
  uint32_t seed = 0, flags = 0;
  float *rgb = nullptr, *depth = nullptr;   // outputs (device)
  uint32_t *ns = nullptr;
  hipStream_t stream = nullptr;
};

// Host side of the staged integrator (qa_wf.hip): buffers are kept between frames
struct WfHost {
  bool eligible = false;        // the uploaded scene can run staged (SelectStaged)
  bool modeSet = false;         // qa_set_pipeline was called
  int mode = 2;                 // qa_set_pipeline: 0 mega, 1 staged, 2 auto (= the megakernel: the staged integrator runs on request only)
  int numLights = 0;            // non-ambient lights
  int32_t lightIdx[QA_WF_MAX_LIGHTS] = {0, 0, 0, 0};
  // The frame's 8x8 tiles are dealt round-robin to a few GROUPS; each group has its own slot state, queues and counters
  // and drives its own logic -> cull -> trace -> redo chain on its own stream, so that the (latency-bound, tail-heavy)
  // kernels of different groups overlap on the chip.
  struct Group {
    WfBuf buf{};
    size_t capSlots = 0;
    int capLights = -1;
    std::vector<void *> allocs;
    WfCounters *dCtr = nullptr, *hCtr = nullptr;   // one per iteration of a chunk (device / pinned host)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t logicDone = nullptr, redoDone = nullptr;   // wf_redo runs on WfHost::redoStream beside the pass's cull and trace stages
    bool finished = false;
  };
  static const int kMaxGroups = 8;
  Group groups[kMaxGroups];
  int numGroups = 1;            // qa_set_option("staged_groups"): several groups only pay when the process has a hardware queue per group stream (GPU_MAX_HW_QUEUES >= 8)
  hipEvent_t start = nullptr;
  hipStream_t redoStream = nullptr;   // shared by the groups
  bool redoAsync = true;              // QA_WF_REDO_ASYNC=0: wf_redo in the group's own chain
  WfStats *dStats = nullptr;
  // diagnostics of the frames rendered since the last reset
  uint64_t iterations = 0, raysClosest = 0, raysShadow = 0, jobs = 0, redo = 0;
  int traceBlocksPerCU = 0;     // QA_WF_BLOCKS: workgroups per CU of every stage kernel of one group (0 = 2 with several groups, what fits with one)
  uint32_t gate = 1;            // new samples start every gate-th pass (QA_WF_GATE).  2 was worth +50 % with the first trace stage; since the
                                // 4-wide tree over triangles and the scalar / global table reads it is equal on long frames and 4 - 10 % behind on short ones
  uint32_t stackCap = 24;       // LDS stack entries per lane of wf_trace (QA_WF_STACK)
  uint32_t budget = 512;        // BVH steps a job may take per pass (QA_WF_BUDGET)
};

struct qa_ctx {
  int device = 0;
  int numCUs = 0;
  hipStream_t stream = nullptr;
  // scene
  std::vector<unsigned char> hostBlob;
  unsigned char *dBlob = nullptr;
  std::vector<void *> sceneAllocs;  // derived arrays
  DScene ds{};
  ScenePlan plan;                   // what the upload decided (qa_scene_build.h)
  bool haveScene = false;
  // scene edits (qa_scene_edit_*): the host tables of the upload without their mesh side (DropMeshSide), the knobs they were
  // built with, the per-thread slabs a plan may need (made by the upload or by the first edit whose plan asks for one), and
  // pinned staging the edits' copies leave from: a bump arena, waited for only when it wraps
  SceneTables tables;
  BuildKnobs knobs;
  float *dAreaSlab = nullptr, *dSurfSlab = nullptr;
  unsigned char *hEditStage = nullptr;
  size_t editStageBytes = 0, editStageUsed = 0;
  StreamFence lastEdit{"lastEdit"};             // end of the last edit's copies (on the context's stream)
  StreamFence texSource{"texSource"};            // qa_scene_edit_texels_device: the caller's stream when its source was handed over
  std::vector<uint32_t> texOnDevice;   // file textures whose texels were edited from device memory: the host blob's bytes of
                                    // these are behind the device blob's until FetchDeviceTexels (qa_scene_download)
  uint64_t statMeshBuilds = 0, statSceneAllocs = 0, statBytesCopied = 0, statEdits = 0;   // qa_get_scene_stats
  float *dHalton = nullptr;
  int haltonCount = 0;
  // launch plumbing
  static const int kCounterRing = 64;
  unsigned int *dWork = nullptr;  // ring of work counters
  // tiles in sample chunks (qa_integrate, RenderParams::chunk_spp): per-pixel state between chunks, per-tile progress
  DevBuf pixState, tileProgress;
  StreamFence lastFrame{"lastFrame"};          // the slabs (these, the area-light log, the many-light surface slab) are one per context: a frame on another stream waits
  int optChunkSpp = -1;           // "chunk_spp": -1 per frame (few tiles per wave), 0 off, n samples of a tile's first chunk
  int optChunkTail = 0;           // "chunk_tail": samples of every further chunk (0: an eighth of the frame's spp)
  int optTileLists = -1;          // "tile_lists": -1 on with the measured limit (QA_TILE_LISTS_AUTO), 0 off, n on with a limit of n leaves per mesh and tile
  int workNext = 0;
  int *hStop = nullptr;           // mapped host memory, read by the kernel's wave leaders
  int *dStopAlias = nullptr;
  DCounters *dCounters = nullptr;
  // host-variant staging
  DevBuf stageRgb, stageDepth, stageNs;
  DevBuf stageQuery;              // the host forms of every query: one buffer, carved by QueryStage (qa_stage.h) and by nothing else, sized for the
                                  // largest call so far - each of them ends with hipStreamSynchronize(stream), so no two use it at once
  // timing
  std::vector<EventPair> pending, freeEvents;
  double totalMs = 0;
  uint64_t launches = 0;
  // the integrators of the uploaded scene (SelectKernel; kPm / kPmStats: qa_photon_maps_build).  kCs: the megakernel with cooperative
  // mesh walks (qa_kernel_cs.h), fn null where the scene or "coop" rules it out, ldsBytes set by the upload; kCsResume: its
  // chunk-capable instance where kCs carries no chunk code (progressive passes)
  Integrator integ[kNumSlots];
  int optBlocksPerCU = 0;       // qa_set_launch_config: workgroups per CU of every slot (0 = the slot's own)
  bool tileOrder = true;        // centre-first tile order (QA_NO_TILE_ORDER=1 turns it off)
  uint32_t *dOrder = nullptr;   // tile launch order of the last region shape
  uint64_t orderKey = 0;
  int syncSamples = -1;  // -1: decide per scene (SelectKernel), 0/1 forced by QA_SYNC
  // photon / caustics maps (qa_photon.hip); valid until the next scene upload or qa_photon_maps_clear
  bool photonReady = false;
  void *dPhotons[2] = {nullptr, nullptr};      // qa_photon records (what qa_photon_maps_download returns)
  void *dPmTables[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};   // DPhotonMap node / dir / power
  void *dHeap = nullptr;
  qa_photon_params photonParams{};
  uint64_t photonEmitted[2] = {0, 0}, photonEmissions[2] = {0, 0};
  std::vector<qa_photon> hostPhotons[2];   // balanced, [0] unused
  WfHost wf;
  std::string kernelName;       // the integrator the next frame is planned to run on (SetKernelName)
  std::string launchedName;     // what the last qa_render_* call really launched (empty before the first)
  // qa_set_option
  bool optCoop = true;          // "coop": cooperative mesh walks (qa_kernel_cs.h) where the scene allows them
  bool optCsCull = true;        // "cs_cull": instance culling in the cooperative kernel's sweeps (0: every instance is visited; A/B tests)
  int optLastCast = -1;           // "last_cast": -1 / 1 the bounce rays of qa_integrate_lastcast ask which emitter they meet, 0 they run the closest-hit sweep (same kernel, same frame)
  int optLeafSweep = -1;          // "leaf_sweep": -1 / 1 those queries sweep a mesh's leaf table where it has one (DScene::lastCast = 2; qa_kernel.h sweepLeaves), 0 they walk its own tree (same frame)
  int optEmptyTiles = -1;         // "empty_tiles": -1 / 1 one-shot frames of qa_integrate_lastcast finish the tiles no camera ray can hit anything from in closed form (qa_emptytile.h), 0 they trace them (same frame)
  uint32_t optWalkZeroTerms = 0; // "walk_zero_terms": tests - also walk the shadow rays of lights whose term is zero whatever they find
  uint32_t optCsForceExact = 0; // "cs_force_exact": tests of the exact walks (bit 0 closest-hit, bit 1 shadow queries)
  uint32_t optCsPool = 0;       // "cs_pool_limit": upper bound for the walks' pool capacity (tests force the overflow path)
  bool optVerbose = false;      // "verbose": tree / launch-shape report on stderr at upload
  uint32_t optProgTileLimit = 0; // "progressive_tile_limit": tests - a progressive pass takes at most n tiles, then ends as if stopped
  // the progressive frame (qa_progressive_*): its slabs are its own, apart from the one-shot frames' pixState / tileProgress
  struct Progressive {
    bool active = false;
    bool stale = false;           // the scene was edited since the frame's pixels were made: qa_progressive_restart before the next pass
    std::string ended;           // why the last frame ended early (a scene upload, the photon maps built or cleared): qa_last_error
    FrameArgs args;               // as qa_progressive_begin got them; rgb / depth / ns: the frame's slabs of finished pixels' outputs, depth of sample 0
    unsigned tiles = 0;
    size_t npix = 0;
    int target = 0;               // the last pass's target, min(S, spp_max)
    int top = 0;                  // the highest target so far: no tile's level is above it
    uint32_t *dState = nullptr;   // 8 words per pixel (output index): RNG state, samples taken | bit 31 finished, running mean, variance
    uint32_t *dLevel = nullptr;   // per tile: the samples every unfinished pixel of it has
    uint32_t *dList = nullptr;    // per tile: the tile order of a pass that re-issues a target (qa_prog_select)
    uint32_t *dProgress = nullptr;   // per tile: the pass's tile_progress (1 before a pass, 2 once the tile's pass is complete)
    DevBuf prevRgb, prevDepth, prevNs;   // qa_progressive_read's preview (made on first use)
    unsigned long long *dStatus = nullptr;   // qa_progressive_status: finished pixels, tiles behind, lowest level
    StreamFence done{"prog.done"};             // end of the frame's setup / last pass, on whatever stream it ran
    // tile-selective and noisiest-first passes (made on first use, freed with the frame): the error map, the pass's mask, the host
    // variant's pinned mask and the end of its last copy, qa_progressive_adaptive_info's four words
    float *dError = nullptr;
    uint8_t *dMask = nullptr, *hMask = nullptr;
    uint32_t *dKeys = nullptr;    // the adaptive selection's key per tile
    hipEvent_t maskCopied = nullptr;
    unsigned long long *dInfo = nullptr;
  } prog;
  // the 8-bit products (qa_display.hip): the statistics block (4 working words, then their initial values) and the staging of
  // qa_progressive_display's host variant are made on first use and live as long as the context
  uint32_t *dDisplay = nullptr;
  StreamFence lastDisplay{"lastDisplay"};      // the block is one per context: a display on another stream waits
  DevBuf displayStage;
  // the denoiser's working planes (qa_denoise.hip): 40 bytes per pixel of the largest frame filtered so far, made on first use
  DevBuf denoisePlanes;
  StreamFence lastDenoise{"lastDenoise"};      // the planes are one per context: a filter on another stream waits
  // qa_progressive_reproject_device's ids plane of the current frame (qa_reproject.hip): 8 bytes per pixel of the largest frame so far
  DevBuf reprojectIds;
  StreamFence lastReproject{"lastReproject"};    // one per context: a call on another stream waits
  // qa_probe_sh*'s rays of one chunk of probes (qa_lightprobe.hip): 44 bytes per ray of the largest chunk so far.  One per context:
  // the call that writes it waits for lastFrame and records it behind its last reduction
  DevBuf probeScratch;
};

void FreePhotonMaps(qa_ctx *c);  // qa_photon.hip
// qa_frame.hip: the integrators of the uploaded scene and the name qa_get_kernel_name gives before a frame has run; what all frames
// share of a launch.  Launch: one launch of the megakernel as LaunchSetup plans it (without the chunk fields of rp)
int SelectKernel(qa_ctx *c);
void SetKernelName(qa_ctx *c);
struct Launch { RenderParams rp; DScene ds; Slot slot = kMega; long long blocks = 1; unsigned tiles = 0; };
int EnsureHalton(qa_ctx *c, int count);
int CheckFrame(qa_ctx *c, const FrameArgs &a);
int LaunchSetup(qa_ctx *c, Launch &L, const FrameArgs &a, int ownRows, unsigned int *work, bool resume);
int LaunchFrame(qa_ctx *c, Launch &L, bool staged, hipStream_t s);
int DrainEvents(qa_ctx *c);
// Scene::usePhotonMap for one launch: the tables of both maps and the heap slab, as qa_photon_maps_build left them (c->photonReady),
// for the frames' PHOTON variants (LaunchSetup) and the gathering batch kernels (qa_raybatch.h)
inline void SetPhotonParams(const qa_ctx *c, RenderParams &rp)
{
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
// qa_capi.hip, for the edits that live elsewhere (qa_texture_edit.hip): bytes of the pinned edit ring; the waits an edit's device
// work begins with (and statBytesCopied = 0); what every edit ends with
int EditStageReserve(qa_ctx *c, size_t need, unsigned char **at);
int EditBegin(qa_ctx *c);
int EditEnd(qa_ctx *c, bool keepsPhotonMaps);
// qa_texture_edit.hip: brings the host blob's texels up to the device blob's (synchronises when there is something to fetch)
int FetchDeviceTexels(qa_ctx *c);
// qa_wf.hip
void FreeStaged(qa_ctx *c);
void SelectStaged(qa_ctx *c);
bool StagedTakes(const qa_ctx *c, uint32_t flags, int spp_max, int max_bounce, size_t slots);
int RenderStaged(qa_ctx *c, const DScene &ds, const RenderParams &rp, hipStream_t s, DCounters *frameCounters);

// Ends the progressive frame, if any, and frees its slabs; a later qa_progressive_advance / read returns QA_EINVAL with `why`
inline void EndProgressive(qa_ctx *c, const char *why)
{
  qa_ctx::Progressive &f = c->prog;
  if (f.active && why) f.ended = why;
  f.active = false;
  void *slabs[] = {f.dState, f.dLevel, f.dList, f.dProgress, f.args.rgb, f.args.depth, f.args.ns, f.dStatus, f.dError, f.dMask, f.dKeys, f.dInfo};
  if (f.dState) (void) hipDeviceSynchronize();   // (a pass may still run on a stream of the caller's)
  for (void *p : slabs)
    if (p) (void) hipFree(p);
  if (f.hMask) (void) hipHostFree(f.hMask);
  if (f.maskCopied) (void) hipEventDestroy(f.maskCopied);
  f.dError = nullptr; f.dMask = f.hMask = nullptr; f.dKeys = nullptr; f.dInfo = nullptr; f.maskCopied = nullptr;
  f.dState = f.dLevel = f.dList = f.dProgress = f.args.ns = nullptr;
  f.args.rgb = f.args.depth = nullptr;
  f.dStatus = nullptr;
  f.prevRgb.Free(); f.prevDepth.Free(); f.prevNs.Free();
}

// What most entries begin with, and the stream they work on: the caller's or the context's
inline int Enter(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  return QA_OK;
}
inline hipStream_t StreamOf(qa_ctx *c, void *hip_stream) { return hip_stream ? (hipStream_t) hip_stream : c->stream; }
// where the upload report goes ("verbose", QA_FAST_VERBOSE), else null
inline FILE *Report(const qa_ctx *c) { return (c->optVerbose || DevEnv("QA_FAST_VERBOSE")) ? stderr : nullptr; }

// A region checked as a frame's is (CheckFrame), for the calls that take nothing else of a frame
inline int CheckRegion(qa_ctx *c, int x0, int y0, int x1, int y1)
{
  FrameArgs a;
  a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
  return CheckFrame(c, a);
}

// Enqueues a kernel that only reads the scene (guide planes, matte planes, ray queries): fn(DScene, Params).  Ordered as a frame
// is: behind the context's last frame and last edit, and the next edit waits for it (it reads the tables an edit rewrites).  The
// kernel's dynamic LDS is laid out as a prefix of the megakernel's, so it gets that kernel's LDS size and stack depth; the grid
// is persistent (what is resident at once, a workgroup of a resident scene first copies the scene image), at most needBlocks
template <class Fn, class Params>
inline int LaunchSceneKernel(qa_ctx *c, Fn fn, const Params &p, long long needBlocks, hipStream_t s)
{
  HIP_TRY(c->lastFrame.WaitOn(s));
  HIP_TRY(c->lastEdit.WaitOn(s));
  const Integrator &mega = c->integ[kMega];
  DScene ds = c->ds;
  ds.stackDepth = mega.stackDepth;
  const long long blocks = std::max<long long>(1, std::min<long long>(needBlocks, (long long) c->numCUs * OccupancyBlocks((KernelFn) fn, mega.ldsBytes)));
  hipLaunchKernelGGL(fn, dim3((unsigned) blocks), dim3(QA_BLOCK), (unsigned) mega.ldsBytes, s, ds, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(c->lastFrame.Record(s));
  return QA_OK;
}
// the workgroups a region's 8x8 tiles need, one wave per tile
inline long long TileBlocks(int x0, int y0, int x1, int y1)
{
  const long long tiles = (long long) ((x1 - x0 + 7) / 8) * ((y1 - y0 + 7) / 8);
  return (tiles + QA_BLOCK / 64 - 1) / (QA_BLOCK / 64);
}

// What every qa_progressive_* call on a frame says when there is none (or why the last one ended)
inline int ProgActive(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (!c->prog.active) return Fail(QA_EINVAL, c->prog.ended.empty() ? "no progressive frame: qa_progressive_begin first" : c->prog.ended);
  return QA_OK;
}

inline void FreeScene(qa_ctx *c)
{
  EndProgressive(c, "the progressive frame ended: a new scene was uploaded");
  FreePhotonMaps(c);
  for (void *p : c->sceneAllocs) (void) hipFree(p);
  c->sceneAllocs.clear();
  if (c->dBlob) (void) hipFree(c->dBlob);
  c->dBlob = nullptr;
  c->dAreaSlab = c->dSurfSlab = nullptr;   // (they were among sceneAllocs)
  c->tables = SceneTables{};
  c->texOnDevice.clear();
  c->haveScene = false;
}

template <class T, class P>
inline int DeviceCopy(qa_ctx *c, const std::vector<T> &v, const P **out)
{
  *out = nullptr;
  if (v.empty()) return QA_OK;
  void *p = nullptr;
  HIP_TRY(hipMalloc(&p, v.size() * sizeof(T)));
  c->sceneAllocs.push_back(p);
  c->statSceneAllocs++;
  HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  c->statBytesCopied += v.size() * sizeof(T);
  *out = static_cast<const P *>(p);
  return QA_OK;
}

