// qa_capi.hip — the context of libqaray_hip.so's C ABI (include/qaray_hip.h): create / destroy, scene upload (blob -> device
// tables), download and edits, options, counters and timing.  Frames: qa_frame.hip, qa_progressive.hip; texel edits and their
// kernel: qa_texture_edit.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <new>

#include "qa_ctx.h"

// The per-thread slab c->plan needs, if any, made on first need and kept with the scene; c->ds points at the one the plan uses
static int EnsurePlanSlab(qa_ctx *c)
{
  const size_t threads = (size_t) c->numCUs * 8 * QA_BLOCK;
  const bool area = c->plan.area, many = !area && c->plan.shadowLights.size() > QA_CS_LIGHT_BATCH;
  float **slab = area ? &c->dAreaSlab : many ? &c->dSurfSlab : nullptr;
  if (slab && !*slab) {
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, threads * (area ? kAreaLogFloats : 13) * sizeof(float)));
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
  c->integ[kCs].ldsBytes = CsLdsBytes(ds.csItems, ds.csSlots);
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

extern "C" {

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
  (void) hipDeviceSynchronize();   // the context's stream, and whatever runs on the callers' streams on this context's memory
  FreeScene(c);
  FreeStaged(c);
  for (EventPair &ev : c->pending) { (void) hipEventDestroy(ev.a); (void) hipEventDestroy(ev.b); }
  for (EventPair &ev : c->freeEvents) { (void) hipEventDestroy(ev.a); (void) hipEventDestroy(ev.b); }
  for (void *p : {(void *) c->dHalton, (void *) c->dOrder, (void *) c->dWork, (void *) c->dCounters, (void *) c->dDisplay})
    if (p) (void) hipFree(p);
  for (void *p : {(void *) c->hEditStage, (void *) c->hStop})
    if (p) (void) hipHostFree(p);
  for (DevBuf *b : {&c->pixState, &c->tileProgress, &c->stageRgb, &c->stageDepth, &c->stageNs, &c->stageQuery, &c->displayStage, &c->denoisePlanes, &c->reprojectIds, &c->probeScratch}) b->Free();
  for (StreamFence *f : {&c->lastFrame, &c->lastEdit, &c->lastDisplay, &c->lastDenoise, &c->lastReproject, &c->texSource, &c->prog.done})
    if (f->ev) (void) hipEventDestroy(f->ev);
  if (c->stream) (void) hipStreamDestroy(c->stream);
  delete c;
  return QA_OK;
}

// Both uploads: `blob` (on the host, or on the device) to the context's host copy and its device copy, then the tables
static int Upload(qa_ctx *c, const void *blob, uint64_t nbytes, bool onDevice)
{
  if (!c || !blob || nbytes == 0) return Fail(QA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());   // frames and passes of the old scene, on the context's stream and on the callers'
  FreeScene(c);
  try { c->hostBlob.resize(nbytes); } catch (const std::bad_alloc &) { return Fail(QA_ENOMEM, "out of memory"); }
  if (!onDevice) memcpy(c->hostBlob.data(), blob, nbytes);
  HIP_TRY(hipMalloc((void **) &c->dBlob, nbytes));
  c->statSceneAllocs++;
  HIP_TRY(hipMemcpy(c->dBlob, blob, nbytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  c->statBytesCopied = nbytes;
  if (onDevice) HIP_TRY(hipMemcpy(c->hostBlob.data(), blob, nbytes, hipMemcpyDeviceToHost));
  const int rc = PrepareScene(c);
  if (rc != QA_OK) FreeScene(c);
  return rc;
}
int qa_scene_upload(qa_ctx *c, const void *host_blob, uint64_t nbytes) { return Upload(c, host_blob, nbytes, false); }
int qa_scene_upload_device(qa_ctx *c, const void *device_blob, uint64_t nbytes) { return Upload(c, device_blob, nbytes, true); }

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
  memcpy(ds.background, t.ds.background, sizeof(ds.background));
  memcpy(ds.environment, t.ds.environment, sizeof(ds.environment));
  ds.rootIdentity = t.ds.rootIdentity;
  ds.csCullS1 = t.ds.csCullS1; ds.csCullS2 = t.ds.csCullS2; ds.csCullK3 = t.ds.csCullK3; ds.csCullK4 = t.ds.csCullK4;
  memcpy(ds.instv, t.ds.instv, sizeof(ds.instv));
  return EnsurePlanSlab(c);
}

struct EditCopy { const void *dst; const void *src; size_t bytes; };

// `need` bytes of the pinned ring (64-byte aligned), valid until a later edit wraps the ring - which first waits for lastEdit, so
// whoever reads them on the device records lastEdit behind that work
int EditStageReserve(qa_ctx *c, size_t need, unsigned char **at)
{
  need = (need + 63) & ~(size_t) 63;
  if (need > c->editStageBytes) {
    if (c->lastEdit.set) HIP_TRY(hipEventSynchronize(c->lastEdit.ev));
    if (c->hEditStage) (void) hipHostFree(c->hEditStage);
    c->hEditStage = nullptr;
    c->editStageBytes = c->editStageUsed = 0;
    const size_t bytes = std::max<size_t>(256 * 1024, 8 * need);
    HIP_TRY(hipHostMalloc((void **) &c->hEditStage, bytes, hipHostMallocDefault));
    c->editStageBytes = bytes;
  }
  if (c->editStageUsed + need > c->editStageBytes) {   // the ring wraps: the copies of the edits before this one must have left it
    if (c->lastEdit.set) HIP_TRY(hipEventSynchronize(c->lastEdit.ev));
    c->editStageUsed = 0;
  }
  *at = c->hEditStage + c->editStageUsed;
  c->editStageUsed += need;
  return QA_OK;
}

// What an edit's device work waits for: a frame on a stream of the caller's may still read the tables
int EditBegin(qa_ctx *c)
{
  HIP_TRY(c->lastFrame.WaitOn(c->stream));
  if (c->prog.active) HIP_TRY(c->prog.done.WaitOn(c->stream));
  c->statBytesCopied = 0;
  return QA_OK;
}

// The copies of one edit: through the pinned ring, asynchronously on the context's stream
static int EnqueueEditCopies(qa_ctx *c, const std::vector<EditCopy> &copies)
{
  size_t need = 0;
  for (const EditCopy &k : copies) need += (k.bytes + 63) & ~(size_t) 63;
  unsigned char *stage = nullptr;
  int rc = EditStageReserve(c, need, &stage);
  if (rc != QA_OK || (rc = EditBegin(c)) != QA_OK) return rc;
  for (const EditCopy &k : copies) {
    if (!k.bytes || !k.dst) continue;
    memcpy(stage, k.src, k.bytes);
    HIP_TRY(hipMemcpyAsync(const_cast<void *>(k.dst), stage, k.bytes, hipMemcpyHostToDevice, c->stream));
    stage += (k.bytes + 63) & ~(size_t) 63;
    c->statBytesCopied += k.bytes;
  }
  HIP_TRY(c->lastEdit.Record(c->stream));
  return QA_OK;
}

// What every edit ends with.  The photon maps do not depend on the camera; every other edit ends Scene::usePhotonMap as an upload
// does (the maps' memory goes with the next upload, build, clear or the context: releasing it here would wait for the device)
int EditEnd(qa_ctx *c, bool keepsPhotonMaps)
{
  if (keepsPhotonMaps) SetKernelName(c);   // (the plan cannot change; the name is the plan's again, as after an upload)
  else {
    c->photonReady = false;
    SelectStaged(c);
    if (int rc = SelectKernel(c)) return rc;
  }
  if (c->prog.active) c->prog.stale = true;
  c->statEdits++;
  return QA_OK;
}

enum EditKind { kEditCamera, kEditLights, kEditMaterials, kEditInstances, kEditTexmaps, kEditTextures, kEditBackdrop };

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
  // (texmaps, texture colours, backdrop: the kernels read the records in the device blob, the two colours travel in DScene)
  if ((rc = EnqueueEditCopies(c, copies)) != QA_OK) return rc;
  return EditEnd(c, kind == kEditCamera);
}

// What every edit checks first; *h: the resident blob's header, whose `count` says how many records the edited table has
static int EditArgs(qa_ctx *c, const void *records, uint32_t first, uint32_t n, uint32_t qa_flat_header::*count, const qa_flat_header **h)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (!records) return Fail(QA_EINVAL, "null argument");
  *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  const uint32_t have = count ? (*h)->*count : 0;
  if (first > have || n > have - first) return Fail(QA_EINVAL, "records beyond the scene's table");
  return QA_OK;
}

extern "C" {

int qa_scene_edit_camera(qa_ctx *c, const qa_camera *cam)
{
  const qa_flat_header *h;
  int rc = EditArgs(c, cam, 0, 0, nullptr, &h);
  if (rc != QA_OK) return rc;
  static_assert(offsetof(qa_flat_header, dof) + sizeof(float) - offsetof(qa_flat_header, screenA) == sizeof(qa_camera), "qa_camera is the header's camera block");
  return ApplyEdit(c, kEditCamera, offsetof(qa_flat_header, screenA), cam, sizeof(qa_camera));
}

int qa_scene_edit_lights(qa_ctx *c, uint32_t first, uint32_t n, const qa_light *lights)
{
  const qa_flat_header *h;
  int rc = EditArgs(c, lights, first, n, &qa_flat_header::num_lights, &h);
  if (rc != QA_OK || n == 0) return rc;
  return ApplyEdit(c, kEditLights, h->off_lights + (size_t) first * sizeof(qa_light), lights, (size_t) n * sizeof(qa_light));
}

int qa_scene_edit_materials(qa_ctx *c, uint32_t first, uint32_t n, const qa_material *materials)
{
  const qa_flat_header *h;
  int rc = EditArgs(c, materials, first, n, &qa_flat_header::num_materials, &h);
  if (rc != QA_OK || n == 0) return rc;
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
  const qa_flat_header *h;
  int rc = EditArgs(c, instances, first, n, &qa_flat_header::num_instances, &h);
  if (rc != QA_OK || n == 0) return rc;
  const qa_instance *cur = QA_BLOB_PTR(qa_instance, c->hostBlob.data(), h->off_instances) + first;
  for (uint32_t i = 0; i < n; ++i) {
    const qa_instance &a = cur[i], &b = instances[i];
    if (a.obj_type != b.obj_type || a.mesh != b.mesh || a.mtlset != b.mtlset || a.parent != b.parent || a.subtree_end != b.subtree_end ||
        a.depth != b.depth)
      return Fail(QA_EINVAL, "an instance edit can change tm, itm and pos only (object, mesh, material set and place in the graph stay): upload the scene instead");
  }
  return ApplyEdit(c, kEditInstances, h->off_instances + (size_t) first * sizeof(qa_instance), instances, (size_t) n * sizeof(qa_instance));
}

int qa_scene_edit_texmaps(qa_ctx *c, uint32_t first, uint32_t n, const qa_texmap *texmaps)
{
  const qa_flat_header *h;
  int rc = EditArgs(c, texmaps, first, n, &qa_flat_header::num_texmaps, &h);
  if (rc != QA_OK || n == 0) return rc;
  // (a texture index out of range: RebuildSceneSide validates the records as an upload does)
  return ApplyEdit(c, kEditTexmaps, h->off_texmaps + (size_t) first * sizeof(qa_texmap), texmaps, (size_t) n * sizeof(qa_texmap));
}

int qa_scene_edit_textures(qa_ctx *c, uint32_t first, uint32_t n, const qa_texture *textures)
{
  const qa_flat_header *h;
  int rc = EditArgs(c, textures, first, n, &qa_flat_header::num_textures, &h);
  if (rc != QA_OK || n == 0) return rc;
  // (a record of another type, size or texel offset: RebuildSceneSide refuses it)
  return ApplyEdit(c, kEditTextures, h->off_textures + (size_t) first * sizeof(qa_texture), textures, (size_t) n * sizeof(qa_texture));
}

int qa_scene_edit_backdrop(qa_ctx *c, const qa_texcolor *background, const qa_texcolor *environment)
{
  const qa_flat_header *h;
  int rc = EditArgs(c, c, 0, 0, nullptr, &h);
  if (rc != QA_OK || (!background && !environment)) return rc;
  static_assert(offsetof(qa_flat_header, environment) == offsetof(qa_flat_header, background) + sizeof(qa_texcolor), "the header's two backdrop colours are adjacent");
  const qa_texcolor both[2] = {background ? *background : h->background, environment ? *environment : h->environment};
  return ApplyEdit(c, kEditBackdrop, offsetof(qa_flat_header, background), both, sizeof(both));
}

int qa_scene_download(qa_ctx *c, void *out, uint64_t capacity, uint64_t *nbytes)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (nbytes) *nbytes = c->hostBlob.size();
  if (!out || capacity < c->hostBlob.size()) return Fail(QA_EINVAL, "output smaller than the scene blob");
  if (int rc = FetchDeviceTexels(c)) return rc;   // (textures edited from device memory: qa_texture_edit.hip)
  memcpy(out, c->hostBlob.data(), c->hostBlob.size());
  return QA_OK;
}

int qa_get_scene_stats(qa_ctx *c, uint64_t out[4])
{
  if (!c || !out) return Fail(QA_EINVAL, "null argument");
  out[0] = c->statMeshBuilds; out[1] = c->statSceneAllocs; out[2] = c->statBytesCopied; out[3] = c->statEdits;
  return QA_OK;
}

int qa_synchronize(qa_ctx *c)
{
  if (int rc = Enter(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DrainEvents(c);
}

static int SetStop(qa_ctx *c, int stop)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  __atomic_store_n(c->hStop, stop, __ATOMIC_SEQ_CST);
  return QA_OK;
}
int qa_request_stop(qa_ctx *c) { return SetStop(c, 1); }
int qa_clear_stop(qa_ctx *c) { return SetStop(c, 0); }

int qa_get_counters(qa_ctx *c, qa_counters *out)
{
  if (!c || !out) return Fail(QA_EINVAL, "null argument");
  if (int rc = qa_synchronize(c)) return rc;
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
    if (h.stamp[19] || h.stamp[21])
      fprintf(stderr, "[stamps] waves without a camera ray: mesh walks of their closest-hit sweeps %.3f (the camera rays': %.3f), after the sweep %.3f | last-cast queries %.3f (mesh walks %.3f), %llu lanes asked again (of %llu casts)\n",
              h.stamp[19] / k, (h.stamp[3] - (double) h.stamp[19]) / k, h.stamp[20] / k, h.stamp[21] / k, h.stamp[22] / k, h.stamp[23], (unsigned long long) h.casts_normal);
    if (!c->integ[kCs].fn && h.stamp[16])   // qa_integrate_lastcast: slots 15 / 16 (the cooperative kernel's otherwise) are the turns of tiles that tileIsEmpty calls empty (qa_emptytile.h)
      fprintf(stderr, "[stamps] turns of empty tiles: %llu of %llu turns (%.3f), share of wave time %.4f\n", h.stamp[16], h.stamp[8], (double) h.stamp[16] / (double) std::max<unsigned long long>(h.stamp[8], 1), h.stamp[15] / k);
    if (!c->integ[kCs].fn && h.stamp[17])   // qa_integrate_lastcast: slots 13 / 14 / 17 / 18 are the two phases of the queries' leaf sweep (qa_kernel.h sweepLeaves)
      fprintf(stderr, "[stamps] leaf sweep: box phase %.4f, triangle phase %.4f of wave time | triangle phase: %.1f turns per wave, %.2f of 64 lanes in a turn, %.1f cycles per turn\n", h.stamp[13] / k, h.stamp[14] / k,
              h.stamp[17] / w, (double) h.stamp[18] / (double) h.stamp[17], (double) h.stamp[14] / (double) h.stamp[17]);
    if (c->integ[kCs].fn && h.stamp[11])   // qa_integrate_cs reuses slots 10 / 11: items taken from the pool / rounds of the cooperative walks
      fprintf(stderr, "[stamps] cooperative walks: %llu rounds, %.1f of 64 lanes hold an item on average (lane occupancy of the walks %.3f); %.3f of the rounds are leaf rounds; 'mesh walks' above = the rounds alone\n", h.stamp[11],
              (double) h.stamp[10] / (double) h.stamp[11], (double) h.stamp[10] / (64.0 * (double) h.stamp[11]), (double) h.stamp[12] / (double) h.stamp[11]);
    if (c->integ[kCs].fn)
      fprintf(stderr, "[stamps] closest-hit sweeps without their rounds %.3f, winners' details %.3f, shadow sweeps without their rounds %.3f; lanes sent to the exact walks: %llu closest, %llu shadow (of %llu + %llu casts)\n",
              (h.stamp[13] - (double) h.stamp[3]) / k, h.stamp[14] / k, (h.stamp[17] - (double) h.stamp[6]) / k, h.stamp[15], h.stamp[16], (unsigned long long) h.casts_normal, (unsigned long long) h.casts_shadow);
  }
#endif
  return QA_OK;
}
int qa_reset_counters(qa_ctx *c)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (int rc = qa_synchronize(c)) return rc;
  HIP_TRY(hipMemset(c->dCounters, 0, sizeof(DCounters)));
  if (c->wf.dStats) HIP_TRY(hipMemset(c->wf.dStats, 0, sizeof(WfStats)));
  c->wf.iterations = c->wf.raysClosest = c->wf.raysShadow = c->wf.jobs = c->wf.redo = 0;
  return QA_OK;
}

int qa_get_staged_stats(qa_ctx *c, uint64_t out[QA_STAGED_STATS])
{
  if (!c || !out) return Fail(QA_EINVAL, "null argument");
  if (int rc = qa_synchronize(c)) return rc;
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
  int rc = Enter(c);
  if (rc != QA_OK || (rc = DrainEvents(c)) != QA_OK) return rc;
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
  else if (n == "last_cast") c->optLastCast = value < 0 ? -1 : (value ? 1 : 0);
  else if (n == "leaf_sweep") c->optLeafSweep = value < 0 ? -1 : (value ? 1 : 0);
  else if (n == "empty_tiles") c->optEmptyTiles = value < 0 ? -1 : (value ? 1 : 0);
  else if (n == "chunk_spp") c->optChunkSpp = value < 0 ? -1 : (int) (value > 65535 ? 65535 : value);
  else if (n == "chunk_tail") c->optChunkTail = value < 0 ? 0 : (int) (value > 65535 ? 65535 : value);
  else if (n == "tile_lists") c->optTileLists = value < 0 ? -1 : (int) (value > QA_TILE_LEAF_CAP ? QA_TILE_LEAF_CAP : value);
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

int qa_set_launch_config(qa_ctx *c, int blocks_per_cu, int threads_per_block)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (threads_per_block != 0 && threads_per_block != QA_BLOCK) return Fail(QA_EINVAL, "this build supports 256-thread workgroups only");
  if (blocks_per_cu < 0 || blocks_per_cu > 8) return Fail(QA_EINVAL, "blocks_per_cu must be in 0..8");
  c->optBlocksPerCU = blocks_per_cu;
  return QA_OK;
}

}  // extern "C"
