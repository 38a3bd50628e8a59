// qa_probes.hip — test-only entries of libqaray_hip.so: the device build of qa_device_math.h and qa_texture_dev.h next to the host's,
// one query per lane (tests/test_device_math.py, tests/test_gpu_parity.py, tests/test_gpu_texture_*.py), and the scratch scrubber
#include <cstring>

#include "qa_device_math.h"
#include "qa_texture_dev.h"
#include "qa_ctx.h"
#include "qa_emptytile.h"

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
}  // namespace qa

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

// The scene tables of a host build as tileIsEmpty reads them (qa_emptytile.h)
struct EmptyTileSceneHost {
  const qa_instance *insts;
  const DMesh *meshes;
  const qa_instance &inst(int k) const { return insts[k]; }
  const DMesh &mesh(int i) const { return meshes[i]; }
};

int qa_test_empty_tiles_host(const void *blob, int x0, int y0, int x1, int y1, int first_strip, int strip_step, uint8_t *mask)
{
  if (!blob || !mask || first_strip < 0 || strip_step < 1) return QA_EINVAL;
  const qa_flat_header *h = static_cast<const qa_flat_header *>(blob);
  if (h->magic != QA_FLAT_MAGIC || h->version != QA_FLAT_VERSION) return QA_EINVAL;
  SceneTables t;
  std::string err;
  const int rc = BuildScene(static_cast<const unsigned char *>(blob), h->total_bytes, BuildKnobs(), t, &err);
  if (rc != QA_OK) return rc;
  const DScene &ds = t.ds;
  if (x0 < 0 || y0 < 0 || x1 > ds.cam.width || y1 > ds.cam.height || x1 <= x0 || y1 <= y0) return QA_EINVAL;
  const int tilesX = (x1 - x0 + 7) / 8, tilesY = (y1 - y0 + 7) / 8;
  // what a context's default options make of the scene (qa_frame.hip EmptyTilesOn)
  const bool on = t.plan.resident && t.plan.lastCastQuery && ds.num_lights == 0 && t.plan.tileListBytes && !(ds.cam.dof > 0.1f);
  const EmptyTileSceneHost s = {QA_BLOB_PTR(qa_instance, blob, h->off_instances), t.plan.meshes.data()};
  size_t n = 0;
  for (int row = first_strip; row < tilesY; row += strip_step)
    for (int tx = 0; tx < tilesX; ++tx) {
      TileCone cone;
      mask[n++] = on && tileIsEmpty(s, ds.cam, ds.background, ds.num_inst, ds.rootIdentity != 0, (float) (x0 + tx * 8), (float) (y0 + row * 8), &cone) ? 1 : 0;
    }
  return QA_OK;
}

int qa_debug_scrub_scratch(qa_ctx *c, uint32_t pattern)
{
  if (int rc = Enter(c)) return rc;
  // eight waves per SIMD on every CU: every wave slot of the chip - and with it every private segment the next launch can get -
  // holds a wave of this kernel at the same time (each lingers until the grid has been placed).  On every stream the context launches on
  std::vector<hipStream_t> streams = {c->stream};
  for (int g = 0; g < c->wf.numGroups; ++g) streams.push_back(c->wf.groups[g].stream);
  streams.push_back(c->wf.redoStream);
  for (hipStream_t s : streams)
    if (s) {
      hipLaunchKernelGGL(qa::qa_scrub_scratch, dim3((unsigned) c->numCUs * 8), dim3(256), 0, s, pattern, reinterpret_cast<uint32_t *>(c->dCounters));
      HIP_TRY(hipGetLastError());
    }
  HIP_TRY(hipDeviceSynchronize());
  return QA_OK;
}

}  // extern "C"
