// qa_bake.hip — bake maps on the resident scene: the surface point behind every texel of a texture laid over a node
// (qa_bake_texels*), and the gutter fill of a baked picture (qa_bake_dilate_device).  qa_bake_dev.h is the specification and holds
// every function of both sides; here are the two kernels, the checks and the C entries.  The map kernel only reads the scene: the
// node's raw mesh arrays, the instance table and nothing else of the resident blob; no integrator kernel, slab, counter of
// qa_get_counters, kernel-time record or progressive frame is touched.  No reference counterpart (the reference bakes nothing).
//
// Shape, map: a workgroup of 256 lanes owns a 16x16 texel tile (lane = texel, 16 texels of a row side by side, so every plane's
// stores are row-contiguous).  Faces are taken in chunks of 256: each lane sets up one face of the chunk (its three T, d, the first
// tile and the tile counts, the box) into LDS as SoA, once per workgroup; behind the barrier every lane walks the chunk in ascending
// order, reading the face by broadcast.  A face whose tile-expanded box misses the wave's texel rectangle is skipped by a
// wave-uniform branch - the test is the per-lane box test of the specification applied to the rectangle's ends, and fp32 addition is
// monotone, so it skips nothing a lane would accept.  A wave leaves the walk when all its lanes are covered; the workgroup leaves the
// chunk loop when all its waves have.  The details and the world transform run once per covered lane, after the walk.
// Shape, fill: a 16x16 tile with a halo of QA_BAKE_MAX_RADIUS texels of covered flags in LDS, one gather pass.
// No atomics, no inline assembly.
#include <algorithm>

#include "qa_ctx.h"
#include "qa_bake_dev.h"
#include "qa_stage.h"

namespace qa {

#define QA_BAKE_TILE 16u
#define QA_BAKE_CHUNK 256u
static_assert(QA_BLOCK == QA_BAKE_TILE * QA_BAKE_TILE && QA_BLOCK == QA_BAKE_CHUNK, "lane = texel of the tile = face of the chunk");

struct BakeParams {
  BakeSource src;             // device pointers
  const qa_instance *inst;    // the resident blob's table
  int32_t node;
  uint32_t rootIdentity;
  uint32_t W, H;
  BakePlanes o;
};

// does some tile of the axis bring a sample of [lo, hi] into [b0, b1]?  (what bakeInside asks of one sample, for the interval's ends)
__device__ __forceinline__ bool bakeAxisMeets(float lo, float hi, float f0, uint32_t n, float b0, float b1)
{
  bool any = false;
  for (uint32_t j = 0; j < n; ++j) {
    const float m = f0 + (float) j;
    any = any || (hi + m >= b0 && lo + m <= b1);
  }
  return any;
}

__device__ __forceinline__ float waveMin(float v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float waveMax(float v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

__global__ __launch_bounds__(QA_BLOCK) void qa_bake_texels_k(const DScene sc, const BakeParams bp)
{
  (void) sc;   // (LaunchSceneKernel's first argument; the map reads the blob's raw arrays)
  enum { T0X, T0Y, T1X, T1Y, T2X, T2Y, D, FM0, FN0, BX0, BX1, BY0, BY1, NFLOAT };
  __shared__ float sF[NFLOAT][QA_BAKE_CHUNK];
  __shared__ uint32_t sCnt[QA_BAKE_CHUNK];   // nm | nn << 8; 0: void

  const uint32_t W = bp.W, H = bp.H, tid = threadIdx.x;
  const uint32_t tilesX = (W + QA_BAKE_TILE - 1) / QA_BAKE_TILE, tilesY = (H + QA_BAKE_TILE - 1) / QA_BAKE_TILE;
  const uint32_t numTiles = tilesX * tilesY, numFaces = bp.src.numFaces;

  for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const uint32_t ix = (tile % tilesX) * QA_BAKE_TILE + (tid % QA_BAKE_TILE), iy = (tile / tilesX) * QA_BAKE_TILE + (tid / QA_BAKE_TILE);
    const bool inside = ix < W && iy < H;   // else: padding slot of a ragged tile
    float sx, sy;
    bakeSample(min(ix, W - 1), min(iy, H - 1), W, H, sx, sy);   // (a padding slot takes the edge texel's sample: the rectangle stays the wave's)
    const float rx0 = waveMin(sx), rx1 = waveMax(sx), ry0 = waveMin(sy), ry1 = waveMax(sy);

    bool done = !inside;
    int32_t face = -1;
    float e0 = 0.f, e1 = 0.f, fd = 1.f;
    for (uint32_t base = 0; base < numFaces; base += QA_BAKE_CHUNK) {
      {
        BakeFace bf = {};
        if (base + tid < numFaces) bf = bakeFaceSetup(bp.src, base + tid);
        sF[T0X][tid] = bf.t0x; sF[T0Y][tid] = bf.t0y; sF[T1X][tid] = bf.t1x; sF[T1Y][tid] = bf.t1y; sF[T2X][tid] = bf.t2x; sF[T2Y][tid] = bf.t2y;
        sF[D][tid] = bf.d; sF[FM0][tid] = bf.fm0; sF[FN0][tid] = bf.fn0;
        sF[BX0][tid] = bf.bx0; sF[BX1][tid] = bf.bx1; sF[BY0][tid] = bf.by0; sF[BY1][tid] = bf.by1;
        sCnt[tid] = bf.nm | (bf.nn << 8);
      }
      __syncthreads();
      if (!__all(done)) {
        const uint32_t count = min(QA_BAKE_CHUNK, numFaces - base);
        for (uint32_t k = 0; k < count; ++k) {
          const uint32_t cnt = sCnt[k];
          if (!cnt) continue;
          BakeFace bf;
          bf.nm = cnt & 0xFFu;
          bf.nn = cnt >> 8;
          bf.fm0 = sF[FM0][k]; bf.fn0 = sF[FN0][k];
          bf.bx0 = sF[BX0][k]; bf.bx1 = sF[BX1][k]; bf.by0 = sF[BY0][k]; bf.by1 = sF[BY1][k];
          if (!(bakeAxisMeets(rx0, rx1, bf.fm0, bf.nm, bf.bx0, bf.bx1) && bakeAxisMeets(ry0, ry1, bf.fn0, bf.nn, bf.by0, bf.by1))) continue;
          if (!done) {
            bf.t0x = sF[T0X][k]; bf.t0y = sF[T0Y][k]; bf.t1x = sF[T1X][k]; bf.t1y = sF[T1Y][k]; bf.t2x = sF[T2X][k]; bf.t2y = sF[T2Y][k];
            bf.d = sF[D][k];
            bf.over = 0;
            float a, b;
            if (bakeFaceCovers(bf, sx, sy, a, b)) {
              done = true;
              face = (int32_t) (base + k);
              e0 = a;
              e1 = b;
              fd = bf.d;
            }
          }
          if (__all(done)) break;
        }
      }
      if (__syncthreads_and(done)) break;   // (also the barrier ahead of the next chunk's setup)
    }

    if (!inside) continue;
    float a = 0.f, b = 0.f;
    f3 p = F3(0.f, 0.f, 0.f), N = F3(0.f, 0.f, 0.f);
    if (face >= 0) bakeDetails(bp.src, bp.inst, bp.node, bp.rootIdentity != 0, (uint32_t) face, fd, e0, e1, a, b, p, N);
    bakeStore(bp.o, (size_t) iy * W + ix, face, a, b, p, N);
  }
}

struct BakeLdsCovered {
  const uint8_t (*cov)[QA_BAKE_TILE + 2 * QA_BAKE_MAX_RADIUS];
  uint32_t lx, ly;
  __device__ bool operator()(int dx, int dy) const { return cov[(int) (ly + QA_BAKE_MAX_RADIUS) + dy][(int) (lx + QA_BAKE_MAX_RADIUS) + dx] != 0; }
};

__global__ __launch_bounds__(256) void qa_bake_dilate_k(const uint8_t *rgb8, const int32_t *face, uint32_t W, uint32_t H, uint32_t radius, uint8_t *out)
{
  constexpr uint32_t SIDE = QA_BAKE_TILE + 2 * QA_BAKE_MAX_RADIUS;
  __shared__ uint8_t sCov[SIDE][SIDE];
  const uint32_t tid = threadIdx.x, lx = tid % QA_BAKE_TILE, ly = tid / QA_BAKE_TILE;
  const uint32_t tilesX = (W + QA_BAKE_TILE - 1) / QA_BAKE_TILE, tilesY = (H + QA_BAKE_TILE - 1) / QA_BAKE_TILE;
  for (uint32_t tile = blockIdx.x; tile < tilesX * tilesY; tile += gridDim.x) {
    const int x0 = (int) ((tile % tilesX) * QA_BAKE_TILE), y0 = (int) ((tile / tilesX) * QA_BAKE_TILE);
    for (uint32_t k = tid; k < SIDE * SIDE; k += 256) {
      const uint32_t cx = k % SIDE, cy = k / SIDE;
      const uint32_t gx = bakeWrap(x0 + (int) cx - (int) QA_BAKE_MAX_RADIUS, W), gy = bakeWrap(y0 + (int) cy - (int) QA_BAKE_MAX_RADIUS, H);
      sCov[cy][cx] = face[(size_t) gy * W + gx] >= 0;
    }
    __syncthreads();
    const uint32_t x = (uint32_t) x0 + lx, y = (uint32_t) y0 + ly;
    if (x < W && y < H) {
      const size_t q = (size_t) y * W + x;
      size_t from = q;
      if (!sCov[ly + QA_BAKE_MAX_RADIUS][lx + QA_BAKE_MAX_RADIUS]) {
        const BakeLdsCovered cov = {sCov, lx, ly};
        int dx = 0, dy = 0;
        if (bakeDilatePick((int) radius, cov, dx, dy)) from = (size_t) bakeWrap((int) y + dy, H) * W + bakeWrap((int) x + dx, W);
      }
      out[3 * q] = rgb8[3 * from];
      out[3 * q + 1] = rgb8[3 * from + 1];
      out[3 * q + 2] = rgb8[3 * from + 2];
    }
    __syncthreads();   // (the next tile's flags)
  }
}

}  // namespace qa

// ---- host side ------------------------------------------------------------------------------------

// Is [off, off + bytes) inside a blob of n bytes?
static bool InBlob(uint64_t off, uint64_t bytes, uint64_t n) { return off <= n && bytes <= n - off; }

// What the self-test hook asks of a blob nothing has validated (an uploaded one went through BuildScene): the tables the map reads
// lie inside it, the node's chain of parents ends at the root, and its mesh's vertex and normal indices are in range
static int BakeValidateBlob(const unsigned char *blob, uint64_t nbytes, int node)
{
  if (!blob || nbytes < sizeof(qa_flat_header)) return Fail(QA_EINVAL, "no blob");
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(blob);
  if (h->magic != QA_FLAT_MAGIC || h->version != QA_FLAT_VERSION || h->total_bytes > nbytes) return Fail(QA_EINVAL, "not a flat scene blob");
  const uint64_t n = h->total_bytes;
  if (!InBlob(h->off_instances, (uint64_t) h->num_instances * sizeof(qa_instance), n) || !InBlob(h->off_meshes, (uint64_t) h->num_meshes * sizeof(qa_mesh), n) ||
      !InBlob(h->off_texmaps, (uint64_t) h->num_texmaps * sizeof(qa_texmap), n) || h->num_instances == 0)
    return Fail(QA_EINVAL, "a table of the blob lies outside it");
  if (node < 0 || (uint32_t) node >= h->num_instances) return QA_OK;   // (refused by name later)
  const qa_instance *inst = QA_BLOB_PTR(qa_instance, blob, h->off_instances);
  for (int at = node; at > 0; at = inst[at].parent)
    if (inst[at].parent < 0 || inst[at].parent >= at) return Fail(QA_EINVAL, "the node's parents are not in pre-order");
  const qa_instance &in = inst[node];
  if (in.obj_type != QA_OBJ_MESH) return QA_OK;
  if (in.mesh < 0 || (uint32_t) in.mesh >= h->num_meshes) return Fail(QA_EINVAL, "mesh index out of range");
  const qa_mesh &m = QA_BLOB_PTR(qa_mesh, blob, h->off_meshes)[in.mesh];
  if (!InBlob(m.off_faces, (uint64_t) m.num_faces * sizeof(qa_face), n) || !InBlob(m.off_vertices, (uint64_t) m.num_vertices * 12, n) ||
      !InBlob(m.off_normals, (uint64_t) m.num_normals * 12, n) || !InBlob(m.off_texcoords, (uint64_t) m.num_texcoords * 8, n))
    return Fail(QA_EINVAL, "a mesh array lies outside the blob");
  const qa_face *faces = QA_BLOB_PTR(qa_face, blob, m.off_faces);
  for (uint32_t f = 0; f < m.num_faces; ++f)
    for (int q = 0; q < 3; ++q)
      if (faces[f].v[q] < 0 || (uint32_t) faces[f].v[q] >= m.num_vertices || faces[f].vn[q] < 0 || (uint32_t) faces[f].vn[q] >= m.num_normals)
        return Fail(QA_EINVAL, "vertex or normal index out of range");
  return QA_OK;
}

struct BakeCall {
  BakeSource src;          // pointers into the blob it was resolved against
  const qa_instance *inst;
  bool rootIdentity;
};

// Every refusal of the specification that does not need a context, in its order, and the source of the faces over `blob`
static int BakeResolve(const unsigned char *blob, int node, int texmap, int mtl, uint32_t W, uint32_t H, bool anyPlane, BakeCall &call)
{
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(blob);
  if (W == 0 || H == 0 || W > QA_BAKE_MAX_DIM || H > QA_BAKE_MAX_DIM) return Fail(QA_EINVAL, "bad size: 1 .. 8192 texels per side");
  if (!anyPlane) return Fail(QA_EINVAL, "no output plane");
  if (node < 0 || (uint32_t) node >= h->num_instances) return Fail(QA_EINVAL, "node index out of range");
  if (mtl < -1) return Fail(QA_EINVAL, "bad mtl: a face's material index, or -1 for every face");
  const qa_instance *inst = QA_BLOB_PTR(qa_instance, blob, h->off_instances);
  const qa_instance &in = inst[node];
  if (in.obj_type == QA_OBJ_NONE) return Fail(QA_EINVAL, "the node has no object");
  if (in.obj_type == QA_OBJ_SPHERE) return Fail(QA_EUNSUPPORTED, "a sphere node: its inverse map needs double-precision trigonometry that nothing here pins");
  BakeSource &src = call.src;
  src = BakeSource{};
  src.mtl = mtl;
  if (texmap < -1 || (texmap >= 0 && (uint32_t) texmap >= h->num_texmaps)) return Fail(QA_EINVAL, "texmap index out of range");
  if (texmap >= 0) {
    src.map = QA_BLOB_PTR(qa_texmap, blob, h->off_texmaps)[texmap];
    if (src.map.texture < 0) return Fail(QA_EINVAL, "the texmap has no texture");
    src.mapped = 1;
  }
  if (in.obj_type == QA_OBJ_PLANE) {
    src.plane = 1;
    src.numFaces = 2;
  } else {
    const qa_mesh &m = QA_BLOB_PTR(qa_mesh, blob, h->off_meshes)[in.mesh];
    if (m.num_texcoords == 0) return Fail(QA_EINVAL, "the mesh has no texture vertices");
    src.faces = QA_BLOB_PTR(qa_face, blob, m.off_faces);
    src.vertices = QA_BLOB_PTR(float, blob, m.off_vertices);
    src.normals = QA_BLOB_PTR(float, blob, m.off_normals);
    src.texcoords = QA_BLOB_PTR(float, blob, m.off_texcoords);
    src.numFaces = m.num_faces;
    src.numTexcoords = m.num_texcoords;
  }
  if (bakeOverTiles(src)) return Fail(QA_EUNSUPPORTED, "a face's texture vertices span more than 4 tiles of the texture along an axis");
  call.inst = inst;
  // DScene::rootIdentity, as BuildScene decides it
  static const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z3[3] = {0, 0, 0};
  call.rootIdentity = memcmp(inst[0].tm, I9, 36) == 0 && memcmp(inst[0].itm, I9, 36) == 0 && memcmp(inst[0].pos, Z3, 12) == 0;
  return QA_OK;
}

template <class T>
static const T *Rebase(const T *p, const unsigned char *from, const unsigned char *to)
{
  return p ? reinterpret_cast<const T *>(to + (reinterpret_cast<const unsigned char *>(p) - from)) : nullptr;
}

// The static LDS of the map kernel (14 words per face of the chunk, and the barrier's own) rides on top of the dynamic LDS
// LaunchSceneKernel gives every scene kernel
static const size_t kBakeStaticLds = 15 * 1024;

// What both forms check, in the specification's order, before anything is sized or written -> the call resolved over the host blob
static int BakeCheck(qa_ctx *c, int node, int texmap, int mtl, uint32_t W, uint32_t H, bool anyPlane, BakeCall &call)
{
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (int rc = BakeResolve(c->hostBlob.data(), node, texmap, mtl, W, H, anyPlane, call)) return rc;
  if (c->integ[kMega].ldsBytes + kBakeStaticLds > kMaxLdsPerBlock)
    return Fail(QA_EUNSUPPORTED, "the scene's traversal stacks leave no LDS for the map's face chunk");
  return QA_OK;
}

// The launch of a checked call: the source's pointers move from the host blob to the resident one
static int BakeTexels(qa_ctx *c, const BakeCall &call, int node, uint32_t W, uint32_t H, const BakePlanes &o, hipStream_t s)
{
  const unsigned char *hb = c->hostBlob.data();
  BakeParams bp;
  bp.src = call.src;
  bp.src.faces = Rebase(call.src.faces, hb, c->dBlob);
  bp.src.vertices = Rebase(call.src.vertices, hb, c->dBlob);
  bp.src.normals = Rebase(call.src.normals, hb, c->dBlob);
  bp.src.texcoords = Rebase(call.src.texcoords, hb, c->dBlob);
  bp.inst = Rebase(call.inst, hb, c->dBlob);
  bp.node = node;
  bp.rootIdentity = call.rootIdentity ? 1u : 0u;
  bp.W = W;
  bp.H = H;
  bp.o = o;
  const long long tiles = (long long) ((W + QA_BAKE_TILE - 1) / QA_BAKE_TILE) * ((H + QA_BAKE_TILE - 1) / QA_BAKE_TILE);
  return LaunchSceneKernel(c, qa_bake_texels_k, bp, tiles, s);
}

extern "C" {

int qa_bake_texels_device(qa_ctx *c, int node, int texmap, int mtl, uint32_t width, uint32_t height, float *d_point, float *d_normal, int32_t *d_face,
                          float *d_bary, void *stream)
{
  if (int rc = Enter(c)) return rc;
  const BakePlanes o = {d_point, d_normal, d_face, d_bary};
  BakeCall call;
  if (int rc = BakeCheck(c, node, texmap, mtl, width, height, d_point || d_normal || d_face || d_bary, call)) return rc;
  return BakeTexels(c, call, node, width, height, o, StreamOf(c, stream));
}

int qa_bake_texels(qa_ctx *c, int node, int texmap, int mtl, uint32_t width, uint32_t height, float *point, float *normal, int32_t *face, float *bary)
{
  if (int rc = Enter(c)) return rc;
  BakeCall call;
  if (int rc = BakeCheck(c, node, texmap, mtl, width, height, point || normal || face || bary, call)) return rc;   // before anything is sized
  const size_t n = (size_t) width * height;
  QueryStage st(c);
  const auto dP = st.Out(point, 3 * n), dN = st.Out(normal, 3 * n);
  const auto dF = st.Out(face, n);
  const auto dB = st.Out(bary, 2 * n);
  if (int rc = st.Begin()) return rc;
  const BakePlanes dev = {st(dP), st(dN), st(dF), st(dB)};
  if (int rc = BakeTexels(c, call, node, width, height, dev, c->stream)) return rc;
  return st.End();
}

static int CheckDilate(const uint8_t *rgb8, const int32_t *face, uint32_t W, uint32_t H, uint32_t radius, const uint8_t *out)
{
  if (!rgb8 || !face || !out) return Fail(QA_EINVAL, "null buffer");
  if (W == 0 || H == 0 || W > QA_BAKE_MAX_DIM || H > QA_BAKE_MAX_DIM) return Fail(QA_EINVAL, "bad size: 1 .. 8192 texels per side");
  if (radius > QA_BAKE_MAX_RADIUS) return Fail(QA_EINVAL, "bad radius: 0 .. 8 texels");
  const size_t bytes = 3 * (size_t) W * H;
  if (out < rgb8 + bytes && rgb8 < out + bytes) return Fail(QA_EINVAL, "out overlaps the picture: the fill is a gather and cannot run in place");
  return QA_OK;
}

int qa_bake_dilate_device(qa_ctx *c, const uint8_t *d_rgb8, const int32_t *d_face, uint32_t width, uint32_t height, uint32_t radius, uint8_t *d_out,
                          void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = CheckDilate(d_rgb8, d_face, width, height, radius, d_out)) return rc;
  const uint32_t tiles = ((width + QA_BAKE_TILE - 1) / QA_BAKE_TILE) * ((height + QA_BAKE_TILE - 1) / QA_BAKE_TILE);
  const uint32_t blocks = std::max(1u, std::min(tiles, (uint32_t) c->numCUs * 8u));
  hipLaunchKernelGGL(qa::qa_bake_dilate_k, dim3(blocks), dim3(256), 0, StreamOf(c, stream), d_rgb8, d_face, width, height, radius, d_out);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// the same source on the CPU (no GPU, no context), from a blob of nbytes
int qa_test_bake_texels_host(const void *blob, uint64_t nbytes, int node, int texmap, int mtl, uint32_t width, uint32_t height, float *point,
                             float *normal, int32_t *face, float *bary)
{
  const unsigned char *b = static_cast<const unsigned char *>(blob);
  if (int rc = BakeValidateBlob(b, nbytes, node)) return rc;
  BakeCall call;
  if (int rc = BakeResolve(b, node, texmap, mtl, width, height, point || normal || face || bary, call)) return rc;
  const BakePlanes o = {point, normal, face, bary};
  for (uint32_t iy = 0; iy < height; ++iy)
    for (uint32_t ix = 0; ix < width; ++ix) bakeTexel(call.src, call.inst, node, call.rootIdentity, ix, iy, width, height, o);
  return QA_OK;
}

int qa_test_bake_dilate_host(const uint8_t *rgb8, const int32_t *face, uint32_t width, uint32_t height, uint32_t radius, uint8_t *out)
{
  if (int rc = CheckDilate(rgb8, face, width, height, radius, out)) return rc;
  for (uint32_t y = 0; y < height; ++y)
    for (uint32_t x = 0; x < width; ++x) bakeDilateTexel(rgb8, face, width, height, radius, x, y, out);
  return QA_OK;
}

}  // extern "C"
