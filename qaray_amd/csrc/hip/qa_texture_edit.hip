// qa_texture_edit.hip — texel edits of the resident scene (qa_scene_edit_texels, qa_scene_edit_texels_device): a rectangle of RGB8
// rows, staged from host memory through the pinned edit ring or already in device memory, goes into the device blob's texel bytes,
// and the float texel table's entries of the rectangle (DScene::texels, 16 bytes per texel) are recomputed where they are, by
// qa_texels_tabulate over qa_texel_dev.h - the source BuildTextures runs at an upload.  The record edits of the texture side
// (texmaps, texture colours, backdrop) are plain blob writes and live with the other edits in qa_capi.hip.
//
// The kernel is memory-bound: 3 bytes read, 3 + 16 written per texel.  tools/gpu_texture_edit_cost.py puts that beside the
// measured times.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "qa_ctx.h"
#include "qa_texel_dev.h"

namespace qa {

// Rows 0 .. h-1 of the source, `srcStride` bytes apart and w texels long, are texels (x0 .. x0 + w - 1, y0 + row) of a texture
// `pitch` texels wide whose bytes start at `bytes` and whose table entries at `entries` (null: the scene has no texel table)
struct TexelJob {
  const uint8_t *src;
  uint64_t srcStride;
  uint8_t *bytes;
  float4 *entries;
  uint32_t pitch, x0, y0, w, h;
};

__device__ __forceinline__ void texelOne(const TexelJob &j, const uint8_t *s, size_t q)
{
  const uint8_t r = s[0], g = s[1], b = s[2];
  uint8_t *d = j.bytes + 3 * q;
  d[0] = r; d[1] = g; d[2] = b;
  if (j.entries) j.entries[q] = texelEntry(r, g, b);
}

// A row is `perRow` = 1 + ceil(w / 4) items: item 0 its head, item k > 0 the four consecutive texels from head + 4 (k - 1) on, their
// 12 bytes read and written as three dwords and their entries as four float4.  The dwords need the source and the blob's bytes at
// the same offset from a 4-byte boundary: the head is then the 0 - 3 texels that lead up to the boundary (3 bytes each: as many
// texels as the offset), and the tail the texels of an incomplete last item.  Head, tail, and every item of a row whose source and
// destination disagree, go texel by texel.
__global__ __launch_bounds__(256) void qa_texels_tabulate(TexelJob j, uint32_t perRow)
{
  const uint64_t items = (uint64_t) j.h * perRow, total = (uint64_t) gridDim.x * 256u;
  for (uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x; t < items; t += total) {
    const uint32_t row = (uint32_t) (t / perRow), k = (uint32_t) (t - (uint64_t) row * perRow);
    const uint8_t *s = j.src + (uint64_t) row * j.srcStride;
    const size_t q0 = (size_t) (j.y0 + row) * j.pitch + j.x0;
    const uint32_t offS = (uint32_t) (reinterpret_cast<uintptr_t>(s) & 3u), offD = (uint32_t) (reinterpret_cast<uintptr_t>(j.bytes + 3 * q0) & 3u);
    const bool vec = offS == offD;
    const uint32_t head = vec ? min(offS, j.w) : 0u;
    if (k == 0) {
      for (uint32_t x = 0; x < head; ++x) texelOne(j, s + 3 * (size_t) x, q0 + x);
      continue;
    }
    const uint64_t xs = (uint64_t) head + 4ull * (k - 1);
    if (xs >= j.w) continue;
    if (vec && xs + 4 <= j.w) {
      const uint32_t *sw = reinterpret_cast<const uint32_t *>(s + 3 * xs);
      const uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2];
      uint32_t *dw = reinterpret_cast<uint32_t *>(j.bytes + 3 * (q0 + xs));
      dw[0] = w0; dw[1] = w1; dw[2] = w2;
      if (j.entries) {
        float4 *e = j.entries + q0 + xs;
        e[0] = texelEntry(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
        e[1] = texelEntry(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
        e[2] = texelEntry((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
        e[3] = texelEntry((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
      }
    } else {
      const uint64_t xe = min(xs + 4, (uint64_t) j.w);
      for (uint64_t x = xs; x < xe; ++x) texelOne(j, s + 3 * x, q0 + x);
    }
  }
}

}  // namespace qa

// One launch on the context's stream.  Full rows that follow each other without a gap on both sides are one long row: its items
// are whole but for one head and one tail
static int Tabulate(qa_ctx *c, qa::TexelJob j)
{
  if (j.x0 == 0 && j.w == j.pitch && (j.h == 1 || j.srcStride == 3ull * j.w) && (uint64_t) j.w * j.h <= 0x7FFFFFFFull &&
      (uint64_t) j.y0 * j.pitch <= 0x7FFFFFFFull) {
    j.x0 = j.y0 * j.pitch;
    j.w *= j.h;
    j.y0 = 0;
    j.h = 1;
  }
  const uint32_t perRow = 1u + (j.w + 3u) / 4u;
  const uint64_t items = (uint64_t) j.h * perRow;
  const uint32_t blocks = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t) c->numCUs * 8));
  hipLaunchKernelGGL(qa::qa_texels_tabulate, dim3(blocks), dim3(256), 0, c->stream, j, perRow);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// What both variants check first; *tx: the resident record of the texture
static int TexelArgs(qa_ctx *c, uint32_t texture, int x0, int y0, int x1, int y1, const void *src, uint64_t stride, const qa_texture **tx)
{
  if (!c) return Fail(QA_EINVAL, "null context");
  if (!c->haveScene) return Fail(QA_ENOSCENE, "no scene uploaded");
  if (!src) return Fail(QA_EINVAL, "null argument");
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  if (texture >= h->num_textures) return Fail(QA_EINVAL, "texture beyond the scene's table");
  const qa_texture &t = QA_BLOB_PTR(qa_texture, c->hostBlob.data(), h->off_textures)[texture];
  if (t.type != QA_TEX_FILE) return Fail(QA_EINVAL, "a checker texture has no texels (qa_scene_edit_textures changes its colours)");
  if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > t.width || y1 > t.height) return Fail(QA_EINVAL, "empty rectangle, or one beyond the texture");
  if (stride < 3ull * (uint64_t) (x1 - x0)) return Fail(QA_EINVAL, "row stride shorter than a row of the rectangle");
  *tx = &t;
  return QA_OK;
}

static qa::TexelJob JobOf(qa_ctx *c, uint32_t texture, const qa_texture &t)
{
  qa::TexelJob j{};
  j.bytes = c->dBlob + t.off_texels;
  j.entries = c->ds.texels ? const_cast<float4 *>(c->ds.texels) + c->tables.texOff[texture] : nullptr;
  j.pitch = (uint32_t) t.width;
  return j;
}

// the host blob's copy of textures edited from device memory (qa_scene_download is the only reader of texels on the host)
int FetchDeviceTexels(qa_ctx *c)
{
  if (c->texOnDevice.empty()) return QA_OK;
  HIP_TRY(hipSetDevice(c->device));
  const qa_flat_header *h = reinterpret_cast<const qa_flat_header *>(c->hostBlob.data());
  for (uint32_t i : c->texOnDevice) {
    const qa_texture &t = QA_BLOB_PTR(qa_texture, c->hostBlob.data(), h->off_textures)[i];
    HIP_TRY(hipMemcpyAsync(c->hostBlob.data() + t.off_texels, c->dBlob + t.off_texels, 3 * (size_t) t.width * (size_t) t.height, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->texOnDevice.clear();
  return QA_OK;
}

extern "C" {

int qa_scene_edit_texels(qa_ctx *c, uint32_t texture, int x0, int y0, int x1, int y1, const uint8_t *rgb8, uint64_t row_stride_bytes)
{
  const qa_texture *tx;
  int rc = TexelArgs(c, texture, x0, y0, x1, y1, rgb8, row_stride_bytes, &tx);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = EditBegin(c)) != QA_OK) return rc;
  // Slices of at most kSlice bytes of the ring (a quarter of its smallest size: texels never make it grow): whole rows of the
  // rectangle, or pieces of a row longer than that.  A slice's rows are staged 4-byte aligned plus the offset of the slice's
  // first byte in the device blob, so that the kernel's dword path takes every row of a texture whose width is a multiple of 4
  const size_t kSlice = 64 * 1024;
  const uint32_t w = (uint32_t) (x1 - x0), h = (uint32_t) (y1 - y0);
  const uint32_t colsPer = std::min<uint32_t>(w, (uint32_t) (kSlice / 3) & ~3u);
  const size_t stageStride = (3 * (size_t) colsPer + 3) & ~(size_t) 3;
  const uint32_t rowsPer = colsPer == w ? (uint32_t) std::max<size_t>(1, kSlice / stageStride) : 1u;
  qa::TexelJob j = JobOf(c, texture, *tx);
  unsigned char *hostTexels = c->hostBlob.data() + tx->off_texels;
  for (uint32_t r0 = 0; r0 < h; r0 += rowsPer)
    for (uint32_t c0 = 0; c0 < w; c0 += colsPer) {
      const uint32_t rows = std::min(rowsPer, h - r0), cols = std::min(colsPer, w - c0);
      const size_t q0 = (size_t) (y0 + r0) * j.pitch + (size_t) x0 + c0;
      const size_t lead = reinterpret_cast<uintptr_t>(j.bytes + 3 * q0) & 3u;
      unsigned char *stage = nullptr;
      if ((rc = EditStageReserve(c, lead + rows * stageStride, &stage)) != QA_OK) return rc;
      for (uint32_t r = 0; r < rows; ++r) {
        const uint8_t *from = rgb8 + (size_t) (r0 + r) * row_stride_bytes + 3 * (size_t) c0;
        memcpy(stage + lead + r * stageStride, from, 3 * (size_t) cols);
        memcpy(hostTexels + 3 * (q0 + (size_t) r * j.pitch), from, 3 * (size_t) cols);
      }
      void *dev = nullptr;
      HIP_TRY(hipHostGetDevicePointer(&dev, stage, 0));
      j.src = static_cast<const uint8_t *>(dev) + lead;
      j.srcStride = stageStride;
      j.x0 = (uint32_t) x0 + c0; j.y0 = (uint32_t) y0 + r0; j.w = cols; j.h = rows;
      if ((rc = Tabulate(c, j)) != QA_OK) return rc;
      HIP_TRY(c->lastEdit.Record(c->stream));   // (the ring's next wrap waits for this slice's kernel)
      c->statBytesCopied += 3 * (uint64_t) cols * rows;
    }
  return EditEnd(c, false);
}

int qa_scene_edit_texels_device(qa_ctx *c, uint32_t texture, int x0, int y0, int x1, int y1, const uint8_t *d_rgb8, uint64_t row_stride_bytes,
                                void *hip_stream)
{
  const qa_texture *tx;
  int rc = TexelArgs(c, texture, x0, y0, x1, y1, d_rgb8, row_stride_bytes, &tx);
  if (rc != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = EditBegin(c)) != QA_OK) return rc;
  hipStream_t theirs = static_cast<hipStream_t>(hip_stream);
  if (theirs && theirs != c->stream) {   // the source is ready once their stream gets here
    HIP_TRY(c->texSource.Record(theirs));
    HIP_TRY(c->texSource.WaitOn(c->stream));
  }
  qa::TexelJob j = JobOf(c, texture, *tx);
  j.src = d_rgb8;
  j.srcStride = row_stride_bytes;
  j.x0 = (uint32_t) x0; j.y0 = (uint32_t) y0; j.w = (uint32_t) (x1 - x0); j.h = (uint32_t) (y1 - y0);
  if ((rc = Tabulate(c, j)) != QA_OK) return rc;
  HIP_TRY(c->lastEdit.Record(c->stream));
  if (theirs) HIP_TRY(c->lastEdit.WaitOn(theirs));   // ... and may be overwritten on it from here on
  if (std::find(c->texOnDevice.begin(), c->texOnDevice.end(), texture) == c->texOnDevice.end()) c->texOnDevice.push_back(texture);
  return EditEnd(c, false);
}

// the same source on the CPU (no GPU, no context): w * h entries of 4 floats
int qa_test_texels_host(const uint8_t *rgb8, int w, int h, uint64_t stride, float *out4)
{
  if (!rgb8 || !out4 || w <= 0 || h <= 0 || stride < 3ull * (uint64_t) w) return QA_EINVAL;
  qa::texelsTabulateHost(rgb8, (size_t) w, (size_t) h, (size_t) stride, out4);
  return QA_OK;
}

}  // extern "C"
