// qa_idmatte_dev.h — the id matte of a pixel: which nodes (or materials) the camera rays of ALL its samples meet and how many samples
// each takes, ranked, and the coverage plane of a chosen set of ids made from it.  This comment is the specification;
// tests/idmatte_util.py restates it in numpy and tests/test_idmatte_host.py holds the host build of the functions below to that
// restatement exactly.  Everything here is integer arithmetic but the one division of the select product.
//
// THE SAMPLES are qa_matte_dev.h's, word for word: sample s of pixel (px, py) is the camera ray qa_kernel.h section B builds for
// sample index s (the Halton pair of s added to (px, py), the point (A + U x) + V y of the image plane, the direction normalised, in
// textured scenes the two differential rays), cast with traceClosest<RES, TEX, false>.  A camera with depth of field (dof > 0.1) is
// refused (QA_EUNSUPPORTED) and nothing is written.  A pixel takes samples 0 .. n - 1: n = spp for every pixel, or, with an ns plane,
// n = min(ns[q], spp); a progressive frame gives the samples each pixel holds now, by the state-word rule of qa_matte.
//
// THE KEY OF A HIT, by `key`:
//   QA_IDMATTE_NODE      word 0 of what qa_gbuffer writes to its ids plane for that ray: the hit's node index, >= 0.
//   QA_IDMATTE_MATERIAL  QA_GBUFFER_MATERIAL(word 1): the material index with the back-face bit cleared, >= 0; or the negative words
//                        of hits without a material as the header documents them, -1 (the node has none) and -2 (a multi-material
//                        mesh whose face names none), which the back-face bit leaves as they are.
// A miss has no key.  So a key is >= -2, and none can be QA_IDMATTE_EMPTY = INT32_MIN, the id of a free slot.
//
// THE TABLE.  A pixel has QA_IDMATTE_SLOTS = 8 slots of (id, count) and one `other` count, all free / 0 before sample 0.  Samples
// are taken in order; a sample that hits
//   - adds 1 to the slot that already holds its key, if one does;
//   - otherwise takes the first free slot, with count 1, if one is free;
//   - otherwise adds 1 to `other`.
// (A key that first appears when the table is full never enters it: every later sample of it goes to `other` too.)
// After the last sample the occupied slots are ordered by count descending, equal counts by id ascending; the free slots follow
// with id = QA_IDMATTE_EMPTY and count 0.  sum(counts) + other is the number of samples that hit; n = 0 gives empties and zeros.
//
// THE OUTPUTS, region-local and row-major: ids int32 (H, W, 8), counts uint32 (H, W, 8), other uint32 (H, W), samples uint32
// (H, W) = n.
//
// THE SELECT PRODUCT.  From ids, counts, samples and a list of m <= QA_IDMATTE_MAX_SELECT ids, one float per pixel:
// (float) c / (float) n, c the integer sum of the counts of the slots whose id is in the list (a slot counts once however often the
// list names its id), and 0 where n == 0.  The sum is in integers and there is one correctly rounded division, so the
// list of every id of a pixel whose `other` is 0 gives qa_matte's coverage bit for bit.  Its 8-bit grey picture is
// displayColorByte(value, false) per pixel: qa_display_dev.h's byte function, included here and not restated.
//
// Every function here is compiled for the host too: qa_test_idmatte_accumulate_host / qa_test_idmatte_select_host and the kernels
// of qa_idmatte.hip run the same source.
#pragma once
#include "qa_display_dev.h"
#include "qaray_hip.h"

namespace qa {

// What a lane carries through its sample loop: seventeen registers.  Slots fill from 0 upwards and are never given up, so the
// occupied ones always come first
struct IdMatteAcc {
  int32_t id[QA_IDMATTE_SLOTS];
  uint32_t count[QA_IDMATTE_SLOTS];
  uint32_t other;
};
__host__ __device__ __forceinline__ IdMatteAcc idMatteInit()
{
  IdMatteAcc a;
#pragma unroll
  for (int k = 0; k < QA_IDMATTE_SLOTS; ++k) {
    a.id[k] = QA_IDMATTE_EMPTY;
    a.count[k] = 0u;
  }
  a.other = 0u;
  return a;
}
// One sample.  No key is QA_IDMATTE_EMPTY and the free slots follow the occupied ones, so the first slot that holds the key or
// is free is the slot the rule names.  Unrolled, with constant indices: the table stays in registers
__host__ __device__ __forceinline__ void idMatteSample(IdMatteAcc &a, bool hit, int32_t key)
{
  bool open = hit;
#pragma unroll
  for (int k = 0; k < QA_IDMATTE_SLOTS; ++k) {
    const bool here = open && (a.id[k] == key || a.id[k] == QA_IDMATTE_EMPTY);
    a.id[k] = here ? key : a.id[k];
    a.count[k] += here ? 1u : 0u;
    open = open && !here;
  }
  a.other += open ? 1u : 0u;
}
// slot i before slot j: the larger count, then the smaller id (two free slots are equal and stay)
__host__ __device__ __forceinline__ void idMatteOrder(IdMatteAcc &a, int i, int j)
{
  const bool swap = a.count[j] > a.count[i] || (a.count[j] == a.count[i] && a.id[j] < a.id[i]);
  const int32_t idI = a.id[i], idJ = a.id[j];
  const uint32_t cI = a.count[i], cJ = a.count[j];
  a.id[i] = swap ? idJ : idI;
  a.id[j] = swap ? idI : idJ;
  a.count[i] = swap ? cJ : cI;
  a.count[j] = swap ? cI : cJ;
}
// The ranking: a fixed network of 19 exchanges in 6 layers that sorts any 8 values (tests/test_idmatte_host.py checks it over
// every 0/1 input, which is enough for a network of exchanges)
__host__ __device__ __forceinline__ void idMatteRank(IdMatteAcc &a)
{
  static_assert(QA_IDMATTE_SLOTS == 8, "the network below sorts eight slots");
  idMatteOrder(a, 0, 2); idMatteOrder(a, 1, 3); idMatteOrder(a, 4, 6); idMatteOrder(a, 5, 7);
  idMatteOrder(a, 0, 4); idMatteOrder(a, 1, 5); idMatteOrder(a, 2, 6); idMatteOrder(a, 3, 7);
  idMatteOrder(a, 0, 1); idMatteOrder(a, 2, 3); idMatteOrder(a, 4, 5); idMatteOrder(a, 6, 7);
  idMatteOrder(a, 2, 4); idMatteOrder(a, 3, 5);
  idMatteOrder(a, 1, 4); idMatteOrder(a, 3, 6);
  idMatteOrder(a, 1, 2); idMatteOrder(a, 3, 4); idMatteOrder(a, 5, 6);
}
// the material key of a material word of the ids planes
__host__ __device__ __forceinline__ int32_t idMatteMaterialKey(int32_t word) { return QA_GBUFFER_MATERIAL(word); }

// The select product of one pixel: its eight slots, its sample count, the list
__host__ __device__ __forceinline__ float idMatteSelect(const int32_t *id, const uint32_t *count, uint32_t n, const int32_t *select, uint32_t m)
{
  bool in[QA_IDMATTE_SLOTS];
#pragma unroll
  for (int k = 0; k < QA_IDMATTE_SLOTS; ++k) in[k] = false;
  for (uint32_t j = 0; j < m; ++j) {
    const int32_t want = select[j];
#pragma unroll
    for (int k = 0; k < QA_IDMATTE_SLOTS; ++k) in[k] = in[k] || id[k] == want;
  }
  uint32_t c = 0u;
#pragma unroll
  for (int k = 0; k < QA_IDMATTE_SLOTS; ++k) c += in[k] ? count[k] : 0u;
  return n ? (float) c / (float) n : 0.f;
}

}  // namespace qa
