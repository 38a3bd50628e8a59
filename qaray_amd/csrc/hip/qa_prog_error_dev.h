// qa_prog_error_dev.h — a progressive frame's error estimate per 8x8 tile, and the rule by which a noisiest-first pass
// (qa_progressive_advance_adaptive) picks its tiles.  This comment is the specification; tests/progressive_tiles_util.py restates
// it in numpy and tests/test_progressive_tiles_host.py holds the host build of the functions below to that restatement bit for bit.
//
// THE ERROR MAP.  The frame's region is w x h pixels, cut into tx = (w + 7) / 8 by ty = (h + 7) / 8 tiles, tile t = row * tx + col,
// row-major from the region's top left corner.  Slot l (0 .. 63) of a tile is the pixel (col * 8 + l % 8, row * 8 + l / 8) of the
// region; its state is the 8 words at 8 * (y * w + x) of the frame's state slab: word 1 = samples taken n (bits 0 .. 30) | bit 31
// finished, words 5 .. 7 = the running sample variance of r, g, b as floats (words 0 and 2 .. 4 are not read).  A slot's value s:
//   outside the region (x >= w or y >= h), or finished ......................  s = 0
//   not finished, n < 2 .....................................................  s = +inf
//   not finished, n >= 2:  m = the largest of the three variances, NaN if any of them is a NaN;
//                          v = m / (float) n, one correctly rounded float division (the variance of the pixel's mean in its
//                          worst channel);  s = v where 0 <= v <= FLT_MAX (a -0 counts as +0), and s = +inf for every other v
//                          (NaN, +inf, negative)
// The tile's error is the sum of its 64 slot values times 1/64, the sum taken by halving: a[l] += a[l + 32] for l < 32, then
// a[l] += a[l + 16] for l < 16, then 8, 4, 2, 1; error = a[0] * 0.015625f.  Every addition is one float addition, nothing is
// contracted.  So the error is never negative and never a NaN; it is +inf where a live pixel has no estimate yet (or where the sum
// overflows), and +0 where every pixel of the tile is finished.
//
// THE SELECTION.  Given every tile's error and level, a target T, max_tiles K and min_error (not a NaN, not negative):
//   a tile is a CANDIDATE when level < T and error > min_error (so a NaN error is none);
//   C = the number of candidates, K' = C when K == 0 or K > C, else K;
//   the K' candidates that come first in this order are selected: greater error first (+inf first of all), equal errors by
//   ascending tile index.
// A candidate's error is positive, so errors compare as their bit patterns do as unsigned integers (the KEY).  The cut is found by
// a radix select on the key, 8 bits a round from the top: with `prefix` the bits decided so far and `remaining` the tiles still
// to admit (K' at first), a round counts the candidates whose decided bits equal the prefix by their next 8 bits (256 bins), walks
// the bins from 255 down to the first bin b at which the running count reaches `remaining`, subtracts the count of the bins above b
// from `remaining` and appends b to the prefix (progRadixPick).  After 4 rounds the prefix is the CUT key - the smallest selected
// key - and `remaining` the number of candidates with exactly that key to admit: the first by tile index (progAdmit).
// The info block: [0] K', [1] C, [2] the cut key (0 when K' == 0), [3] the largest key below +inf's among the candidates (0: none).
//
// Every function here is compiled for the host too (qa_test_tile_error_host, qa_test_tile_select_host) from the source the kernels
// of qa_progressive.hip use.
#pragma once
#include <cstdint>

namespace qa {

#define QA_PROG_INF_BITS 0x7F800000u
#if defined(__HIPCC__)
#define QA_PROG_FN __host__ __device__ __forceinline__
#else
#define QA_PROG_FN inline /* a plain C++ compiler: the host half alone (tests/cpp/tile_select_check.cpp) */
#endif
QA_PROG_FN uint32_t progBits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
QA_PROG_FN float progFloat(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
#define QA_PROG_BITS(f) progBits(f)
#define QA_PROG_FLOAT(u) progFloat(u)

// A slot's value from word 1 and words 5 .. 7 of its pixel's state; inside = false for a slot of an edge tile beyond the region
QA_PROG_FN float progSlotValue(bool inside, uint32_t w1, uint32_t vx, uint32_t vy, uint32_t vz)
{
  if (!inside || (w1 & 0x80000000u)) return 0.f;
  const float inf = QA_PROG_FLOAT(QA_PROG_INF_BITS);
  if (w1 < 2u) return inf;
  const float x = QA_PROG_FLOAT(vx), y = QA_PROG_FLOAT(vy), z = QA_PROG_FLOAT(vz);
  if (x != x || y != y || z != z) return inf;
  float m = x;
  if (y > m) m = y;
  if (z > m) m = z;
  const float v = m / (float) w1;
  if (!(v >= 0.f && v <= 3.402823466e+38f)) return inf;
  return v > 0.f ? v : 0.f;
}

// The host's tile: a[64] holds the slot values and is used up
QA_PROG_FN float progTileSum(float *a)
{
  for (int half = 32; half >= 1; half >>= 1)
    for (int l = 0; l < half; ++l) a[l] = a[l] + a[l + half];
  return a[0] * 0.015625f;
}

QA_PROG_FN bool progCandidate(float error, uint32_t level, uint32_t target, float minError) { return level < target && error > minError; }

// K' of C candidates
QA_PROG_FN uint32_t progTake(uint32_t candidates, uint32_t maxTiles) { return (maxTiles == 0u || maxTiles > candidates) ? candidates : maxTiles; }

// Does `key` belong to this round's count?  shift = 24, 16, 8, 0: the bits above shift + 8 are decided
QA_PROG_FN bool progRadixMatch(uint32_t key, uint32_t prefix, uint32_t shift)
{
  return shift == 24u || (key >> (shift + 8u)) == (prefix >> (shift + 8u));
}

// One round's decision from its 256 bins (remaining >= 1 and at most the bins' total)
QA_PROG_FN void progRadixPick(const uint32_t *hist, uint32_t shift, uint32_t &prefix, uint32_t &remaining)
{
  uint32_t above = 0;
  int b = 255;
  for (; b > 0; --b) {
    if (above + hist[b] >= remaining) break;
    above += hist[b];
  }
  remaining -= above;
  prefix |= (uint32_t) b << shift;
}

// Is a candidate selected?  tieRank: how many candidates of lower tile index have exactly the cut key
QA_PROG_FN bool progAdmit(uint32_t key, uint32_t cut, uint32_t ties, uint32_t tieRank) { return key > cut || (key == cut && tieRank < ties); }

// The selection on the host, as the kernel qa_prog_adaptive_mask makes it.  mask: one byte per tile (1 selected)
inline void progSelectHost(const float *error, const uint32_t *level, uint32_t tiles, uint32_t target, uint32_t maxTiles, float minError, uint8_t *mask,
                           uint64_t info[4])
{
  uint32_t cand = 0, top = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    mask[t] = 0;
    if (!progCandidate(error[t], level[t], target, minError)) continue;
    ++cand;
    const uint32_t key = QA_PROG_BITS(error[t]);
    if (key < QA_PROG_INF_BITS && key > top) top = key;
  }
  const uint32_t take = progTake(cand, maxTiles);
  info[0] = take; info[1] = cand; info[2] = 0; info[3] = top;
  if (!take) return;
  uint32_t prefix = 0, remaining = take;
  for (uint32_t shift = 24u;; shift -= 8u) {
    uint32_t hist[256] = {};
    for (uint32_t t = 0; t < tiles; ++t)
      if (progCandidate(error[t], level[t], target, minError) && progRadixMatch(QA_PROG_BITS(error[t]), prefix, shift)) ++hist[(QA_PROG_BITS(error[t]) >> shift) & 255u];
    progRadixPick(hist, shift, prefix, remaining);
    if (shift == 0u) break;
  }
  info[2] = prefix;
  uint32_t rank = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    if (!progCandidate(error[t], level[t], target, minError)) continue;
    const uint32_t key = QA_PROG_BITS(error[t]);
    mask[t] = progAdmit(key, prefix, remaining, rank) ? 1 : 0;
    if (key == prefix) ++rank;
  }
}

}  // namespace qa
