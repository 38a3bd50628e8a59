// tile_select_check.cpp — the host half of qaray_amd/csrc/hip/qa_prog_error_dev.h under a plain C++ compiler, for AddressSanitizer
// and UBSan (tests/test_progressive_tiles_host.py builds and runs it): the selection of a noisiest-first pass against a stable sort,
// and the error map of state slabs whose edge tiles reach beyond the region, on heap buffers of exactly the sizes the calls are given.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "qa_prog_error_dev.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t Next()
{
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (uint32_t) (g_rng >> 32);
}

static int CheckSelect(uint32_t tiles, uint32_t target, uint32_t maxTiles, float minError)
{
  static const float kValues[] = {0.f, 1e-45f, 1e-12f, 3e-7f, 0.001f, 0.5f, 1.f, 7.5f, 3e38f, std::numeric_limits<float>::infinity()};
  std::vector<float> error(tiles);
  std::vector<uint32_t> level(tiles);
  for (uint32_t t = 0; t < tiles; ++t) {
    error[t] = (Next() & 3u) ? kValues[Next() % 10u] : (float) (Next() & 0xFFFFu) * 1e-6f;
    if (Next() % 97u == 0) error[t] = std::numeric_limits<float>::quiet_NaN();
    level[t] = 4u * (Next() % 4u);
  }
  std::vector<uint8_t> mask(tiles, 0xAA);
  uint64_t info[4];
  qa::progSelectHost(error.data(), level.data(), tiles, target, maxTiles, minError, mask.data(), info);
  std::vector<uint32_t> cand;
  for (uint32_t t = 0; t < tiles; ++t)
    if (level[t] < target && error[t] > minError) cand.push_back(t);
  std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return error[a] > error[b]; });
  const size_t take = (maxTiles == 0 || maxTiles > cand.size()) ? cand.size() : maxTiles;
  std::vector<uint8_t> want(tiles, 0);
  for (size_t i = 0; i < take; ++i) want[cand[i]] = 1;
  int bad = want != mask || info[0] != take || info[1] != cand.size();
  if (take) {
    uint32_t cut;
    std::memcpy(&cut, &error[cand[take - 1]], 4);
    bad |= info[2] != cut;
  } else bad |= info[2] != 0;
  if (bad) std::printf("select: tiles %u target %u max %u min %g: MISMATCH\n", tiles, target, maxTiles, (double) minError);
  return bad;
}

static int CheckError(uint32_t w, uint32_t h)
{
  std::vector<uint32_t> state((size_t) w * h * 8);
  for (size_t q = 0; q < (size_t) w * h; ++q) {
    for (int k = 0; k < 8; ++k) state[8 * q + k] = Next();
    state[8 * q + 1] = (Next() % 5u == 0) ? 0x80000000u : Next() % 41u;
    for (int k = 5; k < 8; ++k) {
      const float v = (Next() % 13u == 0) ? std::numeric_limits<float>::quiet_NaN() : (float) (Next() & 0xFFFFu) * 1e-6f;
      std::memcpy(&state[8 * q + k], &v, 4);
    }
  }
  const uint32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
  int bad = 0;
  for (uint32_t t = 0; t < tx * ty; ++t) {
    float a[64];
    double sum = 0;
    bool inf = false;
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t x = (t % tx) * 8 + (l & 7), y = (t / tx) * 8 + (l >> 3);
      const bool inside = x < w && y < h;
      const uint32_t *st = inside ? &state[8 * ((size_t) y * w + x)] : nullptr;
      a[l] = qa::progSlotValue(inside, inside ? st[1] : 0u, inside ? st[5] : 0u, inside ? st[6] : 0u, inside ? st[7] : 0u);
      bad |= !(a[l] >= 0.f);
      inf |= std::isinf(a[l]);
      sum += a[l];
    }
    const float e = qa::progTileSum(a);
    bad |= !(e >= 0.f) || std::isinf(e) != inf || (!inf && std::fabs((double) e - sum / 64) > 1e-5 * (sum / 64) + 1e-30);
  }
  if (bad) std::printf("error map %u x %u: MISMATCH\n", w, h);
  return bad;
}

int main()
{
  int bad = 0;
  const float inf = std::numeric_limits<float>::infinity();
  for (uint32_t tiles : {1u, 2u, 63u, 64u, 65u, 700u, 5000u})
    for (uint32_t target : {0u, 4u, 8u, 100u})
      for (uint32_t maxTiles : {0u, 1u, 2u, 17u, tiles / 2u, tiles, tiles + 1u, 0xFFFFFFFFu})
        for (float minError : {0.f, 1e-6f, 0.5f, 3e38f, inf}) bad |= CheckSelect(tiles, target, maxTiles, minError);
  for (uint32_t w : {1u, 8u, 9u, 40u})
    for (uint32_t h : {1u, 7u, 9u, 28u}) bad |= CheckError(w, h);
  std::printf(bad ? "tile_select_check: FAILED\n" : "tile_select_check: clean\n");
  return bad;
}
