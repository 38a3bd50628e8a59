// reflprobe_check.cpp — the host half of qaray_amd/csrc/hip/qa_reflprobe_dev.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_reflprobe_host.py builds and runs it).  Every buffer lives on the heap at exactly the size the loops may touch, so a
// step outside one is reported.  Checked here:
//   - the layout at every (m, L): offsets ascend by 6 r^2, T is their end, the squarings are 2 (lg - l) - 1 floored at 0;
//   - the prefilter at m = 1, 2, 4, 8, 16 and, at L = 2, 32 - with NaN, inf, -0 and denormal texels among the source: a constant
//     cube stays constant within 1e-5, zeros stay +0, every output of a finite positive cube lies within its source's range;
//   - the lookup at every level of chains of m = 1 .. 16: texel-centre directions answer their texel, directions on axes, edges and
//     corners, just inside the face edges, huge, tiny, zero and not finite, lambda at, between, outside the levels and not finite,
//     indices clamped at both ends of int32: every tap stays inside the chain's T texels;
//   - the grid lookup at counts (1,1,1), (2,1,3), (4,2,2): points on the probes (that probe's answer, bit for bit), outside on every
//     side, not finite.
// Prints "reflprobe_check: clean" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "qa_reflprobe_dev.h"

using namespace qa;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

static uint32_t Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static const float kInf = std::numeric_limits<float>::infinity(), kNan = std::numeric_limits<float>::quiet_NaN();

struct Lcg {   // (a fixed stream: the program's output does not depend on the C library's rand)
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 32); }
  float unit() { return (float) (next() & 0xFFFFFF) / 16777216.0f; }
};

static void CheckLayout()
{
  for (int m = 1; m <= 128; m *= 2) {
    const int lg = reflLog2(m);
    CHECK(lg >= 0 && (1 << lg) == m, "m %d", m);
    uint32_t off = 0;
    for (int l = 0; l <= lg + 1; ++l) {
      CHECK(reflOffset((uint32_t) m, l) == off, "m %d l %d", m, l);
      if (l <= lg) off += 6u * (m >> l) * (m >> l);
      if (l >= 1 && l <= lg) CHECK((int) reflSquarings(lg, l) == (2 * (lg - l) - 1 > 0 ? 2 * (lg - l) - 1 : 0), "m %d l %d", m, l);
    }
  }
  const int bad[] = {0, -1, 3, 6, 12, 100, 256};
  for (int m : bad) CHECK(reflLog2(m) < 0, "m %d", m);
  CHECK(reflSquarings(4, 1) == 5 && reflSquarings(4, 2) == 3 && reflSquarings(4, 3) == 1 && reflSquarings(4, 4) == 0, "m = 16");
}

// one probe's chain of L levels from cube [K][3] into a buffer of exactly T texels
static std::unique_ptr<float[]> Prefilter(int m, int L, const float *cube)
{
  const int lg = reflLog2(m);
  const uint32_t K = 6u * m * m, T = reflOffset((uint32_t) m, L);
  std::unique_ptr<ProbeDir[]> rec(new ProbeDir[K]);
  for (uint32_t k = 0; k < K; ++k) rec[k] = probeDirection((uint32_t) m, k, .5f, .5f);
  std::unique_ptr<float[]> chain(new float[3 * (size_t) T]);
  memcpy(chain.get(), cube, 12 * (size_t) K);
  for (int l = 1; l < L; ++l)
    for (uint32_t k = 0; k < 6u * (m >> l) * (m >> l); ++k)
      reflPrefilterTexel((uint32_t) m, lg, l, k, rec.get(), cube, chain.get() + 3 * ((size_t) reflOffset((uint32_t) m, l) + k));
  return chain;
}

static void CheckPrefilter(int m, int L)
{
  const uint32_t K = 6u * m * m, T = reflOffset((uint32_t) m, L);
  std::unique_ptr<float[]> cube(new float[3 * (size_t) K]);
  Lcg rng(m * 17 + L);
  // a finite positive cube: every output is a weighted mean of its source
  float lo = 1e30f, hi = 0.f;
  for (uint32_t i = 0; i < 3 * K; ++i) { cube[i] = 0.25f + 3.f * rng.unit(); lo = fminf(lo, cube[i]); hi = fmaxf(hi, cube[i]); }
  std::unique_ptr<float[]> chain = Prefilter(m, L, cube.get());
  for (uint32_t i = 0; i < 3 * K; ++i) CHECK(Bits(chain[i]) == Bits(cube[i]), "m %d L %d: level 0 texel %u", m, L, i);
  for (uint32_t i = 3 * K; i < 3 * T; ++i) CHECK(chain[i] >= lo * (1.f - 1e-5f) && chain[i] <= hi * (1.f + 1e-5f), "m %d L %d: %u = %g", m, L, i, chain[i]);
  // a constant cube and a zero cube
  for (uint32_t i = 0; i < 3 * K; ++i) cube[i] = 1.7f;
  chain = Prefilter(m, L, cube.get());
  for (uint32_t i = 0; i < 3 * T; ++i) CHECK(fabsf(chain[i] / 1.7f - 1.f) <= 1e-5f, "m %d L %d: constant, %u = %g", m, L, i, chain[i]);
  for (uint32_t i = 0; i < 3 * K; ++i) cube[i] = 0.f;
  chain = Prefilter(m, L, cube.get());
  for (uint32_t i = 0; i < 3 * T; ++i) CHECK(Bits(chain[i]) == 0u, "m %d L %d: zero, %u", m, L, i);
  // special texels: nothing is read or written outside, whatever the values
  const float special[8] = {kNan, kInf, -kInf, -0.f, 1e-42f, -1e-45f, 3e38f, 0.f};
  for (uint32_t i = 0; i < 3 * K; ++i) cube[i] = rng.unit();
  for (uint32_t i = 0; i < 8; ++i) cube[(i * 11u) % (3 * K)] = special[i];
  chain = Prefilter(m, L, cube.get());
  CHECK(std::isnan(chain[0]), "the NaN texel is copied");
}

static void CheckLookup(int m, int L)
{
  const uint32_t T = reflOffset((uint32_t) m, L);
  const int probes = 3;
  std::unique_ptr<float[]> chain(new float[3 * (size_t) T * probes]);
  Lcg rng(m * 29 + L);
  for (size_t i = 0; i < 3 * (size_t) T * probes; ++i) chain[i] = rng.unit();
  float out[3];
  // a texel centre at its level answers that texel
  for (int l = 0; l < L; ++l) {
    const uint32_t r = (uint32_t) m >> l;
    for (uint32_t k = 0; k < 6u * r * r; ++k) {
      const ProbeDir d = probeDirection(r, k, .5f, .5f);
      reflLookup(chain.get(), (uint32_t) m, L, d.d, (float) l, out);
      const float *want = chain.get() + 3 * ((size_t) reflOffset((uint32_t) m, l) + k);
      for (int ch = 0; ch < 3; ++ch) CHECK(fabsf(out[ch] - want[ch]) <= 1e-5f, "m %d L %d l %d k %u: %g vs %g", m, L, l, k, out[ch], want[ch]);
    }
  }
  // the edge directions and levels: inside the chain, finite for finite texels, zero for what is void
  const float in = std::nextafter(1.f, 0.f);
  const float comps[] = {0.f, -0.f, 1.f, -1.f, in, -in, 0.25f, 3e38f, -3e38f, 1e-45f, -1e-40f, kInf, -kInf, kNan};
  const float lams[] = {0.f, -0.f, 0.5f, 1.f, (float) (L - 1), (float) L - 0.5f, (float) L, -2.f, 1e30f, kInf, -kInf, kNan};
  const int nc = sizeof(comps) / sizeof(comps[0]);
  for (int a = 0; a < nc; ++a)
    for (int b = 0; b < nc; ++b)
      for (int c = 0; c < nc; ++c)
        for (float lam : lams) {
          const float R[3] = {comps[a], comps[b], comps[c]};
          const int64_t q = probeIndex((int64_t) (a * 7 + b * 3 + c) - 5, probes);
          reflLookup(chain.get() + 3 * (size_t) T * (size_t) q, (uint32_t) m, L, R, lam, out);
          const bool isVoid = !(std::isfinite(R[0]) && std::isfinite(R[1]) && std::isfinite(R[2])) || (R[0] == 0.f && R[1] == 0.f && R[2] == 0.f) || std::isnan(lam);
          for (int ch = 0; ch < 3; ++ch) {
            CHECK(std::isfinite(out[ch]) && out[ch] >= 0.f && out[ch] <= 1.f + 1e-6f, "m %d L %d: (%g %g %g) at %g -> %g", m, L, R[0], R[1], R[2], lam, out[ch]);
            if (isVoid) CHECK(Bits(out[ch]) == 0u, "void (%g %g %g) at %g", R[0], R[1], R[2], lam);
          }
        }
  CHECK(probeIndex(INT32_MIN, probes) == 0 && probeIndex(INT32_MAX, probes) == probes - 1, "the index clamp");
  // the tie rule: the lowest axis wins
  float u, v;
  const float xy[3] = {1.f, 1.f, 1.f}, yz[3] = {0.5f, -1.f, 1.f}, nx[3] = {-2.f, 2.f, 0.f};
  CHECK(reflFace(xy, u, v) == 0 && u == 1.f && v == 1.f, "(1, 1, 1) lies on +x");
  CHECK(reflFace(yz, u, v) == 3 && u == 1.f && v == -0.5f, "(0.5, -1, 1) lies on -y");
  CHECK(reflFace(nx, u, v) == 1 && u == 1.f && v == -0.f, "(-2, 2, 0) lies on -x");
}

static void CheckGrid(const int32_t cn[3])
{
  const int m = 4, L = 3;
  const uint32_t T = reflOffset((uint32_t) m, L);
  const size_t probes = (size_t) cn[0] * cn[1] * cn[2];
  std::unique_ptr<float[]> chain(new float[3 * (size_t) T * probes]);
  Lcg rng(cn[0] * 100 + cn[1] * 10 + cn[2]);
  for (size_t i = 0; i < 3 * (size_t) T * probes; ++i) chain[i] = rng.unit();
  ProbeGrid G;
  const float origin[3] = {0.5f, -1.f, 0.25f}, spacing[3] = {1.f, 0.5f, 2.f};   // (dyadic: a probe's position is exact)
  CHECK(GridOk(origin, spacing, cn), "the grid");
  G = GridOf(origin, spacing, cn);
  float out[3], want[3];
  for (int iz = 0; iz < cn[2]; ++iz)
    for (int iy = 0; iy < cn[1]; ++iy)
      for (int ix = 0; ix < cn[0]; ++ix) {
        const float P[3] = {origin[0] + ix * spacing[0], origin[1] + iy * spacing[1], origin[2] + iz * spacing[2]};
        const float R[3] = {rng.unit() - 0.5f, rng.unit() - 0.5f, rng.unit() + 0.01f}, lam = 2.f * rng.unit();
        reflGridLookup(G, chain.get(), (uint32_t) m, L, P, R, lam, out);
        reflLookup(chain.get() + 3 * (size_t) T * (((size_t) iz * cn[1] + iy) * cn[0] + ix), (uint32_t) m, L, R, lam, want);
        for (int ch = 0; ch < 3; ++ch) CHECK(Bits(out[ch]) == Bits(want[ch]), "grid %d x %d x %d: on probe (%d, %d, %d)", cn[0], cn[1], cn[2], ix, iy, iz);
      }
  const float far[] = {1e30f, -1e30f, 3e38f, -3e38f, kInf, -kInf, kNan, 0.7f};
  for (float x : far)
    for (float y : far)
      for (float z : far) {
        const float P[3] = {x, y, z}, R[3] = {0.3f, -0.2f, 0.9f};
        reflGridLookup(G, chain.get(), (uint32_t) m, L, P, R, 1.5f, out);
        const bool isVoid = !(std::isfinite(x) && std::isfinite(y) && std::isfinite(z));
        for (int ch = 0; ch < 3; ++ch) {
          CHECK(std::isfinite(out[ch]) && out[ch] >= 0.f && out[ch] <= 1.f + 1e-6f, "grid: point (%g %g %g) -> %g", x, y, z, out[ch]);
          if (isVoid) CHECK(Bits(out[ch]) == 0u, "grid: a void point");
        }
      }
}

int main()
{
  CheckLayout();
  for (int m = 1; m <= 16; m *= 2)
    for (int L = 1; L <= reflLog2(m) + 1; ++L) {
      CheckPrefilter(m, L);
      CheckLookup(m, L);
    }
  CheckPrefilter(32, 2);
  const int32_t grids[3][3] = {{1, 1, 1}, {2, 1, 3}, {4, 2, 2}};
  for (const int32_t *cn : grids) CheckGrid(cn);
  if (g_fail) { printf("reflprobe_check: %d failure(s)\n", g_fail); return 1; }
  printf("reflprobe_check: clean\n");
  return 0;
}
