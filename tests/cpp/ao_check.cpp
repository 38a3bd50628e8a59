// ao_check.cpp — the host half of qaray_amd/csrc/hip/qa_ao_dev.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_ao_host.py builds and runs it).  Every buffer lives on the heap at exactly the size the loops may touch, so a step
// outside one is reported.  Checked here, over batches of 1, 17, 4096 and 65 536 rays, seeds 0, 0xFFFFFFFF and the default, streams
// and counters at both ends of 32 bits:
//   - the properties the header's comment states: the signed unit is in [-1, 1) and a multiple of 2^-23; a sphere point has unit
//     length to 3e-7 or is the fallback (0, 0, 1); a direction has unit length to 4e-7 and lies on the normal's side; the fallback
//     and the l2 <= 1e-6 branch through the outer step given s directly; the facing normal never points along the ray; the sample
//     clamp, the radius clamp and the ao value at their edges,
//   - the generator against a second chain written out in place (the same integer and fp32 operations: equal bits).
// Prints "ao_check: clean" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "qa_ao_dev.h"

using namespace qa;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

static uint32_t Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Lcg {   // (a fixed stream: the program's output does not depend on the C library's rand)
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 32); }
  float unit() { return (float) (next() & 0xFFFFFF) / 16777216.0f; }
};

static uint32_t MixOut(uint32_t h)
{
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// the specification's chain written out: -> d, and whether the fallback was taken
static void DirectionOut(uint32_t seed, uint32_t stream, uint32_t c, const float n[3], float d[3], bool &fallback)
{
  const uint32_t key = MixOut(seed ^ stream * 0x9E3779B9u);
  const uint32_t kr = MixOut(key ^ MixOut(c + 0x632BE5ABu));
  float s[3] = {0.f, 0.f, 1.f};
  fallback = true;
  for (uint32_t a = 0; a < 8 && fallback; ++a) {
    const float x0 = (float) (MixOut(kr ^ (2u * a + 1u) * 0x9E3779B9u) >> 8) * 1.1920928955078125e-07f - 1.f;
    const float x1 = (float) (MixOut(kr ^ (2u * a + 2u) * 0x9E3779B9u) >> 8) * 1.1920928955078125e-07f - 1.f;
    const float q = x0 * x0 + x1 * x1;
    if (q < 1.f) {
      const float r = sqrtf(1.f - q);
      s[0] = 2.f * x0 * r; s[1] = 2.f * x1 * r; s[2] = 1.f - 2.f * q;
      fallback = false;
    }
  }
  const float v[3] = {n[0] + s[0], n[1] + s[1], n[2] + s[2]};
  const float l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (l2 > 1e-6f) {
    const float l = sqrtf(l2);
    for (int k = 0; k < 3; ++k) d[k] = v[k] / l;
  } else {
    for (int k = 0; k < 3; ++k) d[k] = n[k];
  }
}

static void CheckBatch(size_t count, uint32_t seed)
{
  std::unique_ptr<uint32_t[]> stream(new uint32_t[count]), c(new uint32_t[count]);
  std::unique_ptr<float[]> n(new float[3 * count]), d(new float[3 * count]), faced(new float[3 * count]);
  Lcg rng(count * 31 + seed);
  for (size_t i = 0; i < count; ++i) {
    stream[i] = i % 7 == 0 ? 0xFFFFFFFFu - (uint32_t) i : i % 7 == 1 ? (uint32_t) i : rng.next();
    c[i] = i % 5 == 0 ? 0xFFFFFFFFu - (uint32_t) i : i % 5 == 1 ? (uint32_t) i : rng.next();
    double v[3], l = 0;
    do {
      l = 0;
      for (int k = 0; k < 3; ++k) { v[k] = 2.0 * rng.unit() - 1.0; l += v[k] * v[k]; }
    } while (l < 1e-3 || l > 1.0);
    for (int k = 0; k < 3; ++k) n[3 * i + k] = (float) (v[k] / std::sqrt(l));
  }
  for (size_t i = 0; i < count; ++i) {
    const AoVec nn = {n[3 * i], n[3 * i + 1], n[3 * i + 2]};
    const AoVec v = aoDirection(aoKey(seed, stream[i]), c[i], nn);
    d[3 * i] = v.x; d[3 * i + 1] = v.y; d[3 * i + 2] = v.z;
    const AoVec f = aoFaceNormal(nn, v);   // (v as a ray's direction: it lies on n's side, so the normal is turned)
    faced[3 * i] = f.x; faced[3 * i + 1] = f.y; faced[3 * i + 2] = f.z;
  }
  for (size_t i = 0; i < count; ++i) {
    float ref[3];
    bool fb, fb2;
    DirectionOut(seed, stream[i], c[i], &n[3 * i], ref, fb);
    CHECK(Bits(ref[0]) == Bits(d[3 * i]) && Bits(ref[1]) == Bits(d[3 * i + 1]) && Bits(ref[2]) == Bits(d[3 * i + 2]), "ray %zu seed %u: the chain", i, seed);
    const AoVec s = aoSphere(aoRayKey(aoKey(seed, stream[i]), c[i]), fb2);
    CHECK(fb == fb2, "ray %zu: fallback flag", i);
    const double sl = std::sqrt((double) s.x * s.x + (double) s.y * s.y + (double) s.z * s.z);
    CHECK(std::fabs(sl - 1.0) < 3e-7, "ray %zu: sphere point length %.9g", i, sl);
    if (fb2) CHECK(s.x == 0.f && s.y == 0.f && s.z == 1.f, "ray %zu: the fallback point", i);
    const double dl = std::sqrt((double) d[3 * i] * d[3 * i] + (double) d[3 * i + 1] * d[3 * i + 1] + (double) d[3 * i + 2] * d[3 * i + 2]);
    const double dn = (double) d[3 * i] * n[3 * i] + (double) d[3 * i + 1] * n[3 * i + 1] + (double) d[3 * i + 2] * n[3 * i + 2];
    CHECK(std::fabs(dl - 1.0) < 4e-7, "ray %zu: direction length %.9g", i, dl);
    CHECK(dn >= -1e-6, "ray %zu: below the surface, d.n = %.9g", i, dn);
    const double fd = (double) faced[3 * i] * d[3 * i] + (double) faced[3 * i + 1] * d[3 * i + 1] + (double) faced[3 * i + 2] * d[3 * i + 2];
    CHECK(fd <= 1e-6, "ray %zu: the facing normal points along the ray, %.9g", i, fd);
  }
}

int main()
{
  const size_t sizes[4] = {1, 17, 4096, 65536};
  const uint32_t seeds[3] = {0u, 0xFFFFFFFFu, 0x51A7A7u};
  for (size_t n : sizes)
    for (uint32_t s : seeds) CheckBatch(n, s);

  // the signed unit: the ends of the word, exactness
  CHECK(aoSigned(0u) == -1.f && aoSigned(0xFFu) == -1.f && aoSigned(0x100u) == -1.f + 1.1920928955078125e-07f, "signed unit: low end");
  CHECK(aoSigned(0xFFFFFFFFu) == 1.f - 1.1920928955078125e-07f && aoSigned(0x80000000u) == 0.f, "signed unit: high end and middle");

  // the outer step given s directly: the fallback point, and the sum too short to normalise
  const AoVec up = {0.f, 0.f, 1.f}, down = {0.f, 0.f, -1.f}, x = {1.f, 0.f, 0.f};
  AoVec d = aoDirectionFrom(up, up);
  CHECK(d.x == 0.f && d.y == 0.f && d.z == 1.f, "n + s along n");
  d = aoDirectionFrom(down, up);
  CHECK(d.x == 0.f && d.y == 0.f && d.z == -1.f, "s = -n: d = n");
  const AoVec nearDown = {9.9e-4f, 0.f, 1.f};
  d = aoDirectionFrom(down, nearDown);
  CHECK(Bits(d.x) == Bits(down.x) && Bits(d.z) == Bits(down.z), "l2 below 1e-6: d = n");
  const AoVec offDown = {1.1e-3f, 0.f, 1.f};
  d = aoDirectionFrom(down, offDown);
  CHECK(d.x == 1.f && d.z == 0.f, "l2 above 1e-6: normalised");
  d = aoDirectionFrom(x, up);
  CHECK(Bits(d.x) == Bits(1.f / sqrtf(2.f)) && Bits(d.z) == Bits(d.x) && d.y == 0.f, "the fallback about x");

  // the facing normal: the dot's sign, zero included
  AoVec f = aoFaceNormal(up, down);
  CHECK(f.z == 1.f, "facing: against the ray stays");
  f = aoFaceNormal(up, up);
  CHECK(f.z == -1.f, "facing: along the ray is turned");
  f = aoFaceNormal(up, x);
  CHECK(f.z == 1.f && Bits(f.x) == 0u, "facing: perpendicular stays, bits and all");

  // void points, the clamps, the value
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const AoVec zero = {0.f, 0.f, 0.f}, bad1 = {nan, 0.f, 0.f}, bad2 = {0.f, -inf, 0.f};
  CHECK(!aoVoidPoint(zero, up) && aoVoidPoint(zero, zero) && aoVoidPoint(bad1, up) && aoVoidPoint(up, bad2) && aoVoidPoint(bad2, up), "void points");
  CHECK(aoSamples(7, 0, 5) == 5 && aoSamples(7, 4, 5) == 3 && aoSamples(4, 4, 5) == 0 && aoSamples(2, 4, 5) == 0 && aoSamples(0, 0, 5) == 0, "the sample clamp");
  CHECK(aoTmax(inf) == 1e30f && aoTmax(3.f) == 3.f && aoTmax(2e30f) == 1e30f, "the radius clamp");
  CHECK(aoValue(0, 0) == 1.f && aoValue(0, 8) == 0.f && aoValue(8, 8) == 1.f && Bits(aoValue(1, 3)) == Bits(1.f / 3.f), "the ao value");

  if (g_fail) { printf("ao_check: %d failure(s)\n", g_fail); return 1; }
  printf("ao_check: clean\n");
  return 0;
}
