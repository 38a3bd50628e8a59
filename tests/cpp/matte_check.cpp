// matte_check.cpp — the host half of qaray_amd/csrc/hip/qa_matte_dev.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_matte_host.py builds and runs it).  Every buffer lives on the heap at exactly the size the functions may touch, so a
// step outside one is reported.  Checked here, over frames of 1x1, 17x13 and 33x35 pixels with the edge cases of the specification
// planted in them (a in {0, 1/5, 1}, ns == 0, rgb an ulp below the backdrop, NaN and infinite components) and over sample runs of
// n in 1, 2, 5, 64, 2048 with the five hit patterns:
//   - the properties the header's comment states (ns == 0 -> four zero bytes; a == 1 over a zero backdrop -> displayColorByte of the
//     colour itself; alpha = displayColorByte(a, false); NaN -> byte 0; one sample -> the value itself; no hit -> normal 0 and
//     backdrop == albedo; all hit -> backdrop 0; coverage = hits / n),
//   - the running mean against a second loop written out in place (the same fp32 operations: equal bits).
// Prints "matte_check: clean" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "qa_matte_dev.h"

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
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); }
  float unit() { return (float) (next() & 0xFFFFFF) / 16777216.0f; }
};

static void CheckFrame(int w, int h, bool srgb)
{
  const size_t n = (size_t) w * h;
  std::unique_ptr<float[]> rgb(new float[3 * n]), back(new float[3 * n]), cov(new float[n]);
  std::unique_ptr<uint32_t[]> ns(new uint32_t[n]);
  std::unique_ptr<uint8_t[]> out(new uint8_t[4 * n]);
  Lcg rng((uint64_t) w * 1000 + h);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (size_t q = 0; q < n; ++q) {
    cov[q] = (float) (rng.next() % 6) / 5.0f;
    ns[q] = 1 + rng.next() % 5;
    for (int k = 0; k < 3; ++k) {
      rgb[3 * q + k] = 1.5f * rng.unit();
      back[3 * q + k] = rgb[3 * q + k] * rng.unit() * (1.f - cov[q]);
    }
    const int k = (int) (q % 3);
    switch (n > 1 ? q % 11 : 4) {
      case 0: cov[q] = 0.f; break;
      case 1: cov[q] = 1.f / 5.f; break;
      case 2: cov[q] = 1.f; break;
      case 3: ns[q] = 0; break;
      case 4: for (int j = 0; j < 3; ++j) back[3 * q + j] = std::nextafter(rgb[3 * q + j], inf); cov[q] = (q % 2) ? 1.f : 1.f / 5.f; break;
      case 5: rgb[3 * q + k] = nan; break;
      case 6: cov[q] = nan; break;
      case 7: rgb[3 * q + k] = inf; break;
      case 8: rgb[3 * q + k] = -inf; break;
      case 9: rgb[3 * q + k] = inf; back[3 * q + k] = inf; break;
      default: cov[q] = 1.f; for (int j = 0; j < 3; ++j) back[3 * q + j] = 0.f; break;
    }
  }
  for (size_t q = 0; q < n; ++q) {
    const MatteRgba o = matteRgbaEncode(rgb[3 * q], rgb[3 * q + 1], rgb[3 * q + 2], back[3 * q], back[3 * q + 1], back[3 * q + 2], cov[q], ns[q], srgb);
    out[4 * q] = o.r; out[4 * q + 1] = o.g; out[4 * q + 2] = o.b; out[4 * q + 3] = o.a;
  }
  for (size_t q = 0; q < n; ++q) {
    const uint8_t *o = &out[4 * q];
    const float a = cov[q];
    if (ns[q] == 0) { CHECK(!o[0] && !o[1] && !o[2] && !o[3], "pixel %zu: ns == 0", q); continue; }
    CHECK(o[3] == displayColorByte(a, false), "pixel %zu: alpha", q);
    if (std::isnan(a) || a == 0.f) CHECK(!o[0] && !o[1] && !o[2] && !o[3], "pixel %zu: no coverage", q);
    for (int k = 0; k < 3; ++k) {
      const float c = rgb[3 * q + k], b = back[3 * q + k];
      if (a == 1.f && b == 0.f) CHECK(o[k] == displayColorByte(c, srgb), "pixel %zu.%d: opaque over nothing", q, k);
      if (a > 0.f && (std::isnan(c) || std::isnan(c - b))) CHECK(o[k] == 0, "pixel %zu.%d: NaN", q, k);
      if (a > 0.f && c < b) CHECK(o[k] == 0, "pixel %zu.%d: below the backdrop", q, k);
      if (a > 0.f && c == inf && b != inf) CHECK(o[k] == 255, "pixel %zu.%d: +inf", q, k);
      if (a > 0.f && c == -inf) CHECK(o[k] == 0, "pixel %zu.%d: -inf", q, k);
    }
  }
}

static void CheckRun(uint32_t n, int pattern)
{
  std::unique_ptr<float[]> x(new float[3 * (size_t) n]), nrm(new float[3 * (size_t) n]);
  std::unique_ptr<uint8_t[]> hit(new uint8_t[n]);
  Lcg rng(n * 10 + (uint32_t) pattern);
  for (uint32_t s = 0; s < n; ++s) {
    hit[s] = pattern == 0 ? 1 : pattern == 1 ? 0 : pattern == 2 ? (s % 2 == 0) : pattern == 3 ? (s == 0) : (s == n - 1);
    for (int k = 0; k < 3; ++k) {
      x[3 * s + k] = (rng.next() % 7 == 0) ? 1e21f : (rng.next() % 5 == 0) ? 0.f : rng.unit();
      nrm[3 * s + k] = 2.f * rng.unit() - 1.f;
    }
  }
  MatteAcc acc = matteAccInit();
  for (uint32_t s = 0; s < n; ++s)
    matteAccSample(acc, s, hit[s] != 0, x[3 * s], x[3 * s + 1], x[3 * s + 2], nrm[3 * s], nrm[3 * s + 1], nrm[3 * s + 2]);
  // the specification's loops written out
  float a[3] = {0, 0, 0}, b[3] = {0, 0, 0}, m[3] = {0, 0, 0};
  uint32_t hits = 0;
  for (uint32_t s = 0; s < n; ++s) {
    if (hit[s]) ++hits;
    for (int k = 0; k < 3; ++k) {
      a[k] = a[k] + (x[3 * s + k] - a[k]) / (float) (s + 1);
      b[k] = b[k] + ((hit[s] ? 0.f : x[3 * s + k]) - b[k]) / (float) (s + 1);
      if (hit[s]) m[k] = m[k] + (nrm[3 * s + k] - m[k]) / (float) hits;
    }
  }
  CHECK(acc.hits == hits, "n %u pattern %d: hits", n, pattern);
  CHECK(Bits(matteCoverage(acc.hits, n)) == Bits((float) hits / (float) n), "n %u pattern %d: coverage", n, pattern);
  for (int k = 0; k < 3; ++k) {
    CHECK(Bits(acc.albedo[k]) == Bits(a[k]) && Bits(acc.backdrop[k]) == Bits(b[k]) && Bits(acc.normal[k]) == Bits(m[k]), "n %u pattern %d: means", n, pattern);
    if (hits == 0) CHECK(Bits(acc.normal[k]) == 0 && Bits(acc.backdrop[k]) == Bits(acc.albedo[k]), "n %u pattern %d: no hit", n, pattern);
    if (hits == n) CHECK(Bits(acc.backdrop[k]) == 0, "n %u pattern %d: all hit", n, pattern);
    if (n == 1) CHECK(Bits(acc.albedo[k]) == Bits(x[k]), "n 1: the value itself");
  }
}

int main()
{
  const int sizes[3][2] = {{1, 1}, {17, 13}, {33, 35}};
  for (const auto &s : sizes)
    for (int srgb = 0; srgb < 2; ++srgb) CheckFrame(s[0], s[1], srgb != 0);
  const uint32_t runs[5] = {1, 2, 5, 64, 2048};
  for (uint32_t n : runs)
    for (int pattern = 0; pattern < 5; ++pattern) CheckRun(n, pattern);
  CHECK(matteCoverage(0, 0) == 0.f && matteSamples(7, 5) == 5 && matteSamples(3, 5) == 3 && matteSamples(0, 5) == 0, "n = 0 / the clamp");
  if (g_fail) { printf("matte_check: %d failure(s)\n", g_fail); return 1; }
  printf("matte_check: clean\n");
  return 0;
}
