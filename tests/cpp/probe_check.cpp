// probe_check.cpp — the host half of qaray_amd/csrc/hip/qa_lightprobe_dev.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_probe_host.py builds and runs it).  Every buffer lives on the heap at exactly the size the loops may touch, so a step
// outside one is reported.  Checked here:
//   - directions and weights at m = 1, 2, 3, 5, 16 and 128, centres and jitter, stream ids at both ends of 32 bits: unit length to
//     4e-7, the face and the texel a direction falls into, weights > 0, jitter offsets in [0, 1);
//   - the projection as the wave does it (64 lanes, the butterfly) at K = 6, 54, 96 and 150 - below, across and well above 64
//     lanes - with NaN, inf and -0 among the radiance: every lane ends with the same bits, hits and tmin are the plain count and
//     minimum, a constant radiance lands on band 0;
//   - shading and grid shading at the edge shapes: counts of 1 on an axis, a single probe, points outside the grid on every side,
//     points on the probes (the probe's own shading, bit for bit), the last cell's far edge, inputs that are not finite, an index
//     clamped at both ends.
// Prints "probe_check: clean" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "qa_lightprobe_dev.h"

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

static void CheckDirections(uint32_t m, bool jitter, uint32_t seed, uint32_t S)
{
  const uint32_t K = 6u * m * m;
  std::unique_ptr<float[]> d(new float[3 * (size_t) K]), w(new float[K]);
  for (uint32_t k = 0; k < K; ++k) {
    float j0, j1;
    probeOffsets(seed, S, k, jitter, j0, j1);
    CHECK(j0 >= 0.f && j0 < 1.f && j1 >= 0.f && j1 < 1.f, "m %u ray %u: offsets %g %g", m, k, j0, j1);
    if (!jitter) CHECK(j0 == 0.5f && j1 == 0.5f, "m %u ray %u: centres", m, k);
    const ProbeDir pd = probeRecord(m, seed, S, k, jitter);
    for (int e = 0; e < 3; ++e) d[3 * (size_t) k + e] = pd.d[e];
    w[k] = pd.w;
  }
  for (uint32_t k = 0; k < K; ++k) {
    const float *v = &d[3 * (size_t) k];
    const double l = std::sqrt((double) v[0] * v[0] + (double) v[1] * v[1] + (double) v[2] * v[2]);
    CHECK(std::fabs(l - 1.0) < 4e-7, "m %u ray %u: length %.9g", m, k, l);
    CHECK(w[k] > 0.f && w[k] <= 4.f / (float) (m * m), "m %u ray %u: weight %g", m, k, w[k]);
    // the face: the major axis and its sign; the texel: the other two components over the major one
    const uint32_t f = k / (m * m), a = f / 2;
    const float s = (f & 1u) ? -1.f : 1.f;
    CHECK(v[a] * s > 0.f && std::fabs(v[a]) >= std::fabs(v[(a + 1) % 3]) && std::fabs(v[a]) >= std::fabs(v[(a + 2) % 3]), "m %u ray %u: face", m, k);
    const double u = v[(a + 1) % 3] / (v[a] * s), t = v[(a + 2) % 3] * s / (v[a] * s);
    const uint32_t c = k % m, b = (k % (m * m)) / m;
    const double cu = (u + 1.0) * 0.5 * m, cv = (t + 1.0) * 0.5 * m;
    CHECK(cu > c - 1e-4 && cu < c + 1 + 1e-4 && cv > b - 1e-4 && cv < b + 1 + 1e-4, "m %u ray %u: texel (%g, %g) of column %u row %u", m, k, cu, cv, c, b);
  }
  CHECK(probeRayStream(S, K, K - 1) == (uint32_t) ((uint64_t) S * K + K - 1), "stream ids wrap");
}

static void CheckProjection(uint32_t m, bool special)
{
  const uint32_t K = 6u * m * m;
  std::unique_ptr<float[]> d(new float[3 * (size_t) K]), w(new float[K]), rgb(new float[3 * (size_t) K]), t(new float[K]);
  Lcg rng(m * 2 + special);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  uint32_t wantHits = 0;
  float wantMin = 1e30f;
  for (uint32_t k = 0; k < K; ++k) {
    const ProbeDir pd = probeRecord(m, 0x51A7A7u, 0xFFFFFFFFu, k, true);
    for (int e = 0; e < 3; ++e) { d[3 * (size_t) k + e] = pd.d[e]; rgb[3 * (size_t) k + e] = special ? 4.f * rng.unit() : 0.5f; }
    w[k] = pd.w;
    t[k] = (rng.next() & 3u) ? 0.01f + 50.f * rng.unit() : 1e30f;
    if (t[k] < 1e30f) { ++wantHits; wantMin = t[k] < wantMin ? t[k] : wantMin; }
  }
  if (special) {
    rgb[0] = nan; rgb[3 * (size_t) K - 1] = inf; rgb[(3 * (size_t) K) / 2] = -0.f;
    if (K > 64) rgb[3 * 64 + 1] = -inf;
  }
  std::unique_ptr<ProbeAcc[]> lanes(new ProbeAcc[QA_PROBE_LANES]), next(new ProbeAcc[QA_PROBE_LANES]);
  for (uint32_t l = 0; l < QA_PROBE_LANES; ++l) {
    probeAccInit(lanes[l]);
    for (uint32_t k = l; k < K; k += QA_PROBE_LANES) probeAccAdd(lanes[l], &d[3 * (size_t) k], w[k], &rgb[3 * (size_t) k], t[k]);
  }
  for (uint32_t off = 32; off >= 1; off >>= 1) {
    for (uint32_t l = 0; l < QA_PROBE_LANES; ++l) { next[l] = lanes[l]; probeAccFold(next[l], lanes[l ^ off]); }
    for (uint32_t l = 0; l < QA_PROBE_LANES; ++l) lanes[l] = next[l];
  }
  std::unique_ptr<float[]> sh(new float[27]), other(new float[27]);
  probeAccFinish(lanes[0], sh.get());
  for (uint32_t l = 1; l < QA_PROBE_LANES; ++l) {
    probeAccFinish(lanes[l], other.get());
    CHECK(!memcmp(sh.get(), other.get(), 27 * sizeof(float)) && lanes[l].hits == lanes[0].hits && Bits(lanes[l].tmin) == Bits(lanes[0].tmin),
          "m %u: lane %u ends with other bits than lane 0", m, l);
  }
  CHECK(lanes[0].hits == wantHits && lanes[0].tmin == wantMin, "m %u: hits %u (%u), tmin %g (%g)", m, lanes[0].hits, wantHits, lanes[0].tmin, wantMin);
  if (!special) {
    // a constant 0.5: band 0 is 0.5 * Y0 * 4 pi up to rounding, whatever the weights sum to
    for (int ch = 0; ch < 3; ++ch) CHECK(std::fabs(sh[ch] - 0.5 * 0.282095 * 12.566371) < 1e-5, "m %u: band 0 of a constant, %.9g", m, sh[ch]);
  }
}

static void CheckShading()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  Lcg rng(77);
  const int32_t shapes[5][3] = {{3, 4, 2}, {2, 1, 3}, {1, 1, 1}, {1, 5, 1}, {1, 1, 4}};
  for (const int32_t *cn : shapes) {
    const size_t probes = (size_t) cn[0] * cn[1] * cn[2];
    std::unique_ptr<float[]> sh(new float[27 * probes]);
    for (size_t i = 0; i < 27 * probes; ++i) sh[i] = 3.f * rng.unit() - 1.f;
    ProbeGrid g;
    for (int e = 0; e < 3; ++e) { g.origin[e] = -1.f + (float) e; g.spacing[e] = 0.5f * (float) (e + 1); g.counts[e] = cn[e]; }
    std::unique_ptr<float[]> P(new float[3]), N(new float[3]), out(new float[3]), want(new float[3]);
    N[0] = 0.6f; N[1] = 0.f; N[2] = 0.8f;
    // on every probe: that probe's shading
    for (int iz = 0; iz < cn[2]; ++iz)
      for (int iy = 0; iy < cn[1]; ++iy)
        for (int ix = 0; ix < cn[0]; ++ix) {
          const int idx[3] = {ix, iy, iz};
          for (int e = 0; e < 3; ++e) P[e] = g.origin[e] + (float) idx[e] * g.spacing[e];   // (dyadic: exact)
          probeGridShade(g, sh.get(), P.get(), N.get(), out.get());
          probeShade(&sh[27 * (((size_t) iz * cn[1] + iy) * cn[0] + ix)], N[0], N[1], N[2], want.get());
          CHECK(!memcmp(out.get(), want.get(), 12), "grid %d x %d x %d: probe (%d, %d, %d)", cn[0], cn[1], cn[2], ix, iy, iz);
        }
    // outside on every side, far outside, and at random: the walk stays inside sh (ASan), the result is finite and not negative
    for (int k = 0; k < 400; ++k) {
      for (int e = 0; e < 3; ++e) P[e] = g.origin[e] + ((float) cn[e] + 2.f) * g.spacing[e] * (1.5f * rng.unit() - 0.25f);
      if (k < 6) P[k / 2] = (k & 1) ? 1e30f : -1e30f;
      if (k == 6) { P[0] = 3e38f; P[1] = -3e38f; P[2] = 3e38f; }
      probeGridShade(g, sh.get(), P.get(), N.get(), out.get());
      for (int ch = 0; ch < 3; ++ch) CHECK(std::isfinite(out[ch]) && out[ch] >= 0.f, "grid %d x %d x %d: point %d", cn[0], cn[1], cn[2], k);
    }
    // inputs that are not finite shade to +0
    const float bad[3] = {nan, inf, -inf};
    for (int k = 0; k < 18; ++k) {
      for (int e = 0; e < 3; ++e) { P[e] = g.origin[e]; N[e] = e == 2 ? 1.f : 0.f; }
      (k < 9 ? P : N)[(k % 9) / 3] = bad[k % 3];
      probeGridShade(g, sh.get(), P.get(), N.get(), out.get());
      CHECK(Bits(out[0]) == 0u && Bits(out[1]) == 0u && Bits(out[2]) == 0u, "input %d that is not finite", k);
    }
    // the axis function at its edges
    int i0, i1;
    float f;
    probeGridAxis(-5.f, 0.f, 1.f, 4, i0, i1, f);
    CHECK(i0 == 0 && i1 == 1 && f == 0.f, "below the grid");
    probeGridAxis(3.f, 0.f, 1.f, 4, i0, i1, f);
    CHECK(i0 == 2 && i1 == 3 && f == 1.f, "on the last probe");
    probeGridAxis(1e30f, 0.f, 1.f, 4, i0, i1, f);
    CHECK(i0 == 2 && i1 == 3 && f == 1.f, "above the grid");
    probeGridAxis(2.25f, 0.f, 1.f, 4, i0, i1, f);
    CHECK(i0 == 2 && i1 == 3 && f == 0.25f, "inside the last cell");
    probeGridAxis(7.f, 0.f, 1.f, 1, i0, i1, f);
    CHECK(i0 == 0 && i1 == 0 && f == 0.f, "a count of 1");
  }
  // the index clamp, the shade's NaN sum and negative sum
  CHECK(probeIndex(-7, 5) == 0 && probeIndex(0, 5) == 0 && probeIndex(4, 5) == 4 && probeIndex(5, 5) == 4 && probeIndex(0x7FFFFFFF, 1) == 0, "index clamp");
  std::unique_ptr<float[]> sh(new float[27]), out(new float[3]);
  for (int i = 0; i < 27; ++i) sh[i] = 0.f;
  sh[0] = nan; sh[1] = -1.f; sh[2] = 1.f;
  probeShade(sh.get(), 0.f, 0.f, 1.f, out.get());
  CHECK(Bits(out[0]) == 0u && Bits(out[1]) == 0u && Bits(out[2]) == Bits(0.282095f), "NaN and negative sums shade to 0");
}

int main()
{
  const uint32_t ms[6] = {1, 2, 3, 5, 16, 128};
  const uint32_t streams[3] = {0u, 1u, 0xFFFFFFFFu};
  for (uint32_t m : ms)
    for (uint32_t S : streams) {
      CheckDirections(m, false, 0x51A7A7u, S);
      if (m <= 16) CheckDirections(m, true, S ? 0xFFFFFFFFu : 0u, S);
    }
  const uint32_t pm[4] = {1, 3, 4, 5};
  for (uint32_t m : pm) { CheckProjection(m, false); CheckProjection(m, true); }
  CheckShading();

  if (g_fail) { printf("probe_check: %d failure(s)\n", g_fail); return 1; }
  printf("probe_check: clean\n");
  return 0;
}
