// probevis_check.cpp — the host half of qaray_amd/csrc/hip/qa_probevis_dev.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_probevis_host.py builds and runs it).  Every buffer lives on the heap at exactly the size the loops may touch, so a
// step outside one is reported.  Checked here:
//   - the moments at (m, d) = (1, 1), (2, 1), (2, 2), (4, 2), (6, 3), (6, 6), (16, 8) and (128, 1) with 0, -0, dmax, values above
//     it, 1e30, inf and NaN among t: every cell against a double pooling of its texels, 0 <= mean <= dmax, all misses -> dmax;
//   - the cell a vector points into: every texel-centre direction of DIRECTIONS lands in the cell that pools its texel, jittered
//     ones in a cell of their face; the tie rule; zero, huge, inf and NaN vectors stay inside the 6 d^2 cells;
//   - the visibility shading at the edge shapes: counts of 1 on an axis, a single probe, points on the probes (the probe's own
//     shading, bit for bit), outside on every side, void probes (moments 0), normal_bias 0 and 0.1, inputs that are not finite, a
//     biased point that overflows (the trilinear fall-back, bit for bit), uniform coefficients.
// Prints "probevis_check: clean" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "qa_probevis_dev.h"

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

static void CheckMoments(uint32_t m, uint32_t d, float dmax)
{
  const uint32_t K = 6u * m * m, cells = 6u * d * d, r = m / d;
  std::unique_ptr<float[]> t(new float[K]), out(new float[2 * (size_t) cells]);
  Lcg rng(m * 131 + d);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[9] = {0.f, -0.f, dmax, std::nextafter(dmax, 0.f), std::nextafter(dmax, inf), 3.f * dmax, 1e30f, inf, nan};
  for (uint32_t k = 0; k < K; ++k) t[k] = (rng.next() & 3u) ? 2.f * dmax * rng.unit() : 1e30f;
  for (uint32_t i = 0; i < 9 && i < K; ++i) t[(i * 7u) % K] = special[i];
  for (uint32_t cell = 0; cell < cells; ++cell) probeVisMoments(m, d, dmax, t.get(), cell, &out[2 * (size_t) cell]);
  for (uint32_t f = 0; f < 6; ++f)
    for (uint32_t B = 0; B < d; ++B)
      for (uint32_t C = 0; C < d; ++C) {
        double s = 0, s2 = 0;
        for (uint32_t b = B * r; b < (B + 1) * r; ++b)
          for (uint32_t c = C * r; c < (C + 1) * r; ++c) {
            const float tk = t[(f * m + b) * m + c];
            const double x = (tk < dmax) ? tk : dmax;
            s += x; s2 += x * x;
          }
        const float *mo = &out[2 * (size_t) ((f * d + B) * d + C)];
        const double n = (double) r * r;
        // (a running fp32 sum of n terms in [0, dmax]: each addition rounds a partial sum of at most n dmax, so n * 2^-24 of
        // the mean's range bounds the mean's error; the product and the quotient add two roundings)
        const double tol = (n + 2.0) * 5.97e-8;
        CHECK(std::fabs(mo[0] - s / n) <= tol * dmax && std::fabs(mo[1] - s2 / n) <= tol * dmax * dmax, "m %u d %u cell (%u, %u, %u): %g %g", m, d, f, B, C, mo[0], mo[1]);
        CHECK(mo[0] >= 0.f && mo[0] <= dmax * (1.0 + tol) && mo[1] >= 0.f, "m %u d %u: range", m, d);
      }
  for (uint32_t k = 0; k < K; ++k) t[k] = 1e30f;
  for (uint32_t cell = 0; cell < cells; ++cell) {
    probeVisMoments(m, d, dmax, t.get(), cell, &out[2 * (size_t) cell]);
    CHECK(std::fabs(out[2 * (size_t) cell] - dmax) <= ((double) r * r + 2.0) * 5.97e-8 * dmax, "m %u d %u: all misses", m, d);
  }
}

static void CheckCells(uint32_t m, uint32_t d)
{
  const uint32_t K = 6u * m * m, r = m / d;
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t f = k / (m * m), b = (k % (m * m)) / m, c = k % m;
    const ProbeDir centre = probeRecord(m, 0u, 0u, k, false);
    const float far[3] = {centre.d[0] * 3.5f, centre.d[1] * 3.5f, centre.d[2] * 3.5f};
    CHECK(probeVisCell(far, (int) d) == (f * d + b / r) * d + c / r, "m %u d %u ray %u: cell %u", m, d, k, probeVisCell(far, (int) d));
    const ProbeDir jit = probeRecord(m, 0x51A7A7u, 0xFFFFFFFFu, k, true);
    const uint32_t cell = probeVisCell(jit.d, (int) d);
    CHECK(cell < 6u * d * d && cell / (d * d) == f, "m %u d %u ray %u: a jittered ray's face", m, d, k);
  }
}

static void CheckOddVectors()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float vals[9] = {0.f, -0.f, 1.f, -1.f, 1e-45f, 3e38f, inf, -inf, nan};
  for (int d : {1, 2, 3, 8, 128})
    for (float x : vals)
      for (float y : vals)
        for (float z : vals) {
          const float v[3] = {x, y, z};
          CHECK(probeVisCell(v, d) < 6u * (uint32_t) d * (uint32_t) d, "d %d: (%g, %g, %g) leaves the map", d, x, y, z);
        }
  // ties take the lowest axis; the sign picks the face
  const float xy[3] = {1.f, 1.f, 0.5f}, yz[3] = {0.5f, -1.f, -1.f}, all[3] = {-2.f, 2.f, -2.f};
  CHECK(probeVisCell(xy, 1) == 0u && probeVisCell(yz, 1) == 3u && probeVisCell(all, 1) == 1u, "the tie rule");
  // the far edge of a face: u = w = 1 stays in the last row and column
  CHECK(probeVisCell(xy, 4) == (uint32_t) ((0 * 4 + 3) * 4 + 3), "the last column at u = 1: %u", probeVisCell(xy, 4));
}

static void CheckShading()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  Lcg rng(91);
  const int32_t shapes[5][3] = {{3, 4, 2}, {2, 1, 3}, {1, 1, 1}, {1, 5, 1}, {4, 2, 2}};
  for (const int32_t *cn : shapes)
    for (int d : {1, 2, 4}) {
      const size_t probes = (size_t) cn[0] * cn[1] * cn[2], per = (size_t) 12 * d * d;
      std::unique_ptr<float[]> sh(new float[27 * probes]), mo(new float[per * probes]);
      for (size_t i = 0; i < 27 * probes; ++i) sh[i] = 3.f * rng.unit() - 1.f;
      for (size_t q = 0; q < probes; ++q)
        for (size_t i = 0; i < per; i += 2) {
          const float mean = 0.1f + 2.f * rng.unit();
          mo[per * q + i] = (q % 3 == 1) ? 0.f : mean;                                  // (every third probe is void)
          mo[per * q + i + 1] = (q % 3 == 1) ? 0.f : mean * mean + 0.3f * rng.unit();
        }
      ProbeGrid g;
      for (int e = 0; e < 3; ++e) { g.origin[e] = -1.f + (float) e; g.spacing[e] = 0.5f * (float) (e + 1); g.counts[e] = cn[e]; }
      std::unique_ptr<float[]> P(new float[3]), N(new float[3]), out(new float[3]), want(new float[3]);
      N[0] = 0.6f; N[1] = 0.f; N[2] = 0.8f;
      // on every probe (dyadic: exact): that probe's shading
      for (int iz = 0; iz < cn[2]; ++iz)
        for (int iy = 0; iy < cn[1]; ++iy)
          for (int ix = 0; ix < cn[0]; ++ix) {
            const int idx[3] = {ix, iy, iz};
            for (int e = 0; e < 3; ++e) P[e] = g.origin[e] + (float) idx[e] * g.spacing[e];
            probeVisGridShade(g, sh.get(), mo.get(), d, 0.f, P.get(), N.get(), out.get());
            probeShade(&sh[27 * (((size_t) iz * cn[1] + iy) * cn[0] + ix)], N[0], N[1], N[2], want.get());
            CHECK(!memcmp(out.get(), want.get(), 12), "grid %d x %d x %d d %d: probe (%d, %d, %d)", cn[0], cn[1], cn[2], d, ix, iy, iz);
          }
      // outside on every side, far outside, and at random, with and without a bias: inside the arrays (ASan), finite, not negative
      for (int k = 0; k < 400; ++k) {
        for (int e = 0; e < 3; ++e) P[e] = g.origin[e] + ((float) cn[e] + 2.f) * g.spacing[e] * (1.5f * rng.unit() - 0.25f);
        if (k < 6) P[k / 2] = (k & 1) ? 1e30f : -1e30f;
        if (k == 6) { P[0] = 3e38f; P[1] = -3e38f; P[2] = 3e38f; }
        probeVisGridShade(g, sh.get(), mo.get(), d, (k & 1) ? 0.1f : 0.f, P.get(), N.get(), out.get());
        for (int ch = 0; ch < 3; ++ch) CHECK(std::isfinite(out[ch]) && out[ch] >= 0.f, "grid %d x %d x %d d %d: point %d", cn[0], cn[1], cn[2], d, k);
      }
      // a huge bias whose squared distance overflows: every probe is at its floor, the result stays finite
      for (int e = 0; e < 3; ++e) P[e] = g.origin[e] + 0.25f * g.spacing[e];
      probeVisGridShade(g, sh.get(), mo.get(), d, 3e38f, P.get(), N.get(), out.get());
      probeVisGridShade(g, sh.get(), mo.get(), d, -3e38f, P.get(), N.get(), want.get());
      for (int ch = 0; ch < 3; ++ch) CHECK(std::isfinite(out[ch]) && out[ch] >= 0.f && std::isfinite(want[ch]) && want[ch] >= 0.f, "a huge bias");
      // inputs that are not finite shade to +0
      const float bad[3] = {nan, inf, -inf};
      for (int k = 0; k < 18; ++k) {
        for (int e = 0; e < 3; ++e) { P[e] = g.origin[e]; N[e] = e == 2 ? 1.f : 0.f; }
        (k < 9 ? P : N)[(k % 9) / 3] = bad[k % 3];
        probeVisGridShade(g, sh.get(), mo.get(), d, 0.1f, P.get(), N.get(), out.get());
        CHECK(Bits(out[0]) == 0u && Bits(out[1]) == 0u && Bits(out[2]) == 0u, "input %d that is not finite", k);
      }
      // a normal whose bias overflows to inf: v is inf, W is NaN, the fall-back's bits
      for (int e = 0; e < 3; ++e) { P[e] = g.origin[e] + 0.25f * g.spacing[e]; N[e] = e == 0 ? 3e38f : 0.f; }
      probeVisGridShade(g, sh.get(), mo.get(), d, 2.f, P.get(), N.get(), out.get());
      probeGridShade(g, sh.get(), P.get(), N.get(), want.get());
      CHECK(!memcmp(out.get(), want.get(), 12), "grid %d x %d x %d d %d: the fall-back", cn[0], cn[1], cn[2], d);
      // uniform coefficients: one probe's shading within 40 * 2^-24 T, T <= 9 terms of |sh| <= 2 and |A Y| <= 1 (the derivation:
      // tests/test_probevis_host.py; twice that, as both sides are fp32)
      for (size_t q = 1; q < probes; ++q) memcpy(&sh[27 * q], &sh[0], 27 * sizeof(float));
      N[0] = 0.6f; N[1] = 0.f; N[2] = 0.8f;
      for (int e = 0; e < 3; ++e) P[e] = g.origin[e] + 0.3f * g.spacing[e] * (float) (cn[e] - 1);
      probeVisGridShade(g, sh.get(), mo.get(), d, 0.1f, P.get(), N.get(), out.get());
      probeShade(&sh[0], N[0], N[1], N[2], want.get());
      for (int ch = 0; ch < 3; ++ch) CHECK(std::fabs(out[ch] - want[ch]) <= 80.f * 5.96e-8f * 9.f * 2.f, "uniform coefficients: %.9g against %.9g", out[ch], want[ch]);
    }
}

int main()
{
  const uint32_t md[8][2] = {{1, 1}, {2, 1}, {2, 2}, {4, 2}, {6, 3}, {6, 6}, {16, 8}, {128, 1}};
  for (const uint32_t *p : md) {
    CheckMoments(p[0], p[1], 1.5f);
    CheckMoments(p[0], p[1], 0.37f);
    if (p[0] <= 16) CheckCells(p[0], p[1]);
  }
  CheckOddVectors();
  CheckShading();

  if (g_fail) { printf("probevis_check: %d failure(s)\n", g_fail); return 1; }
  printf("probevis_check: clean\n");
  return 0;
}
