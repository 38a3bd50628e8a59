// Why qa_integrate_lastcast carries no Beer-Lambert block (qa_kernel_lastcast_body.h section C): PlanLastCast admits a scene only
// where every material's absorption is +0 or -0, so the factor of a back-face hit at distance z is qexpf(-a * z) with a = +-0 and z
// finite and positive, and the throughput is multiplied by it.  Shown here on the host build of qa_device_math.h (the device build
// is pinned to it by tests/test_gpu_device_math.py), stand-alone, no GPU:
//   * qexpf(-a * z) has the bits of 1.0f for a in {+0, -0} and a sweep of finite z > 0, denormals and QA_BIGFLOAT among them
//   * t * 1.0f has t's bits for a sweep of floats, -0, denormals and infinities among them
// Exit code 0 and "absorb_identity_check: clean" = both hold.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "qa_device_math.h"
#include "qa_flat_scene.h"

using namespace qa;

static uint32_t Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float Float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main()
{
  unsigned long long factors = 0, products = 0, bad = 0;
  const float zero[2] = {0.f, -0.f};
  auto factor = [&](float z) {
    for (float a : zero) {
      // the kernel's expression: qexpf(-asF(ab.x) * h.z); volatile keeps the compiler from folding it
      volatile float av = a, zv = z;
      const float f = qexpf(-av * zv);
      ++factors;
      if (Bits(f) != 0x3f800000u && bad++ < 5) printf("  qexpf(-(%a) * %a) = %a\n", (double) a, (double) z, (double) f);
    }
  };
  // every finite positive float whose low 12 mantissa bits are one of three patterns: denormals (exponent 0) to FLT_MAX
  for (uint32_t hi = 0; hi < (0x7f800000u >> 12); ++hi)
    for (uint32_t lo : {0x000u, 0x001u, 0xfffu}) {
      const uint32_t u = (hi << 12) | lo;
      if (u == 0) continue;
      factor(Float(u));
    }
  factor(Float(1u));            // the smallest denormal
  factor(Float(0x007fffffu));   // the largest
  factor(Float(0x00800000u));   // FLT_MIN
  factor(QA_BIGFLOAT);
  factor(Float(0x7f7fffffu));   // FLT_MAX

  auto product = [&](uint32_t u) {
    volatile float t = Float(u), one = 1.0f;
    const float p = t * one;
    ++products;
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;   // (a NaN stays a NaN; no throughput of these scenes is one)
    if (nan ? p == p : Bits(p) != u) { if (bad++ < 5) printf("  %08x * 1.0f = %08x\n", u, Bits(p)); }
  };
  for (uint32_t hi = 0; hi < (1u << 20); ++hi)   // both signs, every exponent, denormals and infinities included
    for (uint32_t lo : {0x000u, 0x001u, 0xfffu}) product((hi << 12) | lo);
  product(0x80000000u);   // -0
  product(0x00000001u);
  product(0x80000001u);
  product(0x807fffffu);

  printf("absorb_identity_check: %llu factors, %llu products, %llu not as claimed\n", factors, products, bad);
  printf(bad ? "absorb_identity_check: FAILED\n" : "absorb_identity_check: clean\n");
  return bad ? 1 : 0;
}
