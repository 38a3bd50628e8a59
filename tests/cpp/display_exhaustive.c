/* tests/cpp/display_exhaustive.c - TEST TOOL: the colour byte of the 8-bit products (qa_display_dev.h displayColorByte, compiled for
 * the host inside libqaray_hip.so, entry point qa_test_display_host) against the expression of csrc/host/framebuffer.cpp
 * (LinearToSRGB, MIN, MAX, roundf, the byte) built here with the host libm, for both sRGB settings.
 *   display_exhaustive <libqaray_hip.so> [stride]   every stride-th block of 196608 float bit patterns; stride 1 = all 2^32 floats
 * Build: gcc -O2 -ffp-contract=off -fopenmp display_exhaustive.c -o display_exhaustive -ldl -lm */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <omp.h>
typedef int (*fn_t)(const float *, const float *, const uint32_t *, uint64_t, int, int, uint8_t *, uint8_t *, uint8_t *, uint8_t *, uint8_t *, void *);

static float linear_to_srgb(const float c)
{
  const float a = 0.055f;
  if (c < 0.0031308f) return 12.92f * c;
  return (1.f + a) * powf(c, 1.f / 2.4f) - a;
}
static uint8_t color_byte(float c, int srgb)
{
  if (srgb) c = linear_to_srgb(c);
  const float lo = (1.f < c) ? 1.f : c;
  c = (0.f > lo) ? 0.f : lo;
  return (uint8_t) roundf(c * 255.f);
}

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: display_exhaustive <libqaray_hip.so> [stride]\n"); return 2; }
  void *h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
  fn_t f = (fn_t) dlsym(h, "qa_test_display_host");
  if (!f) { fprintf(stderr, "no qa_test_display_host\n"); return 1; }
  const long long stride = argc > 2 ? atoll(argv[2]) : 1;
  unsigned long long bad = 0, total = 0;
  enum { PIX = 1 << 16, CH = 3 * PIX };
  const long long chunks = ((1LL << 32) + CH - 1) / CH;
#pragma omp parallel reduction(+ : bad, total)
  {
    float *x = malloc(CH * 4), *z = malloc(PIX * 4);
    uint32_t *ns = malloc(PIX * 4);
    uint8_t *o = malloc(CH);
    for (int i = 0; i < PIX; ++i) { z[i] = 1.f; ns[i] = 1u; }
#pragma omp for schedule(dynamic, 16)
    for (long long c = 0; c < chunks; c += stride) {
      for (int i = 0; i < CH; ++i) { const uint32_t u = (uint32_t) (c * CH + i); memcpy(&x[i], &u, 4); }   /* (the last chunk wraps: harmless) */
      for (int srgb = 0; srgb < 2; ++srgb) {
        if (f(x, z, ns, PIX, 1, srgb, o, NULL, NULL, NULL, NULL, NULL) != 0) { bad++; continue; }
        for (int i = 0; i < CH; ++i) {
          const uint8_t e = color_byte(x[i], srgb);
          total++;
          if (e != o[i]) { if (bad < 5) fprintf(stderr, "srgb %d: colour byte of %a: framebuffer.cpp's expression %u, qa_display_dev.h %u\n", srgb, x[i], e, o[i]); bad++; }
        }
      }
    }
  }
  printf("colour byte, sRGB off and on: %llu evaluations, %llu mismatches\n", total, bad);
  return bad != 0;
}
