/* tests/cpp/texture_f2i.c - TEST TOOL: the float -> int conversion of the texture lookups (qa_texture_dev.h qa_f2i_x86, compiled for
 * the host inside libqaray_hip.so, entry point qa_test_texture_host op 9) against the x86 instruction the reference's (int) casts
 * compile to (cvttss2si: INT_MIN for NaN and everything outside [-2^31, 2^31)), bit for bit.
 *   texture_f2i <libqaray_hip.so> [stride]   every stride-th block of 65536 float bit patterns; stride 1 = all 2^32 floats */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <xmmintrin.h>
typedef int (*probe_t)(const void *, int, int, int, const float *, float *);
int main(int argc, char **argv)
{
  void *h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
  probe_t f = (probe_t) dlsym(h, "qa_test_texture_host");
  if (!f) { fprintf(stderr, "qa_test_texture_host missing\n"); return 1; }
  const long long stride = argc > 2 ? atoll(argv[2]) : 1;
  unsigned long long bad = 0, total = 0;
#pragma omp parallel reduction(+ : bad, total)
  {
    const int CH = 1 << 16;
    float *in = calloc((size_t) CH * 16, 4), *out = malloc((size_t) CH * 9 * 4);
#pragma omp for schedule(dynamic, 16)
    for (long long c = 0; c < (1LL << 32) / CH; c += stride) {
      for (int i = 0; i < CH; ++i) { const uint32_t u = (uint32_t) (c * CH + i); memcpy(&in[16 * (size_t) i], &u, 4); }
      if (f(NULL, 9, 0, CH, in, out) != 0) { bad++; continue; }
      for (int i = 0; i < CH; ++i) {
        const float x = in[16 * (size_t) i];
        const int want = _mm_cvtt_ss2si(_mm_set_ss(x));
        int got;
        memcpy(&got, &out[9 * (size_t) i], 4);
        total++;
        if (got != want) { if (bad < 5) fprintf(stderr, "(int) %a: x86 %d, helper %d\n", x, want, got); bad++; }
      }
    }
    free(in); free(out);
  }
  printf("%llu conversions, %llu mismatches\n", total, bad);
  return bad != 0;
}
