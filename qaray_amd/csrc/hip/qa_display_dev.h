// qa_display_dev.h — the FrameBuffer's 8-bit products on either side: colour, sample-count byte, z image, sample-count image and
// mask of a frame of float results, and the statistics the two images are scaled with.
//
// Reference: the tail of PixelRender (src/renderers/renderer.cpp:347-365: LinearToSRGB, src/renderers/renderer.cpp:34-39, MIN / MAX,
// roundf, the byte) and FrameBuffer::ComputeZBufferImage / ComputeSampleCountImage (src/fb/framebuffer.cpp:62-107), as
// csrc/host/framebuffer.cpp restates them: the expressions below are that file's, in its operation order (no contraction, the
// correctly rounded division of this build), with qpowf for the host's powf (qa_device_math.h: glibc's bits).
//
// Every function here is compiled for the host too: qa_test_display_host and the kernels of qa_display.hip run the same source;
// tests/test_display_host.py pins the host build to the reference's bytes and to the host FrameBuffer, tests/test_gpu_display.py
// the device build to the host's.
#pragma once
#include "qa_texture_dev.h"

namespace qa {

#define QA_DISPLAY_MISS 1.0e30f /* BIGFLOAT: the depth of a pixel whose sample 0 left the scene */

// A float -> uint8_t cast as the host library's x86-64 build executes it: cvttss2si to a 32-bit int, of which the low byte is
// kept.  NaN and |x| >= 2^31 give 0 (the low byte of INT_MIN); a negative value inside the range gives its int's low byte.
__host__ __device__ __forceinline__ uint8_t displayByte(float x) { return (uint8_t) (uint32_t) qa_f2i_x86(x); }

// LinearToSRGB (src/renderers/renderer.cpp:34-39).  A NaN fails the comparison and goes through qpowf, which returns a NaN
__host__ __device__ __forceinline__ float displaySRGB(float c)
{
  const float a = 0.055f;
  if (c < 0.0031308f) return 12.92f * c;
  return (1.f + a) * qpowf(c, 1.f / 2.4f) - a;
}

// one colour component -> its byte (FrameBuffer::Deposit): MIN(1, c) and MAX(0, .) as the reference's macros expand, so that a NaN
// passes both and ends as byte 0
__host__ __device__ __forceinline__ uint8_t displayColorByte(float c, bool useSRGB)
{
  if (useSRGB) c = displaySRGB(c);
  const float lo = (1.f < c) ? 1.f : c;   // MIN(1, c)
  c = (0.f > lo) ? 0.f : lo;              // MAX(0, ..)
  return displayByte(__builtin_roundf(c * 255.f));
}

// the sample-count byte (FrameBuffer::Deposit)
__host__ __device__ __forceinline__ uint8_t displayCountByte(uint32_t ns, int sppMax) { return displayByte(255.f * (float) ns / (float) sppMax); }

// ComputeZBufferImage's byte (src/fb/framebuffer.cpp:76-82); zmax == zmin gives 0 / 0 = NaN or x / 0 = +-inf: byte 0
__host__ __device__ __forceinline__ uint8_t displayZByte(float z, float zmin, float zmax)
{
  if (z == QA_DISPLAY_MISS) return 0;
  const float f = (zmax - z) / (zmax - zmin);
  return displayByte(f * 255.f);
}

// ComputeSampleCountImage's byte (src/fb/framebuffer.cpp:100-105), integer arithmetic; all zero when smax == smin
__host__ __device__ __forceinline__ uint8_t displayCountImageByte(uint32_t count, uint32_t smin, uint32_t smax)
{
  if (smax == smin) return 0;
  return (uint8_t) ((255 * ((int) count - (int) smin)) / ((int) smax - (int) smin));
}

// What the two images' sequential loops end with: zmin from 1e30 down with >, zmax from 0 up with <, over the depths other than
// 1e30 (a NaN fails both comparisons); smin from 255, smax from 0 over the count bytes.  The result does not depend on the order
// of the pixels except for the sign of a zero zmin (the first zero met stays), which no byte depends on: zmax is never -0, and
// zmax - (+-0) is the same float.  displayStatsEnd makes that zero +0, so that any order gives the same bits.
struct DisplayAcc {
  float zmin, zmax;
  uint32_t smin, smax;
};
__host__ __device__ __forceinline__ DisplayAcc displayAccInit()
{
  DisplayAcc a;
  a.zmin = QA_DISPLAY_MISS; a.zmax = 0.f; a.smin = 255u; a.smax = 0u;
  return a;
}
__host__ __device__ __forceinline__ void displayAccPixel(DisplayAcc &a, float z, uint32_t count)
{
  if (z != QA_DISPLAY_MISS) {   // (a NaN depth gets here and fails both comparisons)
    if (a.zmin > z) a.zmin = z;
    if (a.zmax < z) a.zmax = z;
  }
  if (a.smin > count) a.smin = count;
  if (a.smax < count) a.smax = count;
}
// two partial results (neither holds a NaN; an untouched zmin is 1e30 itself, which no partial zmin exceeds)
__host__ __device__ __forceinline__ void displayAccMerge(DisplayAcc &a, const DisplayAcc &b)
{
  if (a.zmin > b.zmin) a.zmin = b.zmin;
  if (a.zmax < b.zmax) a.zmax = b.zmax;
  if (a.smin > b.smin) a.smin = b.smin;
  if (a.smax < b.smax) a.smax = b.smax;
}
__host__ __device__ __forceinline__ void displayStatsEnd(DisplayAcc &a)
{
  if (a.zmin == 0.f) a.zmin = 0.f;
}

// Floats as unsigned keys of the same order (negative: all bits flipped, else the sign bit set), for the integer atomic min / max
// that combine the workgroups' partial results: right for every non-NaN float, -inf and negative values included
__host__ __device__ __forceinline__ uint32_t displayKey(float f)
{
  const uint32_t u = qa_asuint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float displayUnkey(uint32_t k) { return qa_asfloat((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// A pixel as the FrameBuffer sees it.  ns = 0 is a pixel Deposit skips: it keeps what FrameBuffer::Init left - colour 0, count 0,
// mask 0 and depth 0.0f, which takes part in zmin
struct DisplayPixel {
  float r, g, b, z;
  uint32_t ns;
};
__host__ __device__ __forceinline__ float displayDepth(const DisplayPixel &p) { return p.ns ? p.z : 0.f; }
__host__ __device__ __forceinline__ uint32_t displayCount(const DisplayPixel &p, int sppMax) { return p.ns ? displayCountByte(p.ns, sppMax) : 0u; }

struct DisplayBytes {
  uint8_t r, g, b, count, z, countImg, mask;
};
__host__ __device__ __forceinline__ DisplayBytes displayEncode(const DisplayPixel &p, const DisplayAcc &st, int sppMax, bool useSRGB)
{
  DisplayBytes o;
  const bool on = p.ns != 0u;
  o.r = on ? displayColorByte(p.r, useSRGB) : 0;
  o.g = on ? displayColorByte(p.g, useSRGB) : 0;
  o.b = on ? displayColorByte(p.b, useSRGB) : 0;
  o.count = (uint8_t) displayCount(p, sppMax);
  o.z = displayZByte(displayDepth(p), st.zmin, st.zmax);
  o.countImg = displayCountImageByte(o.count, st.smin, st.smax);
  o.mask = on ? 1 : 0;
  return o;
}

}  // namespace qa
