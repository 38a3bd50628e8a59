// qa_texel_dev.h — one RGB8 texel of a file texture -> its entry of the float texel table (DScene::texels), on either side.
//
// Reference: TextureFile::Sample divides every byte it reads by 255.0f (src/textures/texture.cpp:120-131); the same IEEE division
// once per texel gives the same bits.  BuildTextures (qa_scene_build.cpp, an upload), the kernel of qa_texture_edit.hip (a texel
// edit) and qa_test_texels_host run this source: tests/test_texture_edit_host.py pins the host build to numpy's float32 division
// and to the texture probes, tests/test_gpu_texture_edit.py the device build to the host's.  The division must stay the correctly
// rounded one (-fhip-fp32-correctly-rounded-divide-sqrt, no fast math): a reciprocal multiply misses bits.
#pragma once
#include <hip/hip_runtime.h>   // float4

#include <cstddef>
#include <cstdint>

namespace qa {

__host__ __device__ __forceinline__ float texelFloat(uint32_t byte) { return (float) (int) byte / 255.0f; }

__host__ __device__ __forceinline__ float4 texelEntry(uint32_t r, uint32_t g, uint32_t b)
{
  float4 e;
  e.x = texelFloat(r); e.y = texelFloat(g); e.z = texelFloat(b); e.w = 0.f;
  return e;
}

// h rows of w RGB8 texels, `stride` bytes apart -> w * h entries of 4 floats, row after row (the host's loop over texelEntry)
inline void texelsTabulateHost(const uint8_t *rgb8, size_t w, size_t h, size_t stride, float *out4)
{
  for (size_t y = 0; y < h; ++y) {
    const uint8_t *px = rgb8 + y * stride;
    float *o = out4 + 4 * y * w;
    for (size_t x = 0; x < w; ++x) {
      const float4 e = texelEntry(px[3 * x], px[3 * x + 1], px[3 * x + 2]);
      o[4 * x] = e.x; o[4 * x + 1] = e.y; o[4 * x + 2] = e.z; o[4 * x + 3] = e.w;
    }
  }
}

}  // namespace qa
