// tests/cpp/progressive_fb_state.cpp - TEST TOOL (needs a GPU): the FrameBuffer a progressive run of the batch driver's Renderer
// leaves (its passes' products come from the device, qa_progressive_display) against the one the one-shot run leaves (the float frame
// through FrameBuffer::Deposit): colour, z buffer floats, sample-count bytes, mask and both images must be the same, and the rendered
// pixels counted once per pass, as Deposit counted them.
//   progressive_fb_state <scene.xml> <asset root> <width> <height> <spp> <pass spp> <out prefix>
// Build: like the batch driver (csrc/Makefile, target app), with this file in place of app/main.cpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "renderer.h"

using namespace qaray_hip;

static int Differ(const char *what, const void *a, const void *b, size_t bytes)
{
  if (!memcmp(a, b, bytes)) return 0;
  fprintf(stderr, "%s differs\n", what);
  return 1;
}

int main(int argc, char **argv)
{
  if (argc < 8) { fprintf(stderr, "usage: progressive_fb_state scene root w h spp pass out\n"); return 2; }
  const int w = atoi(argv[3]), h = atoi(argv[4]), spp = atoi(argv[5]), pass = atoi(argv[6]);
  try {
    FrameBuffer fbs[2];
    for (int mode = 0; mode < 2; ++mode) {
      RendererParam param;
      param.SetSPPMax(spp);
      param.SetSPPMin(spp);
      Renderer renderer(param, 0);
      renderer.outputPrefix = std::string(argv[7]) + (mode ? "prog_" : "one_");
      renderer.Init();
      Scene scene;
      scene.assetRoot = argv[2];
      if (!scene.assetRoot.empty() && scene.assetRoot.back() != '/') scene.assetRoot += '/';
      LoadSceneInSilentMode(true);
      if (!LoadScene(argv[1], scene)) { fprintf(stderr, "Failed to load %s\n", argv[1]); return 1; }
      scene.camera.imgWidth = w;
      scene.camera.imgHeight = h;
      renderer.ComputeScene(fbs[mode], scene);
      if (mode) renderer.RenderProgressive((size_t) pass);
      else renderer.Render();
      renderer.Terminate();
    }
    const FrameBuffer &a = fbs[0], &b = fbs[1];
    const size_t n = (size_t) w * h;
    int bad = Differ("colour", a.GetPixels(), b.GetPixels(), 3 * n) + Differ("z buffer", a.GetZBuffer(), b.GetZBuffer(), n * sizeof(float)) +
              Differ("sample count", a.GetSampleCount(), b.GetSampleCount(), n) + Differ("mask", a.GetMasks(), b.GetMasks(), n) +
              Differ("z image", a.GetZBufferImage(), b.GetZBufferImage(), n) +
              Differ("sample-count image", a.GetSampleCountImage(), b.GetSampleCountImage(), n);
    const int passes = (spp + pass - 1) / pass;
    if (a.GetNumRenderedPixels() != (int) n || b.GetNumRenderedPixels() != passes * (int) n) {
      fprintf(stderr, "rendered pixels: one-shot %d, progressive %d (expected %zu and %zu)\n", a.GetNumRenderedPixels(), b.GetNumRenderedPixels(), n,
              (size_t) passes * n);
      bad++;
    }
    if (!b.IsRenderDone()) { fprintf(stderr, "progressive frame not done\n"); bad++; }
    printf("framebuffer state after %d passes: %s\n", passes, bad ? "DIFFERENT" : "same as the one-shot run's");
    return bad ? 1 : 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "progressive_fb_state: %s\n", e.what());
    return 2;
  }
}
