// renderer.h — host-side Renderer: the reference's batch renderer with its integrator loop
// replaced by calls into the HIP layer (include/qaray_hip.h).
//
// Mirrors src/renderers/renderer.h:47-111 (RendererParam, Renderer::Init / ComputeScene / Render /
// ThreadRender / Start-Stop-KillTimer / Terminate) and the batch flow of Renderer_MPI::Render
// (src/renderers/Renderer_MPI.cpp:123-215: render, save colorBuffer / depthBuffer / sampleBuffer
// PNGs).  ThreadRender() keeps its name and its place in the call stack; what used to be two nested
// tasking::parallel_for loops over tiles and pixels (renderer.cpp:383-420) is one
// qa_render_region / qa_render_strips call.
#pragma once
#include <limits>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "framebuffer.h"
#include "qaray_hip.h"
#include "scene.h"

namespace qaray_hip {

struct RendererParam {  // src/renderers/renderer.h:47-68
  bool useSRGB = true;
  size_t sppMax = 8;
  size_t sppMin = 4;
  uint32_t seed = 0x51A7A7;
  bool usePhotonMap = false;
  size_t photonMapSize = 10000;
  size_t photonMapBounce = 20;
  float photonMapRadius = 0.2f;
  size_t causticsMapSize = 1000;
  size_t causticsMapBounce = 20;
  float causticsMapRadius = 1.0f;
  void SetSPPMax(int spp) { sppMax = static_cast<size_t>(spp); }
  void SetSPPMin(int spp) { sppMin = static_cast<size_t>(spp); }
  void SetSRGBFlag(bool flag) { useSRGB = flag; }
  void SetPhotonMappingFlag(bool flag) { usePhotonMap = flag; }
  void SetPhotonMapBounce(size_t b) { photonMapBounce = b; }
  void SetPhotonMapSize(size_t sz) { photonMapSize = sz; }
  void SetPhotonMapRadius(float r) { photonMapRadius = r; }
  void SetCausticsMapBounce(size_t b) { causticsMapBounce = b; }
  void SetCausticsMapSize(size_t sz) { causticsMapSize = sz; }
  void SetCausticsMapRadius(float r) { causticsMapRadius = r; }
};

class Renderer {
 public:
  explicit Renderer(RendererParam &param, int device = 0, size_t rank = 0, size_t size = 1);
  // One process, several GPUs (qaray_hip -devices N): the role Renderer_MPI plays across MPI ranks
  // (src/renderers/Renderer_MPI.cpp:123-215), inside one address space.  One host thread and one qa_ctx per device; the
  // flattened scene is uploaded to the first device and copied to the others device-to-device (xGMI); device i renders the
  // 8-row strips i, i + N, ...; the packed colour | depth | sample-count strips are copied to the first device
  // (hipMemcpyPeerAsync) and placed from there (PlaceStrips = PlaceImage<T>).  devices.size() == 1 takes the same path.
  void UseDevices(const std::vector<int> &devices) { multi = devices; }
  virtual ~Renderer();
  virtual void Init();                                  // creates the HIP context
  void ComputeScene(FrameBuffer &renderImage, Scene &scene);  // camera frame, fb, scene upload, photon maps
  virtual void Render();                                // ThreadRender + image dumps (batch mode)
  void ThreadRender();                                  // the hot path: one HIP call
  void RenderProgressive(size_t passSpp);               // Render in passes of passSpp samples, images rewritten after each
  virtual void StartTimer();
  virtual void StopTimer();
  virtual void KillTimer();
  virtual void Terminate();
  double LastSeconds() const { return lastSeconds; }
  const qa_counters &Counters() const { return counters; }
  std::string outputPrefix;                             // like Renderer_MPI's mpiPrefix
  // -denoise [N]: a fourth image, <prefix>denoisedBuffer.png, the colour bytes of the frame filtered on the device
  // (qa_denoise_device, then qa_display_device); N iterations, -1 = the library's default.  One device only
  bool denoise = false;
  int denoiseIterations = -1;
  bool denoiseGuided = false;   // -denoise-guided [N]: the same image through qa_denoise_guided_device with the frame's normal and albedo planes
  // -alpha: another image, <prefix>rgbaBuffer.png, the frame with straight alpha (4 channels): coverage and backdrop of the frame's own
  // sample counts (qa_matte_region_device / qa_progressive_matte_device), then qa_matte_rgba_device.  One device only
  bool alpha = false;
  // -matte-node NAME (repeatable): per node an image, <prefix>matte_NAME.png, 8-bit grey: the fraction of a pixel's samples whose camera
  // ray meets that node first (qa_idmatte_region_device / qa_progressive_idmatte_device once, then qa_idmatte_select_device per
  // node).  (name, the flattener's index of the node: FindNodeIndex.)  One device only
  std::vector<std::pair<std::string, int>> matteNodes;
  // -ao [K] (aoRays > 0) and -ao-radius R: another image, <prefix>aoBuffer.png, 8-bit grey: the ambient occlusion of what the frame's own
  // samples see, K rays per hit within R (qa_ao_region_device / qa_progressive_ao_device with the frame's seed, then qa_ao_grey_device).
  // One device only
  int aoRays = 0;
  float aoRadius = std::numeric_limits<float>::infinity();

 protected:
  RendererParam &param;
  Scene *scene = nullptr;
  FrameBuffer *image = nullptr;
  size_t pixelW = 0, pixelH = 0;
  size_t mpiSize = 1, mpiRank = 0;                      // strip partition: rank, rank+size, ...
  int device = 0;
  qa_ctx *ctx = nullptr;
  std::vector<int> multi;                               // UseDevices: empty = the single-context path
  std::vector<qa_ctx *> ctxs;                           // one per entry of `multi`
  void ThreadRenderMulti();
  void SaveImages();                                    // the three PNGs of the FrameBuffer
  void SaveDenoised(float *dRgb, const float *dDepth, const uint32_t *dNs);   // the fourth; dRgb is filtered in place
  void SaveAlpha(const float *dRgb, const uint32_t *dNs, bool progressive);   // rgbaBuffer.png of the frame in device buffers
  void SaveNodeMattes(const uint32_t *dNs, bool progressive);                 // matte_NAME.png of every -matte-node
  void SaveAo(const uint32_t *dNs, bool progressive);                         // aoBuffer.png
  struct DeviceFrame {                                  // -denoise, -alpha, -matte-node, -ao: the frame's floats on the device, freed with the Renderer at the latest
    float *rgb = nullptr, *depth = nullptr;
    uint32_t *ns = nullptr;
    void Alloc(size_t npix);
    void Free();
    ~DeviceFrame() { Free(); }
  } denoiseFrame;
  double lastSeconds = 0, avgSeconds = 0;
  int numFrames = -1;
  qa_counters counters{};
};

}  // namespace qaray_hip
