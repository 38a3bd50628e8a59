// renderer.cpp — see renderer.h.
#include "renderer.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "image.h"

namespace qaray_hip {

static std::chrono::time_point<std::chrono::system_clock> g_start;

Renderer::Renderer(RendererParam &p, int dev, size_t rank, size_t size) : param(p), mpiSize(size), mpiRank(rank), device(dev)
{
  tasking::signal_start();  // src/renderers/renderer.cpp:67-70
}
Renderer::~Renderer()
{
  for (qa_ctx *c : ctxs) if (c) qa_ctx_destroy(c);
  if (ctx) qa_ctx_destroy(ctx);
}

void Renderer::Init()
{
  if (multi.empty()) {
    if (qa_ctx_create(device, &ctx) != QA_OK) throw std::runtime_error(std::string("qa_ctx_create: ") + qa_last_error());
    return;
  }
  ctxs.assign(multi.size(), nullptr);
  for (size_t i = 0; i < multi.size(); ++i)
    if (qa_ctx_create(multi[i], &ctxs[i]) != QA_OK) throw std::runtime_error(std::string("qa_ctx_create: ") + qa_last_error());
}

// Run f(i) on one host thread per device and rethrow the first failure
template <class F>
static void PerDevice(size_t n, F f)
{
  std::vector<std::thread> th;
  std::vector<std::string> err(n);
  for (size_t i = 0; i < n; ++i)
    th.emplace_back([&, i]() {
      try { f(i); } catch (const std::exception &e) { err[i] = e.what(); }
    });
  for (std::thread &t : th) t.join();
  for (const std::string &e : err) if (!e.empty()) throw std::runtime_error(e);
}
#define HIP_OR_THROW(expr)                                                                               \
  do {                                                                                                   \
    const hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

// src/renderers/renderer.cpp:71-113: canvas + framebuffer here, camera frame inside the flattener
void Renderer::ComputeScene(FrameBuffer &fb, Scene &sc)
{
  image = &fb;
  scene = &sc;
  pixelW = static_cast<size_t>(sc.camera.imgWidth);
  pixelH = static_cast<size_t>(sc.camera.imgHeight);
  image->Init(static_cast<unsigned>(pixelW), static_cast<unsigned>(pixelH));
  const std::vector<unsigned char> blob = FlattenScene(sc);
  if (!multi.empty()) {
    // the flattened scene goes to the first device from the host and to the others device-to-device (the reference re-parses
    // the XML on every rank, Renderer_MPI.cpp:54; across processes bench.py broadcasts the same blob over RCCL)
    unsigned char *d0 = nullptr;
    HIP_OR_THROW(hipSetDevice(multi[0]));
    HIP_OR_THROW(hipMalloc((void **) &d0, blob.size()));
    HIP_OR_THROW(hipMemcpy(d0, blob.data(), blob.size(), hipMemcpyHostToDevice));
    PerDevice(multi.size(), [&](size_t i) {
      HIP_OR_THROW(hipSetDevice(multi[i]));
      unsigned char *di = d0;
      if (i > 0) {
        HIP_OR_THROW(hipMalloc((void **) &di, blob.size()));
        HIP_OR_THROW(hipMemcpyPeer(di, multi[i], d0, multi[0], blob.size()));
      }
      const int rc = qa_scene_upload_device(ctxs[i], di, blob.size());
      if (i > 0) (void) hipFree(di);
      if (rc != QA_OK) throw std::runtime_error(std::string("qa_scene_upload_device: ") + qa_last_error());
    });
    HIP_OR_THROW(hipSetDevice(multi[0]));
    (void) hipFree(d0);
    if (param.usePhotonMap) throw std::runtime_error("-use-photon-map with -devices is not wired up (every device would build the same maps)");
    return;
  }
  if (qa_scene_upload(ctx, blob.data(), blob.size()) != QA_OK)
    throw std::runtime_error(std::string("qa_scene_upload: ") + qa_last_error());
  // src/renderers/renderer.cpp:114-291: both maps, when asked for and non-empty
  if (param.usePhotonMap && param.photonMapSize > 0 && param.causticsMapSize > 0) {
    const auto t0 = std::chrono::system_clock::now();
    qa_photon_params pp;
    pp.photon.size = (uint32_t) param.photonMapSize;
    pp.photon.bounce = (uint32_t) param.photonMapBounce;
    pp.photon.radius = param.photonMapRadius;
    pp.caustics.size = (uint32_t) param.causticsMapSize;
    pp.caustics.bounce = (uint32_t) param.causticsMapBounce;
    pp.caustics.radius = param.causticsMapRadius;
    if (qa_photon_maps_build(ctx, &pp, param.seed) != QA_OK)
      throw std::runtime_error(std::string("qa_photon_maps_build: ") + qa_last_error());
    uint64_t emitted[2], emissions[2];
    qa_photon_maps_info(ctx, emitted, emissions);
    const std::chrono::duration<double> dt = std::chrono::system_clock::now() - t0;
    printf("\nPhoton Map (%zu photons, %llu emitted rays) and Caustics Map (%zu, %llu) Take %f s to Build\n", param.photonMapSize,
           (unsigned long long) emitted[0], param.causticsMapSize, (unsigned long long) emitted[1], dt.count());
  }
}

// src/renderers/renderer.cpp:42-63
void Renderer::StartTimer() { g_start = std::chrono::system_clock::now(); }
void Renderer::StopTimer()
{
  const std::chrono::duration<double> el = std::chrono::system_clock::now() - g_start;
  lastSeconds = el.count();
  printf("\nElapsed Time is %f s\n", lastSeconds);
  if (++numFrames > 0) avgSeconds += (lastSeconds - avgSeconds) / numFrames;
}
void Renderer::KillTimer() { printf("\nProgram Ends, Average Frame Time %f s\n\n", avgSeconds); }

// Renderer_MPI::Render's render + gather (Renderer_MPI.cpp:123-207) across the GPUs of this process
void Renderer::ThreadRenderMulti()
{
  StartTimer();
  const int W = (int) pixelW, H = (int) pixelH, N = (int) multi.size();
  printf("\nRunning on %d HIP device(s), 8-row strips round-robin\n", N);
  const int maxStrips = (((H + QA_STRIP_ROWS - 1) / QA_STRIP_ROWS) + N - 1) / N;
  const size_t n = (size_t) maxStrips * QA_STRIP_ROWS * W;          // pixels of a rank's packed buffer (equal for all ranks)
  const size_t words = 5 * n;                                         // rgb | depth | sample counts
  // the gather target: one packed buffer per rank, on the first device
  float *gathered = nullptr;
  HIP_OR_THROW(hipSetDevice(multi[0]));
  HIP_OR_THROW(hipMalloc((void **) &gathered, (size_t) N * words * sizeof(float)));
  memset(&counters, 0, sizeof(counters));
  std::vector<qa_counters> cnt(N);
  PerDevice((size_t) N, [&](size_t i) {
    HIP_OR_THROW(hipSetDevice(multi[i]));
    qa_ctx *c = ctxs[i];
    if (tasking::has_stop_signal()) qa_request_stop(c);
    else qa_clear_stop(c);
    qa_reset_counters(c);
    float *buf = nullptr;
    HIP_OR_THROW(hipMalloc((void **) &buf, words * sizeof(float)));
    HIP_OR_THROW(hipMemset(buf, 0, words * sizeof(float)));
    hipStream_t s = nullptr;
    HIP_OR_THROW(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (qa_strip_count(0, H, (int) i, N) > 0 &&
        qa_render_strips_device(c, 0, 0, W, H, (int) i, N, (int) param.sppMin, (int) param.sppMax, Material::maxBounce, param.seed, 0, buf, buf + 3 * n,
                                reinterpret_cast<uint32_t *>(buf + 4 * n), s) != QA_OK)
      throw std::runtime_error(std::string("qa_render_strips_device: ") + qa_last_error());
    // the strips travel to the first device right behind the kernel, on the same stream (xGMI peer copy)
    HIP_OR_THROW(hipMemcpyPeerAsync(gathered + i * words, multi[0], buf, multi[i], words * sizeof(float), s));
    HIP_OR_THROW(hipStreamSynchronize(s));
    qa_get_counters(c, &cnt[i]);
    (void) hipStreamDestroy(s);
    (void) hipFree(buf);
  });
  std::vector<float> host((size_t) N * words);
  HIP_OR_THROW(hipSetDevice(multi[0]));
  HIP_OR_THROW(hipMemcpy(host.data(), gathered, host.size() * sizeof(float), hipMemcpyDeviceToHost));
  (void) hipFree(gathered);
  for (int i = 0; i < N; ++i) {
    const float *b = host.data() + (size_t) i * words;
    PlaceStrips(*image, W, H, N, i, b, b + 3 * n, reinterpret_cast<const uint32_t *>(b + 4 * n), (int) param.sppMax, param.useSRGB);
    counters.samples += cnt[i].samples; counters.casts_normal += cnt[i].casts_normal; counters.casts_shadow += cnt[i].casts_shadow;
    counters.bvh_nodes += cnt[i].bvh_nodes; counters.tri_tests += cnt[i].tri_tests; counters.pixels += cnt[i].pixels;
  }
  StopTimer();
}

// src/renderers/renderer.cpp:370-423
void Renderer::ThreadRender()
{
  if (!multi.empty()) { ThreadRenderMulti(); return; }
  StartTimer();
  if (mpiRank == 0) printf("\nRunning on HIP device %d, rank %zu of %zu\n", device, mpiRank, mpiSize);
  const int W = (int) pixelW, H = (int) pixelH;
  if (tasking::has_stop_signal()) qa_request_stop(ctx);
  else qa_clear_stop(ctx);
  qa_reset_counters(ctx);
  if (denoise || alpha || !matteNodes.empty() || aoRays > 0) {
    // the frame stays on the device for the filter and the mattes (Render: SaveAlpha, SaveNodeMattes, SaveAo, SaveDenoised, after the timer has
    // stopped); the FrameBuffer gets the same floats qa_render_region would have copied back
    if (!multi.empty() || mpiSize != 1) throw std::runtime_error("-denoise, -alpha, -matte-node and -ao work on one device and cannot be combined with -devices");
    const size_t n = (size_t) W * H;
    denoiseFrame.Alloc(n);
    if (qa_render_region_device(ctx, 0, 0, W, H, (int) param.sppMin, (int) param.sppMax, Material::maxBounce, param.seed, 0, denoiseFrame.rgb,
                                denoiseFrame.depth, denoiseFrame.ns, nullptr) != QA_OK)
      throw std::runtime_error(std::string("qa_render_region_device: ") + qa_last_error());
    qa_synchronize(ctx);
    std::vector<float> rgb(3 * n), depth(n);
    std::vector<uint32_t> ns(n);
    HIP_OR_THROW(hipMemcpy(rgb.data(), denoiseFrame.rgb, n * 12, hipMemcpyDeviceToHost));
    HIP_OR_THROW(hipMemcpy(depth.data(), denoiseFrame.depth, n * 4, hipMemcpyDeviceToHost));
    HIP_OR_THROW(hipMemcpy(ns.data(), denoiseFrame.ns, n * 4, hipMemcpyDeviceToHost));
    image->Deposit(0, 0, W, H, rgb.data(), depth.data(), ns.data(), (int) param.sppMax, param.useSRGB);
  } else if (mpiSize == 1) {
    std::vector<float> rgb((size_t) 3 * W * H), depth((size_t) W * H);
    std::vector<uint32_t> ns((size_t) W * H);
    if (qa_render_region(ctx, 0, 0, W, H, (int) param.sppMin, (int) param.sppMax, Material::maxBounce, param.seed, 0,
                         rgb.data(), depth.data(), ns.data()) != QA_OK)
      throw std::runtime_error(std::string("qa_render_region: ") + qa_last_error());
    image->Deposit(0, 0, W, H, rgb.data(), depth.data(), ns.data(), (int) param.sppMax, param.useSRGB);
  } else {
    // rank-strided strips, like ThreadRender(tileStart = rank, step = size); this rank deposits
    // only the rows it owns (mask = 1 there), the caller gathers (Renderer_MPI::Render's PlaceImage)
    const int strips = qa_strip_count(0, H, (int) mpiRank, (int) mpiSize);
    const size_t n = (size_t) strips * QA_STRIP_ROWS * W;
    float *dRgb = nullptr, *dDepth = nullptr;
    uint32_t *dNs = nullptr;
    if (n) {
      if (hipMalloc((void **) &dRgb, n * 12) != hipSuccess || hipMalloc((void **) &dDepth, n * 4) != hipSuccess ||
          hipMalloc((void **) &dNs, n * 4) != hipSuccess)
        throw std::runtime_error("hipMalloc failed");
      if (qa_render_strips_device(ctx, 0, 0, W, H, (int) mpiRank, (int) mpiSize, (int) param.sppMin, (int) param.sppMax,
                                  Material::maxBounce, param.seed, 0, dRgb, dDepth, dNs, nullptr) != QA_OK)
        throw std::runtime_error(std::string("qa_render_strips_device: ") + qa_last_error());
      qa_synchronize(ctx);
      std::vector<float> rgb(3 * n), depth(n);
      std::vector<uint32_t> ns(n);
      (void) hipMemcpy(rgb.data(), dRgb, n * 12, hipMemcpyDeviceToHost);
      (void) hipMemcpy(depth.data(), dDepth, n * 4, hipMemcpyDeviceToHost);
      (void) hipMemcpy(ns.data(), dNs, n * 4, hipMemcpyDeviceToHost);
      for (int k = 0; k < strips; ++k) {
        const int y0 = ((int) mpiRank + k * (int) mpiSize) * QA_STRIP_ROWS;
        const int y1 = y0 + QA_STRIP_ROWS < H ? y0 + QA_STRIP_ROWS : H;
        const size_t off = (size_t) k * QA_STRIP_ROWS * W;
        image->Deposit(0, y0, W, y1, rgb.data() + 3 * off, depth.data() + off, ns.data() + off, (int) param.sppMax, param.useSRGB);
      }
      (void) hipFree(dRgb); (void) hipFree(dDepth); (void) hipFree(dNs);
    }
  }
  qa_get_counters(ctx, &counters);
  StopTimer();
}

// Renderer_MPI::Render (src/renderers/Renderer_MPI.cpp:123-139): render, then dump the three images
void Renderer::Render()
{
  ThreadRender();
  SaveImages();
  // outside the timed span: the printed time and rate are the render's, with or without the flags
  if (alpha) SaveAlpha(denoiseFrame.rgb, denoiseFrame.ns, false);   // (first: the filter works in place)
  if (!matteNodes.empty()) SaveNodeMattes(denoiseFrame.ns, false);
  if (aoRays > 0) SaveAo(denoiseFrame.ns, false);
  if (denoise) SaveDenoised(denoiseFrame.rgb, denoiseFrame.depth, denoiseFrame.ns);
  if (denoise || alpha || !matteNodes.empty() || aoRays > 0) denoiseFrame.Free();
}

// The batch counterpart of Renderer_GUI's progressive display (src/renderers/Renderer_GUI.cpp:37-97, which shows renderImage while
// the render threads fill it): the frame stays resident on the GPU (qa_progressive_*) and its samples are raised in passes of
// passSpp up to sppMax; after each pass the FrameBuffer adopts the 8-bit products the device made of the frame where it lies
// (qa_progressive_display: 7 bytes per pixel come back instead of 20, and no powf runs on the host) and the three images are written
// again.  The float depth is read after the last pass only.  The last pass leaves the one-shot frame's images, byte for byte.
void Renderer::RenderProgressive(size_t passSpp)
{
  if (!multi.empty() || mpiSize != 1) throw std::runtime_error("-progressive renders on one device and cannot be combined with -devices");
  if (passSpp < 1) throw std::runtime_error("-progressive needs passes of at least one sample");
  StartTimer();
  printf("\nRunning on HIP device %d, progressive passes of %zu spp\n", device, passSpp);
  const int W = (int) pixelW, H = (int) pixelH;
  if (tasking::has_stop_signal()) qa_request_stop(ctx);
  else qa_clear_stop(ctx);
  qa_reset_counters(ctx);
  if (qa_progressive_begin(ctx, 0, 0, W, H, (int) param.sppMin, (int) param.sppMax, Material::maxBounce, param.seed, 0) != QA_OK)
    throw std::runtime_error(std::string("qa_progressive_begin: ") + qa_last_error());
  const size_t n = (size_t) W * H;
  std::vector<uint8_t> color(3 * n), count(n), zimg(n), countimg(n), mask(n);
  if (denoise || alpha) denoiseFrame.Alloc(n);   // -denoise: the preview of each pass, filtered in place; -alpha: its colour and sample counts
                                                 // (-matte-node and -ao read the frame's own slabs: qa_progressive_idmatte_device, qa_progressive_ao_device)
  for (size_t spp = 0; spp < param.sppMax;) {
    spp = std::min(spp + passSpp, param.sppMax);
    const bool last = spp >= param.sppMax;
    const auto t0 = std::chrono::system_clock::now();
    if (qa_progressive_advance(ctx, (int) spp, nullptr) != QA_OK ||
        qa_progressive_display(ctx, param.useSRGB ? 1 : 0, color.data(), count.data(), zimg.data(), countimg.data(), mask.data(), nullptr) != QA_OK)
      throw std::runtime_error(std::string("qa_progressive: ") + qa_last_error());
    const std::chrono::duration<double, std::milli> ms = std::chrono::system_clock::now() - t0;
    int reached = 0;
    qa_progressive_status(ctx, &reached, nullptr, nullptr);
    printf("pass to %zu spp: %d spp reached, %.3f ms\n", spp, reached, ms.count());
    std::vector<float> rgb, depth;
    std::vector<uint32_t> ns;
    if (last) {   // FrameBuffer::zbuffer ends as Deposit leaves it
      rgb.resize(3 * n); depth.resize(n); ns.resize(n);
      if (qa_progressive_read(ctx, rgb.data(), depth.data(), ns.data()) != QA_OK) throw std::runtime_error(std::string("qa_progressive_read: ") + qa_last_error());
    }
    image->AdoptProducts(color.data(), count.data(), zimg.data(), countimg.data(), mask.data(), last ? depth.data() : nullptr);
    image->SaveImage((outputPrefix + "colorBuffer.png").c_str());
    image->SaveZImage((outputPrefix + "depthBuffer.png").c_str());
    image->SaveSampleCountImage((outputPrefix + "sampleBuffer.png").c_str());
    if (denoise || alpha) {
      if (qa_progressive_read_device(ctx, denoiseFrame.rgb, denoiseFrame.depth, denoiseFrame.ns, nullptr) != QA_OK)
        throw std::runtime_error(std::string("qa_progressive_read_device: ") + qa_last_error());
      if (alpha) SaveAlpha(denoiseFrame.rgb, denoiseFrame.ns, true);
      if (denoise) SaveDenoised(denoiseFrame.rgb, denoiseFrame.depth, denoiseFrame.ns);
    }
    if (!matteNodes.empty()) SaveNodeMattes(nullptr, true);
    if (aoRays > 0) SaveAo(nullptr, true);
  }
  denoiseFrame.Free();
  qa_progressive_end(ctx);
  qa_get_counters(ctx, &counters);
  StopTimer();
}

void Renderer::SaveImages()
{
  image->ComputeZBufferImage();
  image->ComputeSampleCountImage();
  image->SaveImage((outputPrefix + "colorBuffer.png").c_str());
  image->SaveZImage((outputPrefix + "depthBuffer.png").c_str());
  image->SaveSampleCountImage((outputPrefix + "sampleBuffer.png").c_str());
}

void Renderer::DeviceFrame::Alloc(size_t n)
{
  Free();
  HIP_OR_THROW(hipMalloc((void **) &rgb, n * 12));
  HIP_OR_THROW(hipMalloc((void **) &depth, n * 4));
  HIP_OR_THROW(hipMalloc((void **) &ns, n * 4));
}
void Renderer::DeviceFrame::Free()
{
  (void) hipFree(rgb); (void) hipFree(depth); (void) hipFree(ns);
  rgb = depth = nullptr;
  ns = nullptr;
}

// The frame in device buffers -> its filtered colour bytes (encoded as colorBuffer.png's are: qa_display_device honours -srgb) ->
// <prefix>denoisedBuffer.png.  Everything runs on the context's stream, behind the frame
void Renderer::SaveDenoised(float *dRgb, const float *dDepth, const uint32_t *dNs)
{
  if (!multi.empty() || mpiSize != 1) throw std::runtime_error("-denoise filters on one device and cannot be combined with -devices");
  const size_t n = pixelW * pixelH;
  qa_denoise_params dp;
  qa_denoise_params_default(&dp);
  if (denoiseIterations >= 0) dp.iterations = denoiseIterations;
  struct Bytes {   // (freed on every way out)
    uint8_t *p = nullptr;
    ~Bytes() { if (p) (void) hipFree(p); }
  } dColor;
  HIP_OR_THROW(hipMalloc((void **) &dColor.p, 3 * n));
  if (denoiseGuided) {   // -denoise-guided: the frame's first-hit normal and albedo planes (sample 0 of the frame's seed) guide the filter
    Bytes dGuides;
    HIP_OR_THROW(hipMalloc((void **) &dGuides.p, 24 * n));
    float *dNormal = reinterpret_cast<float *>(dGuides.p), *dAlbedo = dNormal + 3 * n;
    qa_denoise_guided_params gp;
    qa_denoise_guided_params_default(&gp);
    if (denoiseIterations >= 0) gp.iterations = denoiseIterations;
    if (qa_gbuffer_region_device(ctx, 0, 0, (int) pixelW, (int) pixelH, param.seed, dNormal, dAlbedo, nullptr, nullptr, nullptr) != QA_OK ||
        qa_denoise_guided_device(ctx, dRgb, dDepth, dNs, dNormal, dAlbedo, (int) pixelW, (int) pixelH, &gp, dRgb, nullptr) != QA_OK)
      throw std::runtime_error(std::string("-denoise-guided: ") + qa_last_error());
    qa_synchronize(ctx);   // (the guide planes are freed on the way out)
  }
  if ((!denoiseGuided && qa_denoise_device(ctx, dRgb, dDepth, dNs, (int) pixelW, (int) pixelH, &dp, dRgb, nullptr) != QA_OK) ||
      qa_display_device(ctx, dRgb, dDepth, dNs, n, (int) param.sppMax, param.useSRGB ? 1 : 0, dColor.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != QA_OK)
    throw std::runtime_error(std::string("-denoise: ") + qa_last_error());
  qa_synchronize(ctx);
  std::vector<uint8_t> color(3 * n);
  HIP_OR_THROW(hipMemcpy(color.data(), dColor.p, 3 * n, hipMemcpyDeviceToHost));
  SavePNG((outputPrefix + "denoisedBuffer.png").c_str(), color.data(), (int) pixelW, (int) pixelH, 3);
}

// The frame's colour and sample counts in device buffers -> coverage and backdrop of exactly the samples each pixel holds (the
// progressive frame's own call while one is open, else the region call with the frame's ns plane) -> straight-alpha bytes ->
// <prefix>rgbaBuffer.png.  Everything runs on the context's stream, behind the frame
void Renderer::SaveAlpha(const float *dRgb, const uint32_t *dNs, bool progressive)
{
  if (!multi.empty() || mpiSize != 1) throw std::runtime_error("-alpha makes its image on one device and cannot be combined with -devices");
  const size_t n = pixelW * pixelH;
  struct Bytes {   // (freed on every way out)
    uint8_t *p = nullptr;
    ~Bytes() { if (p) (void) hipFree(p); }
  } dPlanes;
  HIP_OR_THROW(hipMalloc((void **) &dPlanes.p, 20 * n));   // [backdrop 12 | coverage 4 | rgba 4] bytes per pixel
  float *dBackdrop = reinterpret_cast<float *>(dPlanes.p), *dCoverage = dBackdrop + 3 * n;
  uint8_t *dRgba = reinterpret_cast<uint8_t *>(dCoverage + n);
  const int rc = progressive ? qa_progressive_matte_device(ctx, dCoverage, nullptr, nullptr, dBackdrop, nullptr)
                             : qa_matte_region_device(ctx, 0, 0, (int) pixelW, (int) pixelH, (uint32_t) param.sppMax, dNs, dCoverage, nullptr, nullptr,
                                                      dBackdrop, nullptr);
  if (rc != QA_OK || qa_matte_rgba_device(ctx, dRgb, dBackdrop, dCoverage, dNs, n, param.useSRGB ? 1 : 0, dRgba, nullptr) != QA_OK)
    throw std::runtime_error(std::string("-alpha: ") + qa_last_error());
  qa_synchronize(ctx);
  std::vector<uint8_t> rgba(4 * n);
  HIP_OR_THROW(hipMemcpy(rgba.data(), dRgba, 4 * n, hipMemcpyDeviceToHost));
  if (!SavePNG((outputPrefix + "rgbaBuffer.png").c_str(), rgba.data(), (int) pixelW, (int) pixelH, 4))
    throw std::runtime_error("-alpha: " + outputPrefix + "rgbaBuffer.png could not be written");
}

// The id matte of exactly the samples each pixel holds (the progressive frame's own call while one is open, else the region call
// with the frame's ns plane), once; then per -matte-node NAME the coverage of that node as 8-bit grey -> <prefix>matte_NAME.png.
// Everything runs on the context's stream, behind the frame
void Renderer::SaveNodeMattes(const uint32_t *dNs, bool progressive)
{
  if (!multi.empty() || mpiSize != 1) throw std::runtime_error("-matte-node makes its images on one device and cannot be combined with -devices");
  const size_t n = pixelW * pixelH;
  struct Bytes {   // (freed on every way out)
    uint8_t *p = nullptr;
    ~Bytes() { if (p) (void) hipFree(p); }
  } dPlanes;
  HIP_OR_THROW(hipMalloc((void **) &dPlanes.p, 69 * n));   // [ids 32 | counts 32 | samples 4 | grey 1] bytes per pixel
  int32_t *dIds = reinterpret_cast<int32_t *>(dPlanes.p);
  uint32_t *dCounts = reinterpret_cast<uint32_t *>(dIds + 8 * n), *dSamples = dCounts + 8 * n;
  uint8_t *dGrey = reinterpret_cast<uint8_t *>(dSamples + n);
  const int rc = progressive ? qa_progressive_idmatte_device(ctx, QA_IDMATTE_NODE, dIds, dCounts, nullptr, dSamples, nullptr)
                             : qa_idmatte_region_device(ctx, 0, 0, (int) pixelW, (int) pixelH, (uint32_t) param.sppMax, dNs, QA_IDMATTE_NODE, dIds, dCounts,
                                                        nullptr, dSamples, nullptr);
  if (rc != QA_OK) throw std::runtime_error(std::string("-matte-node: ") + qa_last_error());
  std::vector<uint8_t> grey(n);
  for (const std::pair<std::string, int> &node : matteNodes) {
    const int32_t id = node.second;
    if (qa_idmatte_select_device(ctx, dIds, dCounts, dSamples, n, &id, 1, nullptr, dGrey, nullptr) != QA_OK)
      throw std::runtime_error(std::string("-matte-node: ") + qa_last_error());
    qa_synchronize(ctx);
    HIP_OR_THROW(hipMemcpy(grey.data(), dGrey, n, hipMemcpyDeviceToHost));
    const std::string path = outputPrefix + "matte_" + node.first + ".png";
    if (!SavePNG(path.c_str(), grey.data(), (int) pixelW, (int) pixelH, 1)) throw std::runtime_error("-matte-node: " + path + " could not be written");
  }
}

// The ambient occlusion of exactly the samples each pixel holds (the progressive frame's own call while one is open, else the region
// call with the frame's ns plane and seed), as 8-bit grey -> <prefix>aoBuffer.png.  Everything runs on the context's stream, behind the frame
void Renderer::SaveAo(const uint32_t *dNs, bool progressive)
{
  if (!multi.empty() || mpiSize != 1) throw std::runtime_error("-ao makes its image on one device and cannot be combined with -devices");
  const size_t n = pixelW * pixelH;
  struct Bytes {   // (freed on every way out)
    uint8_t *p = nullptr;
    ~Bytes() { if (p) (void) hipFree(p); }
  } dPlanes;
  HIP_OR_THROW(hipMalloc((void **) &dPlanes.p, 5 * n));   // [ao 4 | grey 1] bytes per pixel
  float *dAo = reinterpret_cast<float *>(dPlanes.p);
  uint8_t *dGrey = reinterpret_cast<uint8_t *>(dAo + n);
  const int rc = progressive ? qa_progressive_ao_device(ctx, (uint32_t) aoRays, aoRadius, nullptr, nullptr, dAo, nullptr)
                             : qa_ao_region_device(ctx, 0, 0, (int) pixelW, (int) pixelH, 0, (uint32_t) param.sppMax, dNs, (uint32_t) aoRays, aoRadius,
                                                   param.seed, nullptr, nullptr, dAo, nullptr);
  if (rc != QA_OK || qa_ao_grey_device(ctx, dAo, n, dGrey, nullptr) != QA_OK) throw std::runtime_error(std::string("-ao: ") + qa_last_error());
  qa_synchronize(ctx);
  std::vector<uint8_t> grey(n);
  HIP_OR_THROW(hipMemcpy(grey.data(), dGrey, n, hipMemcpyDeviceToHost));
  const std::string path = outputPrefix + "aoBuffer.png";
  if (!SavePNG(path.c_str(), grey.data(), (int) pixelW, (int) pixelH, 1)) throw std::runtime_error("-ao: " + path + " could not be written");
}

void Renderer::Terminate()
{
  for (qa_ctx *&c : ctxs) if (c) { qa_ctx_destroy(c); c = nullptr; }
  if (ctx) { qa_ctx_destroy(ctx); ctx = nullptr; }
}

}  // namespace qaray_hip
