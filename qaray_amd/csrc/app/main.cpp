// qaray_hip — batch driver with the reference's command line (src/main.cpp:8-62):
//   qaray_hip [-batch] [-spp N] [-sppMin N] [-sppMax N] [-bounce N] [-srgb 0|1] [-threads N]
//             [-use-photon-map] [-photon-map-size N] [-caustics-map-size N] scene.xml
// plus what the reference has no flag for: -size W H, -seed S, -device D, -devices N (GPUs 0..N-1 of this node in one
// process: one host thread and one context per GPU, strips gathered on the first; Renderer::UseDevices), -out PREFIX, -root DIR,
// -photon-map-radius R, -caustics-map-radius R, -photon-map-bounce N, -caustics-map-bounce N, -progressive N (the frame in passes of
// N spp up to -spp / -sppMax, the images rewritten after each: the batch counterpart of the reference's progressive display),
// -denoise [N] (a fourth image, <prefix>denoisedBuffer.png: the frame filtered on the device with N iterations - default the
// library's - and encoded as colorBuffer.png is; with -progressive rewritten after each pass; the other three images do not change.
// N is optional: an argument made of digits alone right after -denoise is taken as N, so a scene file with such a name goes elsewhere
// on the line or is written ./123), -denoise-guided [N] (as -denoise, through the guided filter with the frame's first-hit normal
// and albedo planes; the same file), -alpha (a fourth image, <prefix>rgbaBuffer.png: the frame with straight alpha, 4 channels - alpha is
// the fraction of a pixel's camera rays that hit something, the colour the frame's without the backdrop's part; made on the device from
// the frame's own sample counts (qa_matte_region_device, qa_matte_rgba_device); with -progressive rewritten after each pass; the other
// three images do not change.  Not with -devices, and not for a camera with depth of field: refused before anything is rendered),
// -matte-node NAME (may be given more than once; per NAME an image, <prefix>matte_NAME.png, 8-bit grey: the fraction of a pixel's samples
// whose camera ray meets the node with that XML name first - an anti-aliased matte of the object; made on the device from the frame's own
// sample counts (qa_idmatte_region_device, qa_idmatte_select_device); rewritten after each pass of -progressive; the other images do not
// change.  Refused as -alpha is, and when no node has the name), -ao [K] and -ao-radius R (an image, <prefix>aoBuffer.png, 8-bit grey: the
// ambient occlusion of what the frame's own samples see - of K rays, default 4, over the facing side of every camera hit the fraction
// that meets nothing within R, default unbounded; made on the device with the frame's seed and sample counts (qa_ao_region_device,
// qa_ao_grey_device); K is optional as -denoise's N is; rewritten after each pass of -progressive; the other images do not change.
// Refused as -alpha is).
// The reference's `-sppMax` sets sppMin by mistake (main.cpp:27-28); here it sets sppMax.
// Flow: Init -> LoadScene -> ComputeScene -> Render -> Terminate (main.cpp:55-59).
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "renderer.h"

using namespace qaray_hip;

int main(int argc, char **argv)
{
  setenv("GPU_MAX_HW_QUEUES", "8", 0);   // the staged integrator's tile groups each want a hardware queue (qa_wf.hip)
  RendererParam param;
  const char *file = nullptr;
  std::string out, root;
  int device = 0, w = -1, h = -1, devices = 0, progressive = 0, denoiseIterations = -1;
  bool denoise = false, denoiseGuided = false, alpha = false;
  std::vector<std::string> matteNodes;
  int aoRays = 0;
  float aoRadius = std::numeric_limits<float>::infinity();
  bool aoRadiusGiven = false;
  if (argc < 2) { fprintf(stderr, "Error: insufficient input\n"); return -1; }
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    auto next = [&]() { return (i + 1 < argc) ? argv[++i] : "0"; };
    if (s == "-batch") {}
    else if (s == "-spp") { const int t = atoi(next()); param.SetSPPMax(t); param.SetSPPMin(t); }
    else if (s == "-sppMin") param.SetSPPMin(atoi(next()));
    else if (s == "-sppMax") param.SetSPPMax(atoi(next()));
    else if (s == "-bounce") Material::maxBounce = atoi(next());
    else if (s == "-srgb") param.SetSRGBFlag(atoi(next()) != 0);
    else if (s == "-threads") (void) next();  // CPU thread count has no meaning here
    else if (s == "-use-photon-map") param.SetPhotonMappingFlag(true);
    else if (s == "-photon-map-size") param.SetPhotonMapSize((size_t) atoi(next()));
    else if (s == "-caustics-map-size") param.SetCausticsMapSize((size_t) atoi(next()));
    else if (s == "-photon-map-radius") param.SetPhotonMapRadius((float) atof(next()));
    else if (s == "-caustics-map-radius") param.SetCausticsMapRadius((float) atof(next()));
    else if (s == "-photon-map-bounce") param.SetPhotonMapBounce((size_t) atoi(next()));
    else if (s == "-caustics-map-bounce") param.SetCausticsMapBounce((size_t) atoi(next()));
    else if (s == "-size") { w = atoi(next()); h = atoi(next()); }
    else if (s == "-seed") param.seed = (uint32_t) strtoul(next(), nullptr, 0);
    else if (s == "-device") device = atoi(next());
    else if (s == "-devices") devices = atoi(next());
    else if (s == "-progressive") progressive = atoi(next());
    else if (s == "-denoise" || s == "-denoise-guided") {   // the iteration count is optional: taken when the next argument is a number
      denoise = true;
      denoiseGuided = s == "-denoise-guided";
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' && std::string(argv[i + 1]).find_first_not_of("0123456789") == std::string::npos)
        denoiseIterations = atoi(argv[++i]);
    }
    else if (s == "-alpha") alpha = true;
    else if (s == "-matte-node") { if (i + 1 < argc) matteNodes.push_back(argv[++i]); else { fprintf(stderr, "Error: -matte-node needs a node's name\n"); return -1; } }
    else if (s == "-ao") {   // the ray count is optional: taken when the next argument is a number
      aoRays = 4;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' && std::string(argv[i + 1]).find_first_not_of("0123456789") == std::string::npos)
        aoRays = atoi(argv[++i]);
      if (aoRays < 1 || aoRays > QA_AO_MAX_RAYS) { fprintf(stderr, "Error: -ao takes 1 .. %d rays per hit\n", QA_AO_MAX_RAYS); return -1; }
    }
    else if (s == "-ao-radius") {
      aoRadius = (float) atof(next());
      aoRadiusGiven = true;
      if (!(aoRadius > 0.005f)) { fprintf(stderr, "Error: -ao-radius must exceed the renderer's bias, 0.005\n"); return -1; }
    }
    else if (s == "-out") out = next();
    else if (s == "-root") root = next();
    else file = argv[i];
  }
  if (!file) { fprintf(stderr, "Error: no scene file\n"); return -1; }
  if (progressive > 0 && devices > 0) { fprintf(stderr, "Error: -progressive renders on one device and cannot be combined with -devices\n"); return -1; }
  if (denoise && devices > 0) { fprintf(stderr, "Error: -denoise filters on one device and cannot be combined with -devices\n"); return -1; }
  if (alpha && devices > 0) { fprintf(stderr, "Error: -alpha makes its image on one device and cannot be combined with -devices\n"); return -1; }
  if (!matteNodes.empty() && devices > 0) { fprintf(stderr, "Error: -matte-node makes its images on one device and cannot be combined with -devices\n"); return -1; }
  if (aoRays > 0 && devices > 0) { fprintf(stderr, "Error: -ao makes its image on one device and cannot be combined with -devices\n"); return -1; }
  if (aoRadiusGiven && aoRays == 0) { fprintf(stderr, "Error: -ao-radius without -ao\n"); return -1; }
  try {
    Renderer renderer(param, device);
    renderer.aoRays = aoRays;
    renderer.aoRadius = aoRadius;
    renderer.alpha = alpha;
    renderer.denoise = denoise;
    renderer.denoiseIterations = denoiseIterations;
    renderer.denoiseGuided = denoiseGuided;
    if (devices > 0) {
      std::vector<int> ids;
      for (int d = 0; d < devices; ++d) ids.push_back(device + d);
      renderer.UseDevices(ids);
    }
    renderer.outputPrefix = out;
    renderer.Init();
    Scene scene;
    scene.assetRoot = root;
    if (!scene.assetRoot.empty() && scene.assetRoot.back() != '/') scene.assetRoot += '/';
    LoadSceneInSilentMode(false);
    if (!LoadScene(file, scene)) { fprintf(stderr, "Failed to load %s\n", file); return 1; }
    if (w > 0 && h > 0) { scene.camera.imgWidth = w; scene.camera.imgHeight = h; }
    if (alpha && scene.camera.depthOfField > 0.1f) {   // (the library's own threshold: qa_matte_region_device refuses such a camera)
      fprintf(stderr, "Error: -alpha needs a pinhole camera: with depth of field the samples' camera rays cannot be cast again\n");
      return 1;
    }
    if (!matteNodes.empty() && scene.camera.depthOfField > 0.1f) {   // (qa_idmatte_region_device refuses such a camera too)
      fprintf(stderr, "Error: -matte-node needs a pinhole camera: with depth of field the samples' camera rays cannot be cast again\n");
      return 1;
    }
    if (aoRays > 0 && scene.camera.depthOfField > 0.1f) {   // (qa_ao_region_device refuses such a camera too)
      fprintf(stderr, "Error: -ao needs a pinhole camera: with depth of field the samples' camera rays cannot be cast again\n");
      return 1;
    }
    for (const std::string &name : matteNodes) {
      const int index = FindNodeIndex(scene, name.c_str());
      if (index < 0) { fprintf(stderr, "Error: -matte-node %s: the scene has no node of that name\n", name.c_str()); return 1; }
      renderer.matteNodes.emplace_back(name, index);
    }
    renderer.ComputeScene(renderImage, scene);
    if (progressive > 0) renderer.RenderProgressive((size_t) progressive);
    else renderer.Render();
    const qa_counters &c = renderer.Counters();
    printf("samples %llu  casts %llu + %llu shadow  %.3f Msamples/s\n", (unsigned long long) c.samples,
           (unsigned long long) c.casts_normal, (unsigned long long) c.casts_shadow, c.samples / renderer.LastSeconds() * 1e-6);
    renderer.KillTimer();
    renderer.Terminate();
  } catch (const std::exception &e) {
    fprintf(stderr, "qaray_hip: %s\n", e.what());
    return 2;
  }
  return 0;
}
