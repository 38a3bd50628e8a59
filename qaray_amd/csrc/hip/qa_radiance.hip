// qa_radiance.hip — radiance along rays of the caller's (qa_radiance_rays*): the per-lane integrator of qa_kernel.h started from a
// ray batch instead of the camera, its ten instances and their picker; and the renderer's own camera rays of every sample handed
// out (qa_camera_sample_rays_device).  A unit of its own, as qa_lastcast.hip: the kernels are compiled side by side with the
// shipped integrators, which keep their names, resources and code.  No reference counterpart (the reference path-traces only the
// rays of its own camera); what ties it to the reference is that the renderer's own camera rays, handed back in, give the frame.
//
// SEMANTICS
// A ray is an origin o and a direction d, both world space, fp32.  d is used as given and is NOT normalised (shading assumes unit
// length, as for a camera ray): the renderer's own rays pass through bit for bit.  Ray q of a batch of n is the first segment of
// spp paths; what follows the first segment is the integrator's, unchanged (qa_kernel_body.h sections C - E: the closest-hit sweep,
// shading, direct light, the bounces, the running mean with its correctly rounded divisions).  The result of a ray depends on the
// ray (with its differentials and screen position), its stream id, the seed, spp and max_bounce alone: not on n, on the ray's place
// in the batch or on what else the batch holds.
//   Rays per sample: by default sample s of ray q starts from record q of every ray array; with QA_RADIANCE_PER_SAMPLE from record
//     q * spp + s (arrays of n * spp records): jittered or lens-sampled rays of the caller's own making.
//   Random numbers: ray q draws from the stream qa_pixel_seed(seed, stream[q]), or qa_pixel_seed(seed, q) without stream ids; the
//     samples of a ray continue one stream, as the samples of a pixel do.  The first segment draws nothing (no lens, no jitter).
//   Differentials (textured scenes): dx / dy are the directions of the ray through the neighbouring pixel samples, DiffRay's x and
//     y; both or neither.  Without them dx = dy = d, a ray of no width, the DiffRay(pos, dir) of a bounce ray: at the first hit
//     the texture filter then takes its unfiltered branch (textureSampleFiltered, `filtered == false`: one unfiltered lookup), so a
//     textured surface seen through such rays differs from the frame's filtered lookup.
//   A first ray that misses takes the background colour, as a frame's camera ray does; a background texmap is looked up at the
//     ray's screen position (screen[2 r], screen[2 r + 1], in pixels: divided by the image's width and height).  A scene whose
//     background has a texmap is refused with QA_EINVAL when neither screen positions nor QA_RADIANCE_MISS_ENVIRONMENT are given:
//     nothing is approximated silently.  With QA_RADIANCE_MISS_ENVIRONMENT it takes the environment by direction
//     (sampleEnvironment), as every bounce ray does.
//   Void rays: a (ray, sample) record is void if any component of o or d is not finite, or if d == (0, 0, 0) (as qa_ray_query.hip).
//     It is not walked and draws nothing from the stream; the sample is black and counts as a sample.
//   Outputs, indexed by ray: rgb [n][3] the mean over the spp samples; t [n] (optional) the parameter of sample 0's first hit, 1e30
//     on a miss and for a void ray; ns [n] uint32 (optional) the samples taken: zeroed first, spp once the ray is finished - a ray
//     that a stop request left unfinished reads 0, and its rgb is not written.
//   spp is fixed: no adaptive stop (the running variance of a batch ray stops nothing).
//   The camera is not read.  Area lights: max_bounce <= 7, as for a frame.  Photon maps: with QA_RADIANCE_PHOTON_MAPS the batch runs
//     with Scene::usePhotonMap = true on the gathering instances of qa_radiance_pm.hip (whose opening comment says the rest); without
//     the flag a context whose maps are built is refused (QA_EUNSUPPORTED), with it one without maps (QA_ENOSCENE).
//   State: the call is ordered as a frame is (behind the context's last frame and last edit, one at a time per context), adds to
//     qa_get_counters (samples += n * spp, the casts of its paths) and to qa_get_kernel_time (one launch) as a frame does, and
//     leaves qa_get_kernel_name, progressive frames and the frames' slabs alone.
//
// qa_camera_sample_rays_device: samples [first, first + count) of the camera rays of the pixels of a region, exactly as
// qa_kernel_body.h section B builds them: texpos = (halton[2 s], halton[2 s + 1]) + (px, py), the point (A + U x) + V y of the
// image plane, d = normalize(point - position), and for the differentials the same point with x + QA_DX and with y + QA_DX.  Record
// (pixel, k) is at pixel * count + k, pixels region-local and row-major; stream ids are one per pixel, py * width + px.
// Handed to qa_radiance_rays_device with QA_RADIANCE_PER_SAMPLE (first = 0, count = spp) they give qa_render_region's rgb, depth
// and ns bit for bit.  A camera with dof > 0.1 is refused (QA_EUNSUPPORTED): its two lens draws come from the pixel's stream
// between a sample's paths, in the middle of the stream - no ray array can carry them, and a frame of such a camera cannot be
// reproduced from outside.
//
// Shape: a work item is 64 consecutive rays, lane = ray, handed out by the frame's work counter (a stop request ends the batch
// between items).  No tiles: no tile order, no strips, no tile lists, no sample chunks; the last-cast query of
// qa_integrate_lastcast is not carried over.  Every mesh is walked per lane (no cooperative walks), rays are taken in the caller's
// order (not sorted).
#include <algorithm>
#include <cstring>

#include "qa_firsthit.h"
#include "qa_raybatch.h"
#include "qa_stage.h"

static_assert(QA_RAYS_PER_SAMPLE == QA_RADIANCE_PER_SAMPLE && QA_RAYS_MISS_ENVIRONMENT == QA_RADIANCE_MISS_ENVIRONMENT, "RayBatch::flags are the C ABI's");

namespace qa {

struct CamSampleParams {
  int32_t x0, y0, x1, y1;
  int32_t first, count;
  float *o, *d, *dx, *dy;   // [pixels * count][3] each; any may be null
  float *screen;            // [pixels * count][2]
  uint32_t *stream;         // [pixels]
};

// One thread per (pixel, sample); reads the camera record and the Halton table only
__global__ __launch_bounds__(QA_BLOCK) void qa_camera_sample_rays(const DCamera cam, const float *halton, const CamSampleParams cs)
{
  const uint64_t rw = (uint64_t) (cs.x1 - cs.x0), nrec = rw * (uint64_t) (cs.y1 - cs.y0) * (uint64_t) cs.count;
  const uint64_t i = (uint64_t) blockIdx.x * QA_BLOCK + threadIdx.x;
  if (i >= nrec) return;
  const uint64_t q = i / (uint64_t) cs.count;
  const int k = (int) (i % (uint64_t) cs.count), si = cs.first + k;
  const int px = cs.x0 + (int) (q % rw), py = cs.y0 + (int) (q / rw);

  // (pinhole: a camera with dof > 0.1 is refused by the host)
  const f3 texpos = camTexpos(halton, si, px, py);
  const f3 campos = ld3(cam.pos);
  const f3 dir = normalize(camPoint(cam, texpos.x, texpos.y) - campos);
  if (cs.o) { cs.o[3 * i] = campos.x; cs.o[3 * i + 1] = campos.y; cs.o[3 * i + 2] = campos.z; }
  if (cs.d) { cs.d[3 * i] = dir.x; cs.d[3 * i + 1] = dir.y; cs.d[3 * i + 2] = dir.z; }
  if (cs.dx) {
    const f3 v = normalize(camPoint(cam, texpos.x + QA_DX, texpos.y) - campos);
    cs.dx[3 * i] = v.x; cs.dx[3 * i + 1] = v.y; cs.dx[3 * i + 2] = v.z;
  }
  if (cs.dy) {
    const f3 v = normalize(camPoint(cam, texpos.x, texpos.y + QA_DX) - campos);
    cs.dy[3 * i] = v.x; cs.dy[3 * i + 1] = v.y; cs.dy[3 * i + 2] = v.z;
  }
  if (cs.screen) { cs.screen[2 * i] = texpos.x; cs.screen[2 * i + 1] = texpos.y; }
  if (cs.stream && k == 0) cs.stream[q] = (uint32_t) py * (uint32_t) cam.width + (uint32_t) px;
}

}  // namespace qa

// ---- the ten instances: qa_integrate_rays<RES, LIGHTS, TEX, AREA> by the picker, the checks and the launch of qa_raybatch.h
QA_DEFINE_RAYS_PICKER(PickRays, qa_integrate_rays)

// (QA_RADIANCE_PHOTON_MAPS: the batch runs on the gathering family, qa_radiance_pm.hip; RayBatch::flags keeps the two bits it knows)
#define QA_RADIANCE_FLAGS (QA_RADIANCE_PER_SAMPLE | QA_RADIANCE_MISS_ENVIRONMENT | QA_RADIANCE_PHOTON_MAPS)
#define QA_RAYBATCH_FLAGS (QA_RADIANCE_PER_SAMPLE | QA_RADIANCE_MISS_ENVIRONMENT)
static RaysFn PickFor(const qa_ctx *c, const qa_radiance_params *p) { return WantsPhotonMaps(p) ? PickRaysPm(c) : PickRays(c); }

extern "C" {

int qa_radiance_params_default(qa_radiance_params *params)
{
  if (!params) return Fail(QA_EINVAL, "null argument");
  params->spp = 1;
  params->max_bounce = 5;
  params->seed = 0x51A7A7u;
  params->flags = 0;
  return QA_OK;
}

int qa_radiance_rays_device(qa_ctx *c, uint64_t n, const float *d_origins, const float *d_dirs, const float *d_dx, const float *d_dy,
                            const float *d_screen, const uint32_t *d_stream, const qa_radiance_params *params, float *d_rgb, float *d_t,
                            uint32_t *d_ns, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = RayBatchChecks(c, n, d_origins && d_dirs, d_dx != nullptr, d_dy != nullptr, d_screen != nullptr, params, d_rgb != nullptr, QA_RADIANCE_FLAGS, true)) return rc;
  if (n == 0) return QA_OK;
  const RayBatch rb = {d_origins, d_dirs, d_dx, d_dy, d_screen, d_stream, (uint32_t) n, params->flags & QA_RAYBATCH_FLAGS};
  return LaunchRayBatch(c, PickFor(c, params), n, rb, *params, d_rgb, d_t, d_ns, StreamOf(c, hip_stream));
}

int qa_radiance_rays(qa_ctx *c, uint64_t n, const float *origins, const float *dirs, const float *dx, const float *dy, const float *screen,
                     const uint32_t *stream, const qa_radiance_params *params, float *rgb, float *t, uint32_t *ns)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = RayBatchChecks(c, n, origins && dirs, dx != nullptr, dy != nullptr, screen != nullptr, params, rgb != nullptr, QA_RADIANCE_FLAGS, true)) return rc;
  if (n == 0) return QA_OK;
  // the ray arrays hold a record per ray, or per ray and sample; dx and dy come both or neither (RayBatchChecks)
  const uint64_t r = n * ((params->flags & QA_RADIANCE_PER_SAMPLE) ? (uint64_t) params->spp : 1ull);
  QueryStage st(c);
  const auto dO = st.In(origins, 3 * r), dD = st.In(dirs, 3 * r), dDx = st.In(dx, 3 * r), dDy = st.In(dy, 3 * r), dScreen = st.In(screen, 2 * r);
  const auto dStream = st.In(stream, n);
  const auto dRgb = st.Out(rgb, 3 * n), dT = st.Out(t, n);
  const auto dNs = st.Out(ns, n);
  if (int rc = st.Begin()) return rc;
  const RayBatch rb = {st(dO), st(dD), st(dDx), st(dDy), st(dScreen), st(dStream), (uint32_t) n, params->flags & QA_RAYBATCH_FLAGS};
  if (int rc = LaunchRayBatch(c, PickFor(c, params), n, rb, *params, st(dRgb), st(dT), st(dNs), c->stream)) return rc;
  if (int rc = st.End()) return rc;
  return DrainEvents(c);   // the batch is complete: fold its event pair into the kernel time
}

int qa_camera_sample_rays_device(qa_ctx *c, int x0, int y0, int x1, int y1, int first, int count, float *d_origins, float *d_dirs, float *d_dx,
                                 float *d_dy, float *d_screen, uint32_t *d_stream, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = CheckRegion(c, x0, y0, x1, y1)) return rc;
  if (first < 0 || count < 1 || (long long) first + count > 0x7FFFFFFFll) return Fail(QA_EINVAL, "bad sample range");
  if (!d_origins && !d_dirs && !d_dx && !d_dy && !d_screen && !d_stream) return Fail(QA_EINVAL, "no output");
  if (c->ds.cam.dof > 0.1f)
    return Fail(QA_EUNSUPPORTED, "depth of field: the lens draws come from the pixel's stream between a sample's paths; no ray array can carry them");
  const uint64_t nrec = (uint64_t) (x1 - x0) * (uint64_t) (y1 - y0) * (uint64_t) count;
  if (nrec > QA_MAX_RAYS) return Fail(QA_EINVAL, "more than 2^31 - 1 rays");
  if (int rc = EnsureHalton(c, first + count)) return rc;
  const hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(c->lastFrame.WaitOn(s));
  HIP_TRY(c->lastEdit.WaitOn(s));
  const CamSampleParams cs = {x0, y0, x1, y1, first, count, d_origins, d_dirs, d_dx, d_dy, d_screen, d_stream};
  hipLaunchKernelGGL(qa_camera_sample_rays, dim3((unsigned) ((nrec + QA_BLOCK - 1) / QA_BLOCK)), dim3(QA_BLOCK), 0, s, c->ds.cam, c->ds.halton, cs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(c->lastFrame.Record(s));
  return QA_OK;
}

}  // extern "C"
