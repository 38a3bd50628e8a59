// qa_irradiance.hip — light arriving at surface points of the caller's (qa_irradiance_points*): the per-lane integrator of qa_kernel.h
// started from a surface point instead of a ray or the camera, its ten instances and their picker.  A unit of its own, as
// qa_radiance.hip: the kernels are compiled side by side with the shipped integrators and with qa_integrate_rays, which keep their
// names, resources and code.  No reference counterpart (the reference shades only what its camera rays hit); what ties it to the
// reference is the anchor below: on a white diffuse surface it is what qa_radiance_rays returns for a ray that hits that surface.
//
// SEMANTICS
// A point is a position P and a normal N, both world space, fp32; N is used as given and is NOT normalised (shading assumes unit
// length, as of a hit's normal).  Point q of a batch of n is shaded spp times as section D of qa_kernel_body.h would shade a hit at P
// with normal N on a white diffuse material, seen along the normal from the front: the direct light at P, one cosine-weighted bounce
// flagged fromDiffuse, and the integrator as it stands behind that bounce (sections C - E: the closest-hit sweep, shading, direct
// light, the bounces, the running mean with its correctly rounded divisions).  kd * result is therefore what the renderer shows for
// a diffuse surface of colour kd at P, in the renderer's own units: the values are not scaled by pi, and each light is weighted
// 1 / num_lights as directLight weights it.  The result of a point depends on the point, its normal, its stream id, the seed, spp
// and max_bounce alone: not on n, on the point's place in the batch or on what else the batch holds.
//   Sample s of point q:
//     Start state: L = 0, T = 1, bounce = max_bounce, fromDiffuse = false, absorbMtl = -1, the area-light log empty.  No first
//       segment is traced, and nothing is cast to reach P.
//     Shading: shadeSurface<false> on the material record {diffuse (1, 1, 1), everything else 0, no texmaps, flags 0} with N,
//       V = N, front = true, bounceLeft = max_bounce: the lobe draw and its select test included; a spawn takes the two draws of
//       CosWeightedHemisphere, and bxdf = kd.
//     Direct light: section D's directLight(P, N, V = N, kd, ks = 0, gloss = 0), added before T *= bxdf; in the AREA variants it
//       is record 0 of the log and is replayed last.
//     Bounce: a spawned ray starts at P with primary = false and fromDiffuse = true; sections C - E run unchanged from there.  A
//       bounce that misses takes the environment (by direction, sampleEnvironment).  With max_bounce = 0 nothing is spawned: the
//       sample is the direct light alone.
//   Random numbers: point q draws from the stream qa_pixel_seed(seed, stream[q]), or qa_pixel_seed(seed, q) without stream ids; the
//     samples of a point continue one stream, as the samples of a pixel do.
//   Void points: a point is void if any component of P or N is not finite, or if N == (0, 0, 0).  Its samples draw nothing from
//     the stream, are black, and count.
//   Outputs, indexed by point: rgb [n][3] the mean over the spp samples (the body's own running mean); ns [n] uint32 (optional) the
//     samples taken: zeroed first, spp once the point is finished - a point that a stop request left unfinished reads 0, and its
//     rgb is not written.  There is no t output.
//   spp is fixed: no adaptive stop.  The camera is not read.  Area lights: max_bounce <= 7, as for a frame.  flags must be 0 or
//     QA_RADIANCE_PHOTON_MAPS.  Photon maps: with the flag the batch runs with Scene::usePhotonMap = true on the gathering instances
//     of qa_irradiance_pm.hip (whose opening comment specifies the gather at the point); without it a context whose maps are built
//     is refused (QA_EUNSUPPORTED), with it one without maps (QA_ENOSCENE).
//   State: as qa_radiance_rays_device - ordered as a frame is (behind the context's last frame and last edit, one at a time per
//     context), adds to qa_get_counters (samples += n * spp and the casts of its paths: a sample's first segment casts nothing) and
//     to qa_get_kernel_time (one launch), and leaves qa_get_kernel_name, progressive frames and the frames' slabs alone.
//
// The anchor: on a scene whose material m is that white record, a ray that hits m on a front face at (P, N) gives, through
// qa_radiance_rays with QA_RADIANCE_MISS_ENVIRONMENT, the bits qa_irradiance_points gives at (P, N) with the same stream id,
// seed, spp and max_bounce: the ray's first segment draws nothing, V enters the white record's shading nowhere (ks = 0, no lobes),
// and everything behind the hit is the same text (tests/test_gpu_irradiance.py).
//
// Shape: qa_integrate_rays' (qa_radiance.hip) - a work item is 64 consecutive points, lane = point, handed out by the frame's work
// counter; padding lanes of the last item sit it out.  No tiles, no sorting: points are taken in the caller's order, every mesh is
// walked per lane.  A lightmap's rows against the frame's 8 x 8 tiles may cost coherence; recorded, not tuned.
#include "qa_firsthit.h"
#include "qa_raybatch.h"
#include "qa_stage.h"

// ---- the ten instances: qa_integrate_points<RES, LIGHTS, TEX, AREA> by the picker, the checks and the launch of qa_raybatch.h
QA_DEFINE_RAYS_PICKER(PickPoints, qa_integrate_points)

// (the checks are the rays' with no differentials or screen positions, no flag known but QA_RADIANCE_PHOTON_MAPS - which picks the
// gathering family, qa_irradiance_pm.hip, and never reaches RayBatch::flags - and no first segment that could miss into a
// background image)
static RaysFn PickFor(const qa_ctx *c, const qa_radiance_params *p) { return WantsPhotonMaps(p) ? PickPointsPm(c) : PickPoints(c); }

extern "C" {

int qa_irradiance_points_device(qa_ctx *c, uint64_t n, const float *d_points, const float *d_normals, const uint32_t *d_stream,
                                const qa_radiance_params *params, float *d_rgb, uint32_t *d_nsamples, void *stream)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = RayBatchChecks(c, n, d_points && d_normals, false, false, false, params, d_rgb != nullptr, QA_RADIANCE_PHOTON_MAPS, false)) return rc;
  if (n == 0) return QA_OK;
  const RayBatch rb = {d_points, d_normals, nullptr, nullptr, nullptr, d_stream, (uint32_t) n, 0u};
  return LaunchRayBatch(c, PickFor(c, params), n, rb, *params, d_rgb, nullptr, d_nsamples, StreamOf(c, stream));
}

int qa_irradiance_points(qa_ctx *c, uint64_t n, const float *points, const float *normals, const uint32_t *stream_ids, const qa_radiance_params *params,
                         float *rgb, uint32_t *nsamples)
{
  if (int rc = Enter(c)) return rc;
  if (int rc = RayBatchChecks(c, n, points && normals, false, false, false, params, rgb != nullptr, QA_RADIANCE_PHOTON_MAPS, false)) return rc;
  if (n == 0) return QA_OK;
  QueryStage st(c);
  const auto dP = st.In(points, 3 * n), dN = st.In(normals, 3 * n);
  const auto dStream = st.In(stream_ids, n);
  const auto dRgb = st.Out(rgb, 3 * n);
  const auto dNs = st.Out(nsamples, n);
  if (int rc = st.Begin()) return rc;
  const RayBatch rb = {st(dP), st(dN), nullptr, nullptr, nullptr, st(dStream), (uint32_t) n, 0u};
  if (int rc = LaunchRayBatch(c, PickFor(c, params), n, rb, *params, st(dRgb), nullptr, st(dNs), c->stream)) return rc;
  if (int rc = st.End()) return rc;
  return DrainEvents(c);   // the batch is complete: fold its event pair into the kernel time
}

}  // extern "C"
