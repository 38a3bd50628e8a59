// qa_radiance_pm.hip — qa_radiance_rays* with QA_RADIANCE_PHOTON_MAPS: the eight instances of qa_integrate_rays_pm<RES, TEX, AREA>
// (qa_kernel.h) and their picker.  A unit of its own, as qa_radiance.hip is beside the frames' integrators: the plain batch kernels
// and every shipped integrator keep their names, resources and code.  The entry points, their checks and the launch stay where they
// are (qa_radiance.hip, qa_raybatch.h); the opening comment of qa_radiance.hip specifies everything a ray batch does, and what
// follows says what the flag adds to it.
//
// SEMANTICS (QA_RADIANCE_PHOTON_MAPS, bit 3 of qa_radiance_params::flags)
// The batch runs with Scene::usePhotonMap = true, exactly as a frame does once qa_photon_maps_build has run: the kernel is
// qa_integrate_rays with PHOTON = true (LIGHTS = true: a map needs a point light; STATS = false), and the text of sections C - E of
// qa_kernel_body.h is the frames' PHOTON variants'.  At every hit whose lobe draw selects diffuse, section D adds
// T * photonGather(caustics map) and, when the ray comes from a diffuse bounce (fromDiffuse), T * photonGather(photon map) ahead of
// it - between the emission term and the direct light (or the AREA variants' log record).  The gathers draw no random number: the
// stream of a sample is the same with and without maps, and so are its first hit (t), its sample count and its casts.
//   Opt-in: a frame changes silently when maps are built; a batch says what it wants.  Without the flag everything is as it was,
//     the QA_EUNSUPPORTED refusal while maps are built included.  With the flag and no maps built: QA_ENOSCENE ("no photon maps
//     built", as qa_photon_maps_info), and nothing is written.  All other refusals, their order, the counters, qa_request_stop and
//     void rays are the plain batch's.
//   The anchor is the plain batch's with maps: the renderer's own camera rays of every sample, handed back in with the flag, give
//     the frame that gathers - rgb, t, ns and the counters bit for bit (tests/test_gpu_radiance_photon.py).
//   Launch (qa_raybatch.h LaunchRayBatch): rp.pm[0..1] and rp.heap as a frame's (qa_ctx.h SetPhotonParams); the LDS bytes and the
//     stack depth are the photon variants' (qa_ctx::integ[kPm]: the kd-tree gather may need a deeper stack than the scene); the
//     persistent grid is capped at numCUs * min(8, resident workgroups per CU): the heap slab holds numCUs * 8 * QA_BLOCK lanes and is
//     indexed by blockIdx.x * QA_BLOCK + threadIdx.x.  A batch waits for and records the context's lastFrame, which serialises it
//     against frames and other batches: that is what keeps two users of the one heap slab apart.
//   Instances: all eight of <RES, TEX, AREA>, by PickPmKernel's predicates (plan.resident, plan.textured, plan.area); each is run by
//     a scene of the tests.
#include "qa_kernel.h"
#include "qa_raybatch.h"

QA_DEFINE_PM_PICKER(PickRaysPm, qa_integrate_rays_pm)
