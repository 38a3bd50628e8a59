// qa_irradiance_pm.hip — qa_irradiance_points* with QA_RADIANCE_PHOTON_MAPS: the eight instances of
// qa_integrate_points_pm<RES, TEX, AREA> (qa_kernel.h) and their picker.  A unit of its own, as qa_radiance_pm.hip: the plain point
// kernels and every shipped integrator keep their names, resources and code.  The entry points, their checks and the launch stay
// where they are (qa_irradiance.hip, qa_raybatch.h); the opening comment of qa_irradiance.hip specifies everything a point batch
// does, and what follows says what the flag adds to it.
//
// SEMANTICS (QA_RADIANCE_PHOTON_MAPS; the point call's flags are 0 or this bit)
// The batch runs with Scene::usePhotonMap = true, as a frame does once qa_photon_maps_build has run (qa_radiance_pm.hip: the flag,
// its refusals and the launch are the ray batch's).
//   The point's gather: in a PHOTON instance the POINTS branch of qa_kernel_body.h applies section D's statements between the
//     emission term and the direct light to the point's Surface: if the lobe draw selected diffuse,
//       L += T * photonGather(rp.pm[1], P, N, V = N, sf.kd, sf.ks, sf.gloss, stack, heap)
//     - the caustics map only, because the point's path has fromDiffuse = false (section D gathers from the photon map, rp.pm[0],
//     only behind a diffuse bounce).  The gather goes before the point's direct light, or before its log record in the AREA
//     variants.  On the white record kd = (1, 1, 1), ks = 0, gloss = 0: V enters nowhere, as in the point's direct light.
//   Behind the spawn, sections C - E run unchanged: the bounce is flagged fromDiffuse, and its diffuse hits gather from the photon
//     map and the caustics map, as they do in a frame.
//   The gathers draw no random number, so the stream of a sample is the same with and without maps.
//   The heap is the lane's: QA_PHOTON_GATHER + 1 elements of the slab at (blockIdx.x * QA_BLOCK + threadIdx.x), as in section D;
//     the stack is the lane's LDS traversal stack, which no walk uses while a point is shaded.
//
// The anchor is qa_irradiance.hip's with maps: on a scene whose material m is the white record, a ray that hits m on a front face at
// (P, N) gives, through qa_radiance_rays with QA_RADIANCE_MISS_ENVIRONMENT | QA_RADIANCE_PHOTON_MAPS, the bits
// qa_irradiance_points gives at (P, N) with QA_RADIANCE_PHOTON_MAPS and the same stream id, seed, spp and max_bounce
// (tests/test_gpu_irradiance_photon.py): the hit of a first segment has fromDiffuse = false too, and gathers from the caustics map
// alone.
//   Instances: all eight of <RES, TEX, AREA>, by PickPmKernel's predicates; each is run by a scene of the tests.
#include "qa_kernel.h"
#include "qa_raybatch.h"

QA_DEFINE_PM_PICKER(PickPointsPm, qa_integrate_points_pm)
