// qa_mega.hip — the per-lane integrators: every qa_integrate instance without photon-map gathers (those: qa_photon.hip), and their picker
#include "qa_kernel.h"
#include "qa_ctx.h"

const int kMaxPath = QA_MAX_PATH;
const size_t kAreaLogFloats = (size_t) QA_MAX_PATH * QA_REC_FLOATS;

// variants: scene memory (LDS-resident | global) x shading (no lights | lights | + textures | + area
// lights | + both) x stats
template <bool RES, bool STATS>
static KernelFn PickShading(bool lights, bool tex, bool area)
{
  if (area) return tex ? (KernelFn) qa_integrate<RES, true, true, true, STATS> : (KernelFn) qa_integrate<RES, true, false, true, STATS>;
  if (tex) return (KernelFn) qa_integrate<RES, true, true, false, STATS>;
  if (lights) return (KernelFn) qa_integrate<RES, true, false, false, STATS>;
  return (KernelFn) qa_integrate<RES, false, false, false, STATS>;
}
KernelFn PickKernel(bool resident, bool lights, bool tex, bool area, bool stats)
{
  if (resident) return stats ? PickShading<true, true>(lights, tex, area) : PickShading<true, false>(lights, tex, area);
  return stats ? PickShading<false, true>(lights, tex, area) : PickShading<false, false>(lights, tex, area);
}
