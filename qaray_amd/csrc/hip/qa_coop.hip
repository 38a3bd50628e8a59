// qa_coop.hip — the integrators with cooperative mesh walks (qa_kernel_cs.h): qa_integrate_cs, qa_integrate_cs_resume and their pickers
#include "qa_kernel_cs.h"
#include "qa_ctx.h"

// per wave [ray slots | results | flags | pool items | accumulators]; four workgroups per CU (160 KB LDS)
size_t CsLdsBytes(uint32_t items, uint32_t slots) { return (size_t) CsLdsWords(items, slots) * (QA_BLOCK / 64) * sizeof(uint32_t); }

// qa_integrate_cs variants; rows: no lights, lights, instance culling without / with lights, MANY, AREA; columns: textures
KernelFn PickCs(bool lights, bool tex, bool cull, bool many, bool area)
{
  static const KernelFn k[6][2] = {
      {(KernelFn) qa_integrate_cs<false, false, false, false>, (KernelFn) qa_integrate_cs<false, true, false, false>},
      {(KernelFn) qa_integrate_cs<true, false, false, false>, (KernelFn) qa_integrate_cs<true, true, false, false>},
      {(KernelFn) qa_integrate_cs<false, false, true, false>, (KernelFn) qa_integrate_cs<false, true, true, false>},
      {(KernelFn) qa_integrate_cs<true, false, true, false>, (KernelFn) qa_integrate_cs<true, true, true, false>},
      {(KernelFn) qa_integrate_cs<true, false, true, true>, (KernelFn) qa_integrate_cs<true, true, true, true>},
      {(KernelFn) qa_integrate_cs<true, false, true, false, true>, (KernelFn) qa_integrate_cs<true, true, true, false, true>}};
  return k[area ? 5 : many ? 4 : 2 * cull + lights][tex];
}
// ... their untextured rows as chunk-capable instances (qa_integrate_cs_resume): the passes of progressive frames
KernelFn PickCsResume(bool lights, bool cull, bool many, bool area)
{
  static const KernelFn k[6] = {(KernelFn) qa_integrate_cs_resume<false, false, false, false>, (KernelFn) qa_integrate_cs_resume<true, false, false, false>,
                                (KernelFn) qa_integrate_cs_resume<false, false, true, false>, (KernelFn) qa_integrate_cs_resume<true, false, true, false>,
                                (KernelFn) qa_integrate_cs_resume<true, false, true, true>, (KernelFn) qa_integrate_cs_resume<true, false, true, false, true>};
  return k[area ? 5 : many ? 4 : 2 * cull + lights];
}
