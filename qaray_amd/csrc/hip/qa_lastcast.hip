// qa_lastcast.hip — the per-lane integrator of resident scenes without lights whose bounce rays need only know which emitter they
// meet (ScenePlan::lastCastQuery; qa_kernel.h lastCastQuery), and its picker.  A unit of its own: the kernel is compiled side by
// side with qa_mega.hip's, and theirs keep their names and resources.
#include "qa_kernel.h"
#include "qa_ctx.h"

KernelFn PickLastCastKernel() { return (KernelFn) qa::qa_integrate_lastcast<true>; }

namespace qa {
// The kernel's decision of section A, observable without timing (qa_empty_tiles_device): one thread per tile of the launch, numbered
// as the kernel's work items are before tile_order (strip-major), asks tileIsEmpty with the arguments section A gives it
__global__ __launch_bounds__(64) void qa_empty_tile_mask(const DScene sc, const RenderParams rp, unsigned tiles, uint8_t *mask)
{
  const unsigned tile = blockIdx.x * 64u + threadIdx.x;
  if (tile >= tiles) return;
  const unsigned tilesX = (unsigned) (rp.x1 - rp.x0 + 7) / 8;
  const unsigned otr = tile / tilesX;
  TileCone cone;
  mask[tile] = tileIsEmpty(EmptyTileScene<true>{sc}, sc.cam, sc.background, sc.num_inst, sc.rootIdentity != 0, (float) (rp.x0 + (int) ((tile % tilesX) * 8)),
                           (float) (rp.y0 + (int) (((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8)), &cone) ? 1 : 0;
}
}  // namespace qa

int LaunchEmptyTileMask(const DScene &ds, const RenderParams &rp, unsigned tiles, uint8_t *d_mask, hipStream_t s)
{
  hipLaunchKernelGGL(qa::qa_empty_tile_mask, dim3((tiles + 63) / 64), dim3(64), 0, s, ds, rp, tiles, d_mask);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}
