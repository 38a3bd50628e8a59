// qa_lastcast.hip — the per-lane integrator of resident scenes without lights whose bounce rays need only know which emitter they
// meet (ScenePlan::lastCastQuery; qa_kernel.h lastCastQuery), and its picker.  A unit of its own: the kernel is compiled side by
// side with qa_mega.hip's, and theirs keep their names and resources.
#include "qa_kernel.h"
#include "qa_ctx.h"

KernelFn PickLastCastKernel() { return (KernelFn) qa::qa_integrate_lastcast<true>; }
