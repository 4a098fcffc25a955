// gol_step.hip -- instantiates the step kernels of one pass depth.  Compiled
// twice per depth G = GOL_STEP_GENS: the plain instances (the Makefile's
// build/gol_step_g<G>.o) and, with GOL_STEP_SERIES, the population-series
// instances (build/gol_step_series_g<G>.o), so the depths and the two sets
// compile in parallel and each is a code object of its own -- one the runtime
// loads when a kernel of it is first asked for.
#include "gol_stencil.h"

namespace gol {

#ifdef GOL_STEP_SERIES
template <int G>
StepKernel step_series_kernel_at(const StepInstance& k) {
    return dev::kernel_at_depth<G, true>(k);
}
template StepKernel step_series_kernel_at<GOL_STEP_GENS>(const StepInstance&);
#else
template <int G>
StepKernel step_kernel_at(const StepInstance& k) {
    return dev::kernel_at_depth<G>(k);
}
template StepKernel step_kernel_at<GOL_STEP_GENS>(const StepInstance&);
#endif

}  // namespace gol
