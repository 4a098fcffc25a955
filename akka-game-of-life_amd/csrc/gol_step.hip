// gol_step.hip -- instantiates the step kernels of one pass depth.  Compiled
// once per depth G = GOL_STEP_GENS (the Makefile's build/gol_step_g<G>.o), so
// the depths compile in parallel and each is a code object of its own.
#include "gol_stencil.h"

namespace gol {

template <int G>
StepKernel step_kernel_at(const StepInstance& k) {
    return dev::kernel_at_depth<G>(k);
}
template StepKernel step_kernel_at<GOL_STEP_GENS>(const StepInstance&);

}  // namespace gol
