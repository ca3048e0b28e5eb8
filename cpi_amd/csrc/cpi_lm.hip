// cpi_lm.hip -- translation unit of the Levenberg-Marquardt step per chain: cpi_lm_prior_kernel (cpi_prior_relinearize_batch),
// cpi_lm_cost_kernel (cpi_chain_cost_batch) and cpi_lm_accept_kernel (cpi_chain_accept_batch) of cpi_lm_kernels.hpp, with their
// launchers (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is recompiled for it, and its kernels have a resource
// report of their own (resource_usage_lm.txt; cpi_amd/build.py).  It includes cpi_factor_kernels.hpp for ld_state and what
// cpi_chain_util.hpp names, and cpi_chain_util.hpp for the ONE statement of how first / count / ffirst are clamped (chain_range); the
// kernels of the first header are templates and none of them is instantiated here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_factor_kernels.hpp"
#include "cpi_chain_util.hpp"
#include "cpi_lm_kernels.hpp"

namespace cpi {
namespace launch {

// 16 lanes per record, 4 records per wavefront
void lm_prior(const LmPriorArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_lm_prior_kernel, dim3((unsigned)((a.P + 3) / 4)), dim3(64), 0, st, a);
}

// 16 lanes per chain, 4 chains per wavefront
void lm_cost(const LmCostArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_lm_cost_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(64), 0, st, a);
}

void lm_accept(const LmCostArgs &a, const LmAcceptArgs &b, hipStream_t st) {
    hipLaunchKernelGGL(cpi_lm_accept_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(64), 0, st, a, b);
}

}  // namespace launch
}  // namespace cpi
