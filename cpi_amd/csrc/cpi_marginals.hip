// cpi_marginals.hip -- translation unit of cpi_chain_marginals_batch: cpi_marginals_kernel (cpi_marginals_kernels.hpp: the diagonal and
// first off-diagonal blocks of the inverse of the block-tridiagonal matrix of every chain, one backward recursion over the factor
// that cpi_chain_solve_batch left in the workspace) with its launcher (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is
// recompiled for it, and its kernel has a resource report of its own (resource_usage_marginals.txt; cpi_amd/build.py).  It includes
// cpi_factor_kernels.hpp for the DPP multiply-adds; the kernels of that header are templates and none of them is instantiated here.
// The solve kernel's header is NOT included: what the two kernels share is cpi_chain_util.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_factor_kernels.hpp"
#include "cpi_chain_util.hpp"
#include "cpi_marginals_kernels.hpp"

namespace cpi {
namespace launch {

// 16 lanes per chain, 4 chains per wavefront
void chain_marginals(const MarginalsArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_marginals_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(64), 0, st, a);
}

}  // namespace launch
}  // namespace cpi
