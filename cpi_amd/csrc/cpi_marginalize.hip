// cpi_marginalize.hip -- translation unit of cpi_chain_marginalize_batch: cpi_marginalize_kernel (cpi_marginalize_kernels.hpp:
// the leading states of every chain of IMU factors eliminated into a prior on the first state that stays, the forward half of the
// chain solve without damping and without the workspace) with its launcher (cpi_args.hpp: cpi::launch).  A unit of its own: no other
// unit is recompiled for it, and its kernel has a resource report of its own (resource_usage_marginalize.txt; cpi_amd/build.py).  It
// includes cpi_factor_kernels.hpp for the DPP multiply-adds and the pivot rule; the kernels of that header are templates and none of
// them is instantiated here.  The solve kernel's header is NOT included: what the kernels share is cpi_chain_util.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_factor_kernels.hpp"
#include "cpi_chain_util.hpp"
#include "cpi_marginalize_kernels.hpp"

namespace cpi {
namespace launch {

// 16 lanes per chain, 4 chains per wavefront
void chain_marginalize(const MarginalizeArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_marginalize_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(64), 0, st, a);
}

}  // namespace launch
}  // namespace cpi
