// cpi_chain.hip -- translation unit of cpi_chain_solve_batch: cpi_chain_solve_kernel (cpi_chain_kernels.hpp: the damped
// block-tridiagonal solve of chains of IMU factors, a block Cholesky along each chain on the hess rows as the Hessian sweep wrote
// them) with its launcher (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is recompiled for it, and its kernel has a
// resource report of its own (resource_usage_chain.txt; cpi_amd/build.py).  It includes cpi_factor_kernels.hpp for the DPP
// multiply-adds and the pivot rule of the square-root-information kernel; the kernels of that header are templates and none of them
// is instantiated here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_factor_kernels.hpp"
#include "cpi_chain_util.hpp"
#include "cpi_chain_kernels.hpp"

namespace cpi {
namespace launch {

size_t chain_workspace_doubles(long long S) { return S > 0 ? (size_t)S * chn::WS_D : 1; }

// 16 lanes per chain, 4 chains per wavefront
void chain_solve(const ChainArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_chain_solve_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(64), 0, st, a);
}

}  // namespace launch
}  // namespace cpi
