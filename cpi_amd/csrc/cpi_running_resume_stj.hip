// cpi_running_resume_stj.hip -- translation unit of cpi_running_resume_stj_batch: cpi_cov_running_stj_carry_kernel (cov_body of
// cpi_cov_kernels.hpp with CARRY, RUNNING and STJ together: the rows of P / P_sym and of model 2's seven Jacobian fields for windows
// that continue from carry records), with its launcher (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is recompiled
// for it, and its kernels have a resource report of their own (resource_usage_running_resume_stj.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#define CPI_COV_TEMPLATES_ONLY   // cov_body and the kernels over it; the Forster comparator belongs to cpi_cov.hip alone
#include "cpi_cov_kernels.hpp"

namespace cpi {
namespace launch {

// model 2 only: what cov_running_carry writes + the fields J_q ... O_b of a.out that are set, W * N rows each
void cov_running_carry_stj(bool avg, const PreArgs &a, const CarryArgs &c, hipStream_t st) {
    constexpr int G = 64 / CovDims<2>::GROUP;
    const dim3 grid((unsigned)((a.W + G - 1) / G)), block(64);
    if (avg) hipLaunchKernelGGL((cpi_cov_running_stj_carry_kernel<true>), grid, block, 0, st, a, c);
    else     hipLaunchKernelGGL((cpi_cov_running_stj_carry_kernel<false>), grid, block, 0, st, a, c);
}

}  // namespace launch
}  // namespace cpi
