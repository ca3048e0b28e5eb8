// cpi_stj.hip -- translation unit of model 2's bias Jacobians at IMU rate and at query times: cpi_cov_running_stj_kernel (cov_body of
// cpi_cov_kernels.hpp with the read-out of the Discrete_J_b columns after every interval; cpi_running_stj_batch) and
// cpi_query_stj_kernel (cpi_stj_kernels.hpp: those columns rebuilt from a row and advanced by one partial interval;
// cpi_query_stj_batch), with their launchers (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is recompiled for it, and
// its kernels have a resource report of their own (resource_usage_stj.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#define CPI_COV_TEMPLATES_ONLY   // cov_body and the kernels over it; the Forster comparator belongs to cpi_cov.hip alone
#include "cpi_cov_kernels.hpp"
#include "cpi_stj_kernels.hpp"

namespace cpi {
namespace launch {

// model 2 only: the P / P_sym rows of cov_running and the fields J_q ... O_b of a.out that are set, W * N rows each
void cov_running_stj(bool avg, const PreArgs &a, hipStream_t st) {
    constexpr int G = 64 / CovDims<2>::GROUP;
    const dim3 grid((unsigned)((a.W + G - 1) / G)), block(64);
    if (avg) hipLaunchKernelGGL((cpi_cov_running_stj_kernel<true>), grid, block, 0, st, a);
    else     hipLaunchKernelGGL((cpi_cov_running_stj_kernel<false>), grid, block, 0, st, a);
}

// model 2 only: 16 lanes per query, 4 queries per wavefront
void query_stj(bool avg, const QueryArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.Q + 3) / 4)), block(64);
    if (avg) hipLaunchKernelGGL((cpi_query_stj_kernel<true>), grid, block, 0, st, a);
    else     hipLaunchKernelGGL((cpi_query_stj_kernel<false>), grid, block, 0, st, a);
}

}  // namespace launch
}  // namespace cpi
