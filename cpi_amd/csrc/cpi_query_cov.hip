// cpi_query_cov.hip -- translation unit of cpi_query_cov_batch: cpi_query_cov_kernel (cpi_query_cov_kernels.hpp), the covariance at
// arbitrary times inside a window from the P / P_sym rows of cpi_preintegrate_running, with its launcher (cpi_args.hpp:
// cpi::launch).  A unit of its own: no other unit is recompiled for it, and its kernels have a resource report of their own
// (resource_usage_query_cov.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_query_cov_kernels.hpp"

namespace cpi {
namespace launch {

// One lane group per query: 4 queries per wavefront for model 1, 2 for model 2.  Model 1 has no instance for imu_avg: the partial
// interval holds its reading, and (x + x) * 0.5 is x.  Model 2's averaging also takes the gravity term at both ends of the interval.
void query_cov(int model, bool avg, const QueryArgs &a, const double q4[4], hipStream_t st) {
    QueryCovNoise nz;
    for (int i = 0; i < 4; i++) nz.q4[i] = q4[i];
    const long long per = 64 / (model == CPI_MODEL_V2 ? CovDims<2>::GROUP : CovDims<1>::GROUP);
    const dim3 grid((unsigned)((a.Q + per - 1) / per)), block(64);
    if (model != CPI_MODEL_V2) hipLaunchKernelGGL((cpi_query_cov_kernel<1, false>), grid, block, 0, st, a, nz);
    else if (avg)              hipLaunchKernelGGL((cpi_query_cov_kernel<2, true>), grid, block, 0, st, a, nz);
    else                       hipLaunchKernelGGL((cpi_query_cov_kernel<2, false>), grid, block, 0, st, a, nz);
}

}  // namespace launch
}  // namespace cpi
