// cpi_query_open.hip -- translation unit of cpi_query_open_batch: cpi_query_open_kernel, cpi_query_cov_open_kernel and
// cpi_query_stj_open_kernel (cpi_query_open_kernels.hpp: the bodies of the three closed query kernels with OPEN -- the state before knot
// 0 is a base row instead of the zero state), with their launchers (cpi_args.hpp: cpi::launch).  A unit of its own:
// no other unit is recompiled for it, and its kernels have a resource report of their own (resource_usage_query_open.txt;
// cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_query_kernels.hpp"
#include "cpi_covq_body.hpp"
#include "cpi_stj_kernels.hpp"
#include "cpi_query_open_kernels.hpp"

namespace cpi {
namespace launch {

// the grids and the instances of query / query_cov / query_stj (cpi_query.hip, cpi_query_cov.hip, cpi_stj.hip)
void query_open(int model, bool jac, bool avg, const QueryArgs &a, const QueryBase &b, hipStream_t st) {
    const dim3 grid((unsigned)((a.Q + 63) / 64)), block(64);
    if (model == CPI_MODEL_V2) {
        if (avg) hipLaunchKernelGGL((cpi_query_open_kernel<2, false, true>), grid, block, 0, st, a, b);
        else     hipLaunchKernelGGL((cpi_query_open_kernel<2, false, false>), grid, block, 0, st, a, b);
    } else if (jac) hipLaunchKernelGGL((cpi_query_open_kernel<1, true, false>), grid, block, 0, st, a, b);
    else            hipLaunchKernelGGL((cpi_query_open_kernel<1, false, false>), grid, block, 0, st, a, b);
}

void query_cov_open(int model, bool avg, const QueryArgs &a, const double q4[4], const QueryBase &b, hipStream_t st) {
    QueryCovNoise nz;
    for (int i = 0; i < 4; i++) nz.q4[i] = q4[i];
    const long long per = 64 / (model == CPI_MODEL_V2 ? CovDims<2>::GROUP : CovDims<1>::GROUP);
    const dim3 grid((unsigned)((a.Q + per - 1) / per)), block(64);
    if (model != CPI_MODEL_V2) hipLaunchKernelGGL((cpi_query_cov_open_kernel<1, false>), grid, block, 0, st, a, nz, b);
    else if (avg)              hipLaunchKernelGGL((cpi_query_cov_open_kernel<2, true>), grid, block, 0, st, a, nz, b);
    else                       hipLaunchKernelGGL((cpi_query_cov_open_kernel<2, false>), grid, block, 0, st, a, nz, b);
}

void query_stj_open(bool avg, const QueryArgs &a, const QueryBase &b, hipStream_t st) {
    const dim3 grid((unsigned)((a.Q + 3) / 4)), block(64);
    if (avg) hipLaunchKernelGGL((cpi_query_stj_open_kernel<true>), grid, block, 0, st, a, b);
    else     hipLaunchKernelGGL((cpi_query_stj_open_kernel<false>), grid, block, 0, st, a, b);
}

}  // namespace launch
}  // namespace cpi
