// cpi_query_stream.hip -- translation unit of cpi_query_stream_batch: cpi_squery_mean_kernel / cpi_squery_cov_kernel /
// cpi_squery_jac2_kernel (cpi_query_stream_kernels.hpp), the query family by absolute time over IMU stream(s) read in place -- the
// window lookup and the search over patched stamps in front of the bodies of the three plain query kernels --, with their
// launchers (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is recompiled for it, and its kernels have a resource
// report of their own (resource_usage_query_stream.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_covq_body.hpp"           // the three bodies (the window kernels beside them are not instantiated here)
#include "cpi_stj_kernels.hpp"
#include "cpi_query_kernels.hpp"
#include "cpi_query_stream_kernels.hpp"

namespace cpi {
namespace launch {

// One lane per query; the instances of launch::query.
void squery_mean(int model, bool jac, bool avg, const StreamQueryArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.Q + 63) / 64)), block(64);
    if (model == CPI_MODEL_V2) {
        if (avg) hipLaunchKernelGGL((cpi_squery_mean_kernel<2, false, true>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((cpi_squery_mean_kernel<2, false, false>), grid, block, 0, st, a);
    } else if (jac) hipLaunchKernelGGL((cpi_squery_mean_kernel<1, true, false>), grid, block, 0, st, a);
    else            hipLaunchKernelGGL((cpi_squery_mean_kernel<1, false, false>), grid, block, 0, st, a);
}

// One lane group per query; the instances of launch::query_cov.
void squery_cov(int model, bool avg, const StreamQueryArgs &a, const double q4[4], hipStream_t st) {
    QueryCovNoise nz;
    for (int i = 0; i < 4; i++) nz.q4[i] = q4[i];
    const long long per = 64 / (model == CPI_MODEL_V2 ? CovDims<2>::GROUP : CovDims<1>::GROUP);
    const dim3 grid((unsigned)((a.Q + per - 1) / per)), block(64);
    if (model != CPI_MODEL_V2) hipLaunchKernelGGL((cpi_squery_cov_kernel<1, false>), grid, block, 0, st, a, nz);
    else if (avg)              hipLaunchKernelGGL((cpi_squery_cov_kernel<2, true>), grid, block, 0, st, a, nz);
    else                       hipLaunchKernelGGL((cpi_squery_cov_kernel<2, false>), grid, block, 0, st, a, nz);
}

// model 2 only: 16 lanes per query, 4 queries per wavefront
void squery_jac2(bool avg, const StreamQueryArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.Q + 3) / 4)), block(64);
    if (avg) hipLaunchKernelGGL((cpi_squery_jac2_kernel<true>), grid, block, 0, st, a);
    else     hipLaunchKernelGGL((cpi_squery_jac2_kernel<false>), grid, block, 0, st, a);
}

}  // namespace launch
}  // namespace cpi
