// cpi_query.hip -- translation unit of cpi_query_batch: cpi_query_kernel (cpi_query_kernels.hpp), the measurement at arbitrary
// times inside a window from the rows of cpi_preintegrate_running, with its launcher (cpi_args.hpp: cpi::launch).  A unit of its
// own: no other unit is recompiled for it, and its kernels have a resource report of their own (resource_usage_query.txt;
// cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_query_kernels.hpp"

namespace cpi {
namespace launch {

// One lane per query.  Model 1 has no instance for imu_avg: the partial interval holds its reading, and (x + x) * 0.5 is x.
// Model 2's averaging also takes the gravity term at both ends of the interval (CpiV2.h:146-149), so it keeps its own.
void query(int model, bool jac, bool avg, const QueryArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.Q + 63) / 64)), block(64);
    if (model == CPI_MODEL_V2) {
        if (avg) hipLaunchKernelGGL((cpi_query_kernel<2, false, true>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((cpi_query_kernel<2, false, false>), grid, block, 0, st, a);
    } else if (jac) hipLaunchKernelGGL((cpi_query_kernel<1, true, false>), grid, block, 0, st, a);
    else            hipLaunchKernelGGL((cpi_query_kernel<1, false, false>), grid, block, 0, st, a);
}

}  // namespace launch
}  // namespace cpi
