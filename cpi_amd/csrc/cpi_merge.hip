// cpi_merge.hip -- translation unit of cpi_merge_batch: cpi_merge_kernel (cpi_merge_kernels.hpp: consecutive preintegrated windows
// joined into one measurement, a segmented left fold over measurement rows) with its launcher (cpi_args.hpp: cpi::launch).  A unit of
// its own: no other unit is recompiled for it, and its kernels have a resource report of their own (resource_usage_merge.txt;
// cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_merge_kernels.hpp"

namespace cpi {
namespace launch {

// 16 lanes per output row, 4 rows per wavefront.  jac / cov: what a.out asks for; a request without cov never reads a.in.P / P_sym,
// a request with neither reads the four mean fields alone.
void merge(bool jac, bool cov, const MergeArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.M + 3) / 4)), block(64);
    if (cov) {
        if (jac) hipLaunchKernelGGL((cpi_merge_kernel<true, true>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((cpi_merge_kernel<false, true>), grid, block, 0, st, a);
    } else {
        if (jac) hipLaunchKernelGGL((cpi_merge_kernel<true, false>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((cpi_merge_kernel<false, false>), grid, block, 0, st, a);
    }
}

}  // namespace launch
}  // namespace cpi
