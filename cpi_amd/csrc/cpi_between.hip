// cpi_between.hip -- translation unit of cpi_state_between_batch: cpi_between_kernel<kind> of cpi_between_kernels.hpp, one instance per
// kind (position, orientation, pose), with its launcher (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is recompiled
// for it, and its kernels have a resource report of their own (resource_usage_between.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_between_kernels.hpp"

namespace cpi {
namespace launch {

// 16 lanes per factor, 4 factors per wavefront; the kind is a template parameter, so d and the touched columns are compile-time
void state_between(int kind, const BetweenArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.F + 3) / 4)), block(64);
    switch (kind) {
        case chn::BETWEEN_POSITION: hipLaunchKernelGGL(cpi_between_kernel<chn::BETWEEN_POSITION>, grid, block, 0, st, a); break;
        case chn::BETWEEN_ORIENTATION: hipLaunchKernelGGL(cpi_between_kernel<chn::BETWEEN_ORIENTATION>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(cpi_between_kernel<chn::BETWEEN_POSE>, grid, block, 0, st, a); break;
    }
}

}  // namespace launch
}  // namespace cpi
