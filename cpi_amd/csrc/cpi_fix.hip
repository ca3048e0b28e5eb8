// cpi_fix.hip -- translation unit of cpi_state_fix_batch: cpi_fix_kernel<kind> of cpi_fix_kernels.hpp, one instance per kind
// (position, velocity, orientation, pose), with its launcher (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is
// recompiled for it, and its kernels have a resource report of their own (resource_usage_fix.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_fix_kernels.hpp"

namespace cpi {
namespace launch {

// 16 lanes per state, 4 states per wavefront; the kind is a template parameter, so d and sel are compile-time
void state_fix(int kind, const FixArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.S + 3) / 4)), block(64);
    switch (kind) {
        case chn::FIX_POSITION: hipLaunchKernelGGL(cpi_fix_kernel<chn::FIX_POSITION>, grid, block, 0, st, a); break;
        case chn::FIX_VELOCITY: hipLaunchKernelGGL(cpi_fix_kernel<chn::FIX_VELOCITY>, grid, block, 0, st, a); break;
        case chn::FIX_ORIENTATION: hipLaunchKernelGGL(cpi_fix_kernel<chn::FIX_ORIENTATION>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(cpi_fix_kernel<chn::FIX_POSE>, grid, block, 0, st, a); break;
    }
}

}  // namespace launch
}  // namespace cpi
