// cpi_condense.hip -- translation unit of cpi_chain_condense_batch and cpi_chain_expand_batch: cpi_condense_kernel and
// cpi_expand_kernel (cpi_condense_kernels.hpp: chains of IMU factors cut into segments whose interior states are eliminated in
// parallel, and the back-substitution into them) with their launchers (cpi_args.hpp: cpi::launch).  A unit of its own: no other unit is
// recompiled for it, and its kernels have a resource report of their own (resource_usage_condense.txt; cpi_amd/build.py).  It includes
// cpi_factor_kernels.hpp for the DPP multiply-adds and the pivot rule; the kernels of that header are templates and none of them is
// instantiated here.  The solve kernel's header is NOT included: what the kernels share is cpi_chain_util.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_factor_kernels.hpp"
#include "cpi_chain_util.hpp"
#include "cpi_condense_kernels.hpp"

namespace cpi {
namespace launch {

size_t condense_workspace_doubles(long long S) { return S > 0 ? (size_t)S * chn::CS_D : 1; }

// 16 lanes per segment slot, 4 slots per wavefront; a chain has max(Gr - 1, 1) slots
long long condense_groups(long long C, int Gr) { return C * (long long)(Gr > 1 ? Gr - 1 : 1); }
void chain_condense(const CondenseArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_condense_kernel, dim3((unsigned)((condense_groups(a.C, a.Gr) + 3) / 4)), dim3(64), 0, st, a);
}
void chain_expand(const ExpandArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(cpi_expand_kernel, dim3((unsigned)((condense_groups(a.C, a.Gr) + 3) / 4)), dim3(64), 0, st, a);
}

}  // namespace launch
}  // namespace cpi
