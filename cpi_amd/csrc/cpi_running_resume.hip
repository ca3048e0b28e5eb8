// cpi_running_resume.hip -- translation unit of cpi_preintegrate_running_resume: cpi_mean_running_carry_kernel (the running mean
// recursion of cpi_running_kernels.hpp / cpi_running_body.inc from and to carry records) and cpi_cov_running_carry_kernel (cov_body
// of cpi_cov_kernels.hpp with CARRY and RUNNING together), with their launchers (cpi_args.hpp: cpi::launch).  A unit of its own:
// cpi_running.hip and cpi_cov.hip are not recompiled for it, and its kernels have a resource report of their own
// (resource_usage_running_resume.txt; cpi_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_running_kernels.hpp"
#define CPI_COV_TEMPLATES_ONLY   // cov_body and the kernels over it; the Forster comparator belongs to cpi_cov.hip alone
#include "cpi_cov_kernels.hpp"

namespace cpi {
namespace launch {

template <int MODEL, bool JAC, bool AVG>
static void launch_running_carry(int L, const PreArgs &a, const CarryArgs &c, hipStream_t st) {
    const long long nb = (a.W + (64 / L) - 1) / (64 / L);
    if (L > 1) hipLaunchKernelGGL((cpi_mean_running_carry_kernel<MODEL, JAC, AVG, true>), dim3((unsigned)nb), dim3(64), 0, st, a, c, L);
    else       hipLaunchKernelGGL((cpi_mean_running_carry_kernel<MODEL, JAC, AVG, false>), dim3((unsigned)nb), dim3(64), 0, st, a, c, 1);
}
// the rows of windows that continue from c.in and are left in c.out (always the owner of the means); jac: model 1 only
void mean_running_carry(int model, bool jac, bool avg, int L, const PreArgs &a, const CarryArgs &c, hipStream_t st) {
    if (model == CPI_MODEL_V2) { if (avg) launch_running_carry<2, false, true>(L, a, c, st); else launch_running_carry<2, false, false>(L, a, c, st); }
    else if (jac)              { if (avg) launch_running_carry<1, true, true>(L, a, c, st); else launch_running_carry<1, true, false>(L, a, c, st); }
    else                       { if (avg) launch_running_carry<1, false, true>(L, a, c, st); else launch_running_carry<1, false, false>(L, a, c, st); }
}

template <int MODEL>
static void launch_cov_running_carry(bool avg, const PreArgs &a, const CarryArgs &c, hipStream_t st) {
    constexpr int G = 64 / CovDims<MODEL>::GROUP;
    const long long nb = (a.W + G - 1) / G;
    if (avg) hipLaunchKernelGGL((cpi_cov_running_carry_kernel<MODEL, true>), dim3((unsigned)nb), dim3(64), 0, st, a, c);
    else     hipLaunchKernelGGL((cpi_cov_running_carry_kernel<MODEL, false>), dim3((unsigned)nb), dim3(64), 0, st, a, c);
}
void cov_running_carry(int model, bool avg, const PreArgs &a, const CarryArgs &c, hipStream_t st) {
    if (model == CPI_MODEL_V2) launch_cov_running_carry<2>(avg, a, c, st); else launch_cov_running_carry<1>(avg, a, c, st);
}

}  // namespace launch
}  // namespace cpi
