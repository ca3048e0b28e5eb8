// cpi_running.hip -- translation unit of cpi_mean_running_kernel: the mean (+ model-1 analytic Jacobian) recursion that writes
// the measurement after EVERY interval (cpi_preintegrate_running), and of cpi_mean_stream_running_kernel, the same recursion on
// windows cut out of IMU stream(s) in place (cpi_preintegrate_stream[s]_running), with their launchers (cpi_args.hpp:
// cpi::launch).  A unit of its own: the batch kernels of cpi_mean.hip are not recompiled for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_running_kernels.hpp"

namespace cpi {
namespace launch {

template <int MODEL, bool JAC, bool AVG>
static void launch_running(int L, const PreArgs &a, hipStream_t st) {
    const long long nb = (a.W + (64 / L) - 1) / (64 / L);
    if (L > 1) hipLaunchKernelGGL((cpi_mean_running_kernel<MODEL, JAC, AVG, true>), dim3((unsigned)nb), dim3(64), 0, st, a, L);
    else       hipLaunchKernelGGL((cpi_mean_running_kernel<MODEL, JAC, AVG, false>), dim3((unsigned)nb), dim3(64), 0, st, a, 1);
}
// jac: model 1 only (the caller refuses the Jacobian fields of model 2)
void mean_running(int model, bool jac, bool avg, int L, const PreArgs &a, hipStream_t st) {
    if (model == CPI_MODEL_V2) { if (avg) launch_running<2, false, true>(L, a, st); else launch_running<2, false, false>(L, a, st); }
    else if (jac)              { if (avg) launch_running<1, true, true>(L, a, st); else launch_running<1, true, false>(L, a, st); }
    else                       { if (avg) launch_running<1, false, true>(L, a, st); else launch_running<1, false, false>(L, a, st); }
}

template <int MODEL, bool JAC, bool AVG>
static void launch_stream_running(int L, const PreArgs &a, hipStream_t st) {
    const long long nb = (a.W + (64 / L) - 1) / (64 / L);
    if (L > 1) hipLaunchKernelGGL((cpi_mean_stream_running_kernel<MODEL, JAC, AVG, true>), dim3((unsigned)nb), dim3(64), 0, st, a, L);
    else       hipLaunchKernelGGL((cpi_mean_stream_running_kernel<MODEL, JAC, AVG, false>), dim3((unsigned)nb), dim3(64), 0, st, a, 1);
}
// a.first / count / tstart / tend: the cut in the workspace; a.K: the readings of the stream (every read stays below it)
void mean_stream_running(int model, bool jac, bool avg, int L, const PreArgs &a, hipStream_t st) {
    if (model == CPI_MODEL_V2) { if (avg) launch_stream_running<2, false, true>(L, a, st); else launch_stream_running<2, false, false>(L, a, st); }
    else if (jac)              { if (avg) launch_stream_running<1, true, true>(L, a, st); else launch_stream_running<1, true, false>(L, a, st); }
    else                       { if (avg) launch_stream_running<1, false, true>(L, a, st); else launch_stream_running<1, false, false>(L, a, st); }
}

}  // namespace launch
}  // namespace cpi
