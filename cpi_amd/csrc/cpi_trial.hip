// cpi_trial.hip -- translation unit of the optimiser's trial step: cpi_retract_kernel / cpi_local_kernel (JPLNavState::retract /
// localCoordinates, JPLNavState.cpp:37-88), cpi_factor_cost_kernel (the whitened cost of the IMU factors at trial states) and the
// two kernels of its deterministic total (cpi_trial_kernels.hpp), with their launchers (cpi_args.hpp: cpi::launch).  A unit of its
// own: no other unit is recompiled for it, and its kernels have a resource report of their own (resource_usage_trial.txt;
// cpi_amd/build.py).  It includes cpi_factor_kernels.hpp for the input fetch and the record layout of the evaluateError sweeps; the
// kernels of that header are templates and none of them is instantiated here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpi_args.hpp"
#include "cpi_math.hpp"

using namespace cpi;

#include "cpi_device_util.hpp"
#include "cpi_factor_kernels.hpp"
#include "cpi_trial_kernels.hpp"

namespace cpi {
namespace launch {

void retract(long long S, const double *states_in, const double *delta, double *states_out, hipStream_t st) {
    hipLaunchKernelGGL(cpi_retract_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, S, states_in, delta, states_out);
}

void local_coordinates(long long S, const double *x, const double *other, double *xi, hipStream_t st) {
    hipLaunchKernelGGL(cpi_local_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, S, x, other, xi);
}

// lpf: 16 | 8 | 4 lanes per factor (cpi_abi.hip: cost_lanes says which and why)
void factor_cost(int model, int lpf, const FactorArgs &a, double *chi2, double *werr, hipStream_t st) {
    const long long F = a.F;
    CostOut o;
    o.chi2 = chi2; o.werr = werr;
#define CPI_COST(M, TR, L) hipLaunchKernelGGL((cpi_factor_cost_kernel<M, TR, L>), dim3((unsigned)((F + 64 / L - 1) / (64 / L))), dim3(64), 0, st, a, o)
#define CPI_COST_L(M, TR) \
    do { if (lpf == 16) CPI_COST(M, TR, 16); else if (lpf == 8) CPI_COST(M, TR, 8); else CPI_COST(M, TR, 4); } while (0)
    if (a.r_tri) {
        if (model == CPI_MODEL_V1) CPI_COST_L(1, true); else CPI_COST_L(2, true);
    } else {
        if (model == CPI_MODEL_V1) CPI_COST_L(1, false); else CPI_COST_L(2, false);
    }
#undef CPI_COST_L
#undef CPI_COST
}

size_t cost_total_doubles(long long F) {
    return 1 + (F > COST_DIRECT ? (size_t)((F + COST_CHUNK - 1) / COST_CHUNK) : 0);
}

// workspace[0] = 0.5 * sum chi2[0 .. F); workspace[1 ..]: the partial sums of the first level when F > COST_DIRECT
void cost_total(long long F, const double *chi2, double *workspace, hipStream_t st) {
    if (F > COST_DIRECT) {
        const long long nb = (F + COST_CHUNK - 1) / COST_CHUNK;
        hipLaunchKernelGGL(cpi_cost_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, F, chi2, workspace + 1);
        hipLaunchKernelGGL(cpi_cost_final_kernel, dim3(1), dim3(256), 0, st, nb, (const double *)(workspace + 1), 0.5, workspace);
    } else {
        hipLaunchKernelGGL(cpi_cost_final_kernel, dim3(1), dim3(256), 0, st, F, chi2, 0.5, workspace);
    }
}

}  // namespace launch
}  // namespace cpi
