// cpi_query_kernels.hpp -- the measurement at arbitrary times inside a window (cpi_query_batch): cpi_query_kernel.
// Part of the translation unit cpi_query.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

// Query k asks for the measurement of window w = qwin[k] at time t_q = qtime[k].  The rows of cpi_preintegrate_running already
// hold the state after every interval, so a query is one gather and at most one partial interval:
//   search   i = the largest knot index in [0, n] with t_i <= t_q (0 when t_q lies before the window), by bisection over the
//            window's stamps.  The trip count ceil(log2(N + 1)) is a launch argument -- the same for every lane --, every probe is
//            clamped into [0, n], and a probe past n never moves i: whatever the stamps hold (the search assumes them finite and
//            non-decreasing), no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
//   gather   the base state = row w N + i - 1 (i == 0: the zero state) and knot i, both requested before either is used;
//   step     when t_i < t_q and i < n: feed_IMU(t_i, t_q, w_i, a_i, w_i, a_i) on the base state -- the reading held as the
//            reference holds it over a window's tail (GraphSolver_IMU.cpp:64-69) -- with the rotation rebuilt from the row's
//            quaternion.  Otherwise (t_q on a stamp, before t_0, at or past t_n) the row's own doubles are selected: they never pass
//            through quat_2_Rot / rot_2_quat, so the output is the row bit for bit.  The step runs for every lane (an inactive
//            one with dt = 0) and the selection is per lane: no divergence beyond what mean_step has itself;
//   store    one lane per query for the arithmetic, not for the stores: the 64 results of a wavefront are parked in LDS record-major
//            (pitch 11 doubles: odd, so the lanes' records start in distinct banks) and leave field by field as consecutive 16-byte
//            non-temporal stores -- every field of 64 consecutive queries is one contiguous run of the output array, as in
//            cpi_predict_kernel.  The Jacobians (five 72-byte matrices per query) take turns in the same area.
// A NaN t_q compares false everywhere (i = 0, no step) and is turned into NaN in every requested field at the end.
// OPEN (cpi_query_open_kernel, cpi_query_open_batch): the window continues from a carried state, and the state before knot 0 is
// row w base_N + base_N - 1 of QueryBase::rows instead of the zero state: the i == 0 gather reads it (per lane: the pointers are
// selected, the loads are the same), N == 0 reads nothing else, and a gathered state whose q[0] is NaN (the rows of a refused carry)
// gives NaN in every field.  Everything behind the gather is the same code, so the closed kernels and the open ones agree bit for bit
// wherever they gather the same doubles.
constexpr int QRY_PITCH = 11;   // DT 1 + alpha 3 + beta 3 + q 4; a 3 x 3 matrix (9) fits as well

// Field of F doubles per query at offset `off` of the staged records -> the nq * F consecutive doubles of its output run.
template <int F>
__device__ __forceinline__ void query_flush(const double *stage, int off, double *field, long long q0, int nq, int lane) {
    double *dst = field + q0 * F;
    const int total = nq * F;
    auto at = [&](int e) { const int g = e / F; return stage[g * QRY_PITCH + off + (e - g * F)]; };
    for (int p = lane; 2 * p + 1 < total; p += 64) st16_nt(dst + 2 * p, at(2 * p), at(2 * p + 1));
    if ((total & 1) && lane == 0) dst[total - 1] = at(total - 1);
}

template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_query_kernel(QueryArgs A) {
    constexpr bool OPEN = false;
    const QueryBase B = QueryBase();
#include "cpi_query_body.inc"
}

}  // namespace
