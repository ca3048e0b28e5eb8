// cpi_stj_kernels.hpp -- model 2's bias Jacobians at arbitrary times inside a window (cpi_query_stj_batch): cpi_query_stj_kernel.
// Part of the translation unit cpi_stj.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

#ifndef CPI_QUERY_STJ_WPS
#define CPI_QUERY_STJ_WPS 2   // wavefronts per SIMD the register allocation must leave room for (the build report shows what it got)
#endif

// Query k asks for J_q ... O_b of window w = qwin[k] at time t_q = qtime[k].  The rows of cpi_running_stj_batch hold the
// read-out of the nine Discrete_J_b transition columns (b_w, b_a, theta_klin) after every interval, and at a row boundary that
// read-out determines the columns: cov_end has just set rows 15..17 to rows 0..2, the bias rows are the unit / zero blocks of
// cov_init (F has no bias rows), and the theta rows of the b_a and theta_klin columns are exactly zero ((F x)_theta = -w x x_theta
// - x_bw keeps a zero theta block zero when x_bw is zero).  So a query rebuilds the columns from row w N + i - 1 and advances them by
// the ONE partial interval [t_i, t_q] of cov_body's phase C (cpi_cov_kernels.hpp) with reading i held:
//   b_w column c        [-J_q[:,c] | e_c | J_b[:,c] | 0   | J_a[:,c] | -J_q[:,c]]
//   b_a column c        [ 0        | 0   | H_b[:,c] | e_c | H_a[:,c] |  0       ]
//   theta_klin column c [ 0        | 0   | O_b[:,c] | 0   | O_a[:,c] |  0       ]   (its unit entry enters through h, cov_h_offset)
// i == 0: the cov_init state.  A transition column has no transposed contribution (its Mt is the zero row), so nothing is exchanged
// between lanes: one group of 16 lanes per query, nine of them live, four queries per wavefront, and the only LDS is the interval
// record lane 0 of a group builds for it (make_sample_rec / finish_interval; the rotation at the start = quat_2_Rot of the row's q
// as in cpi_query_kernel).
//   search   as cpi_query_kernel: i = the largest knot index in [0, n] with t_i <= t_q, by bisection with clamped probes; every lane
//            of a group runs it (the loads are broadcasts), so no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
//   step     the four RK4 stages of cov_body with the zero row as Mt.  A query without a step (t_q on a stamp, before t_0, at or
//            past t_n, NaN) stores what it loaded from the base row, bit for bit (zeros when i == 0);
//   store    the read-out of cov_body (J_q = -theta of the b_w columns, ...), 24 bytes per lane and field, for the fields of out
//            that are set.
// LDS per wavefront: 4 records of 42 doubles + 4 rotations = 1.6 KB.
// OPEN (cpi_query_stj_open_kernel, cpi_query_open_batch): as in cpi_query_kernel -- i == 0 rebuilds the columns from row
// w base_N + base_N - 1 of QueryBase::rows (the carried columns read out) instead of taking the cov_init state, and a gathered q[0]
// that is NaN gives NaN.
template <bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_STJ_WPS) void cpi_query_stj_kernel(QueryArgs A) {
    constexpr bool OPEN = false;
    const QueryBase B = QueryBase();
#include "cpi_query_stj_body.inc"
}

}  // namespace
