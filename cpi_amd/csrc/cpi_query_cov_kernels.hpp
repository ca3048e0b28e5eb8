// cpi_query_cov_kernels.hpp -- the covariance at arbitrary times inside a window (cpi_query_cov_batch): cpi_query_cov_kernel.
// Part of the translation unit cpi_query_cov.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once
#include "cpi_covq_common.hpp"

namespace {

// Query k asks for the covariance of window w = qwin[k] at time t_q = qtime[k].  The rows of cpi_preintegrate_running hold P
// after every interval, so a query is the covariance recursion of cov_body (cpi_cov_kernels.hpp) run for exactly ONE partial
// interval from a gathered row.  One lane group per query (CovDims<MODEL>::GROUP lanes, cov_col_of_lane: a lane owns a column):
//   search   as cpi_query_kernel: i = the largest knot index in [0, n] with t_i <= t_q, by bisection with clamped probes; every lane
//            of a group runs it (the loads are broadcasts), so no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
//   gather   column jj of S = row w N + i - 1 of rows.P (15 contiguous doubles), or, when only rows.P_sym is given, its entries
//            (min(r, jj), max(r, jj)); i == 0: zeros.  Model 2 carries 18 rows and columns; at a row boundary the reference has just
//            cloned and marginalised (Pbig = Bk Pbig Bk^T, CpiV2.h:436-443; cov_end + the column clone in cov_body), so rows 15..17 of
//            every column are its rows 0..2 and columns 15..17 are columns 0..2: the clone lanes load the theta columns.  The nine
//            Discrete_J_b transition columns never feed P: their lanes idle as zero columns (index NCOL);
//   step     lane 0 of the group builds the interval record of [t_i, t_q] with reading i held (make_sample_rec / finish_interval,
//            the rotation at its start = quat_2_Rot of the row's q as in cpi_query_kernel) into LDS; then the four RK4 stages of
//            cov_body through the same exchange rows.  A query without a step (t_q on a stamp, before t_0, at or past t_n, NaN)
//            runs the stages with dt = 0 and its lanes SELECT the gathered column, so the copy is bit for bit the row;
//   store    columns jj < 15, rows 0..14, as cov_body stores them (cov_end and the column clone after the interval would only refresh
//            rows / columns 15..17, which no output reads: they are left out).
// LDS per wavefront: one record per group + the exchange rows = 8.0 KB (model 1), 4.8 KB (model 2).
// OPEN (cpi_query_cov_open_kernel, cpi_query_open_batch): as in cpi_query_kernel -- the i == 0 gather reads row w base_N + base_N - 1
// of QueryBase::rows (its P or, without one, its P_sym) instead of zeros, and a gathered q[0] that is NaN gives NaN.
template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_COV_WPS) void cpi_query_cov_kernel(QueryArgs A, QueryCovNoise NZ) {
    constexpr bool OPEN = false;
    const QueryBase B = QueryBase();
#include "cpi_covq_body.inc"
}

}  // namespace
