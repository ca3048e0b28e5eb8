// cpi_covq_body.hpp -- the covariance at an arbitrary time inside a window: the body of cpi_query_cov_kernel
// (cpi_query_cov_kernels.hpp), cpi_query_cov_open_kernel (cpi_query_open_kernels.hpp) and cpi_squery_cov_kernel
// (cpi_query_stream_kernels.hpp) described, with the noise argument and the occupancy target they share.  The statements themselves
// are cpi_covq_body.inc.
// Part of a kernel translation unit (included after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once
#include "cpi_query_locate.hpp"

namespace {

// sigma^2 of the four diagonal blocks of Q_c (PreArgs::q4).  A kernel argument of its own beside QueryArgs / StreamQueryArgs, which
// the mean and the transition-column kernels take without it.
struct QueryCovNoise { double q4[4]; };

#ifndef CPI_QUERY_COV_WPS
#define CPI_QUERY_COV_WPS 2   // wavefronts per SIMD the register allocation must leave room for (the build report shows what it got)
#endif

// Query k asks for the covariance of window w at time t_q = qtime[k].  The rows of cpi_preintegrate_running hold P
// after every interval, so a query is the covariance recursion of cov_body (cpi_cov_kernels.hpp) run for exactly ONE partial
// interval from a gathered row.  One lane group per query (CovDims<MODEL>::GROUP lanes, cov_col_of_lane: a lane owns a column):
//   search   the locator's (cpi_query_locate.hpp), as in query_mean_body; every lane of a group runs it (the loads are broadcasts),
//            so no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
//   gather   column jj of S = row w N + i - 1 of rows.P (15 contiguous doubles), or, when only rows.P_sym is given, its entries
//            (min(r, jj), max(r, jj)); i == 0: zeros.  Model 2 carries 18 rows and columns; at a row boundary the reference has just
//            cloned and marginalised (Pbig = Bk Pbig Bk^T, CpiV2.h:436-443; cov_end + the column clone in cov_body), so rows 15..17 of
//            every column are its rows 0..2 and columns 15..17 are columns 0..2: the clone lanes load the theta columns.  The nine
//            Discrete_J_b transition columns never feed P: their lanes idle as zero columns (index NCOL);
//   step     lane 0 of the group builds the interval record of [t_i, t_q] with reading i held (make_sample_rec / finish_interval,
//            the rotation at its start = quat_2_Rot of the row's q as in query_mean_body) into LDS; then the four RK4 stages of
//            cov_body through the same exchange rows.  A query without a step (t_q on a stamp, before t_0, at or past t_n, NaN)
//            runs the stages with dt = 0 and its lanes SELECT the gathered column, so the copy is bit for bit the row;
//   store    columns jj < 15, rows 0..14, as cov_body stores them (cov_end and the column clone after the interval would only refresh
//            rows / columns 15..17, which no output reads: they are left out).
// LDS per wavefront: one record per group + the exchange rows = 8.0 KB (model 1), 4.8 KB (model 2).
//
// Unlike the mean and the transition-column bodies this one is a text fragment (cpi_covq_body.inc), not a function template.  As an
// inlined function the optimiser meets the same statements in another phase order and leaves a number of fadd with their operands
// exchanged; under -ffp-contract=fast the instruction selector then fuses another product of a sum of products into the fma, and
// entries of P move by one ulp and more (the largest difference of an array: 7 ulp in the median, 1634 ulp at most;
// profiles/query_family_fold.md).  Pasted into the kernel the statements compile to the sums they always were.

}  // namespace
