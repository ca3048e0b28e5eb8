// cpi_covq_common.hpp -- what cpi_query_cov_kernel (cpi_query_cov_kernels.hpp) and cpi_query_cov_open_kernel
// (cpi_query_open_kernels.hpp) share beside their body (cpi_covq_body.inc): the noise argument and the occupancy target.
#pragma once

namespace {

// sigma^2 of the four diagonal blocks of Q_c (PreArgs::q4).  A kernel argument of its own, so that QueryArgs -- and with it
// cpi_query_kernel -- stays as it was.
struct QueryCovNoise { double q4[4]; };

#ifndef CPI_QUERY_COV_WPS
#define CPI_QUERY_COV_WPS 2   // wavefronts per SIMD the register allocation must leave room for (the build report shows what it got)
#endif

}  // namespace
