// cpi_query_open_kernels.hpp -- the query family for windows that continue from a carried state (cpi_query_open_batch):
// cpi_query_open_kernel, cpi_query_cov_open_kernel, cpi_query_stj_open_kernel.
// Part of the translation unit cpi_query_open.hip (included there after cpi_query_kernels.hpp and cpi_stj_kernels.hpp, whose helpers
// and occupancy targets the bodies use; not a stand-alone header).  Each kernel is the body of its closed twin with OPEN set.
#pragma once
#include "cpi_covq_common.hpp"

namespace {

// cpi_query_open_batch: cpi_query_kernel for windows that continue from a base row.  A kernel of its own name
// over the shared body, so that cpi_query_kernel compiles to the code it had before.
template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_query_open_kernel(QueryArgs A, QueryBase B) {
    constexpr bool OPEN = true;
#include "cpi_query_body.inc"
}

// cpi_query_open_batch: cpi_query_cov_kernel for windows that continue from a base row.  A kernel of its own
// name over the shared body, so that cpi_query_cov_kernel compiles to the code it had before.
template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_COV_WPS) void cpi_query_cov_open_kernel(QueryArgs A, QueryCovNoise NZ, QueryBase B) {
    constexpr bool OPEN = true;
#include "cpi_covq_body.inc"
}

// cpi_query_open_batch: cpi_query_stj_kernel for windows that continue from a base row.  A kernel of its own
// name over the shared body, so that cpi_query_stj_kernel compiles to the code it had before.
template <bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_STJ_WPS) void cpi_query_stj_open_kernel(QueryArgs A, QueryBase B) {
    constexpr bool OPEN = true;
#include "cpi_query_stj_body.inc"
}

}  // namespace
