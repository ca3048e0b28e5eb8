// cpi_query_open_kernels.hpp -- the query family for windows that continue from a carried state (cpi_query_open_batch):
// cpi_query_open_kernel, cpi_query_cov_open_kernel, cpi_query_stj_open_kernel.
// Part of the translation unit cpi_query_open.hip (included there after cpi_query_kernels.hpp, cpi_covq_body.hpp and
// cpi_stj_kernels.hpp, which hold the bodies and the occupancy targets; not a stand-alone header).  Each kernel is the body of its
// closed twin with OPEN set (cpi_query_locate.hpp): the state before knot 0 is a base row.
#pragma once

namespace {

template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_query_open_kernel(QueryArgs A, QueryBase B) {
    query_mean_body<MODEL, JAC, AVG, true, WindowLocator>(A, B);
}

template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_COV_WPS) void cpi_query_cov_open_kernel(QueryArgs A, QueryCovNoise NZ, QueryBase B) {
    constexpr bool OPEN = true;
    typedef WindowLocator Loc;
#include "cpi_covq_body.inc"
}

template <bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_STJ_WPS) void cpi_query_stj_open_kernel(QueryArgs A, QueryBase B) {
    query_stj_body<AVG, true, WindowLocator>(A, B);
}

}  // namespace
