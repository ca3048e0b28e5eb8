// cpi_query_cov_kernels.hpp -- the covariance at arbitrary times inside a window (cpi_query_cov_batch): cpi_query_cov_kernel over
// the covariance query body (cpi_covq_body.inc; described in cpi_covq_body.hpp).
// Part of the translation unit cpi_query_cov.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once
#include "cpi_covq_body.hpp"

namespace {

template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_COV_WPS) void cpi_query_cov_kernel(QueryArgs A, QueryCovNoise NZ) {
    constexpr bool OPEN = false;
    typedef WindowLocator Loc;
    const QueryBase B = QueryBase();
#include "cpi_covq_body.inc"
}

}  // namespace
