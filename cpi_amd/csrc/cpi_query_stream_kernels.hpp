// cpi_query_stream_kernels.hpp -- the query family by ABSOLUTE time over IMU stream(s) read in place (cpi_query_stream_batch):
// cpi_squery_mean_kernel, cpi_squery_cov_kernel, cpi_squery_jac2_kernel.
// Part of the translation unit cpi_query_stream.hip (included there after cpi_math.hpp / cpi_device_util.hpp and after
// cpi_query_kernels.hpp, cpi_covq_body.hpp and cpi_stj_kernels.hpp, which hold the three bodies the kernels call).  The lookup
// helpers at the top are plain inline functions: the CPU emulation (tests/hostsim/hostsim_query_stream.cpp) includes this header after
// cpi_math.hpp and runs the code the kernels run.
#pragma once

namespace cpi {

// ---- window lookup: the window of run r_raw that holds t_q
// r = r_raw clamped into [0, R); [u0, u1) = the run's windows from the CLAMPED offsets (uoff == NULL: one run, [0, U)).  u1 <= u0:
// -1 (a run without update times).  Otherwise u0 + #{v in [u0, u1) : update[v] < t_q}, clamped to u1 - 1: window u covers
// (update[u - 1], update[u]], of equal update times the first wins, a time past the last update gets the last window, and a NaN
// compares false everywhere (u0).  The count is found by bisection: sum of the steps = 2^trips - 1 >= U >= u1 - u0, every probe is
// clamped into [1, u1 - u0], and a probe past the end never moves the count -- no read leaves update[0, U) whatever the offsets hold
// (the update times of a run are assumed non-decreasing).  trips = ceil(log2(U + 1)), the same for every lane.
CPI_HD long long squery_window(const double *update, long long U, const long long *uoff, int R, int r_raw, double tq, int trips) {
    long long u0 = 0, u1 = U;
    if (uoff) {
        const int r = r_raw < 0 ? 0 : (r_raw > R - 1 ? R - 1 : r_raw);
        const long long a = uoff[r], b = uoff[r + 1];
        u0 = a < 0 ? 0 : (a > U ? U : a);
        u1 = b < u0 ? u0 : (b > U ? U : b);
    }
    const long long len = u1 - u0;
    if (len <= 0) return -1;
    long long c = 0;
    for (int s = trips - 1; s >= 0; --s) {
        const long long probe = c + (1ll << s);
        const double t = update[u0 + (probe < len ? probe : len) - 1];
        c = (probe <= len && t < tq) ? probe : c;
    }
    return u0 + (c < len - 1 ? c : len - 1);
}

// ---- the window as the kernels see it: the record cpi_cut_windows_kernel / cpi_cut_runs_kernel left for window u
struct SWindow {
    long long k0;     // the front reading (index into the stream)
    int n;            // the cut count clamped into [0, N]
    bool tail;        // knot n is the end of a tail interval: it carries tend and does not exist in the stream
    double tstart;    // the patched stamp of knot 0
    double tend;
};
CPI_HD SWindow squery_cut(const long long *first, const int *count, const double *tstart, const double *tend, long long u, int N) {
    SWindow w;
    const int c = count[u];
    w.k0 = first[u];
    w.n = c < 0 ? 0 : (c > N ? N : c);
    w.tstart = tstart[u];
    w.tend = tend[u];
    w.tail = (w.tend == w.tend) && c <= N;   // cov_body: a window truncated to N has lost its tail
    return w;
}
// The reading of knot s in [0, n]: the stream's own, except that the tail knot holds the reading before it.  Clamped into the
// stream, so that a workspace that does not belong to this stream still gives no read outside it.
CPI_HD long long squery_reading(const SWindow &w, long long K, int s) {
    const long long k = w.k0 + ((w.tail && s == w.n) ? s - 1 : s);
    return k < 0 ? 0 : (k > K - 1 ? K - 1 : k);
}
// The stamp of knot s in [0, n]: tstart, the stream's own stamps, and tend at the end of a tail interval.
CPI_HD double squery_stamp(const double *stream, long long K, const SWindow &w, int s) {
    const double t = stream[squery_reading(w, K, s) * 7];
    return s == 0 ? w.tstart : ((w.tail && s == w.n) ? w.tend : t);
}
// The interval: i = the largest knot index in [0, n] with stamp(i) <= t_q (0 when t_q lies before the window), the bisection of
// cpi_query_kernel over the patched stamps.  trips = ceil(log2(N + 1)).
CPI_HD int squery_interval(const double *stream, long long K, const SWindow &w, double tq, int trips) {
    int i = 0;
    for (int s = trips - 1; s >= 0; --s) {
        const int probe = i + (1 << s);
        const double t = squery_stamp(stream, K, w, probe < w.n ? probe : w.n);
        i = (probe <= w.n && t <= tq) ? probe : i;
    }
    return i;
}

}  // namespace cpi

#if defined(__HIPCC__)
namespace {

#ifndef CPI_SQUERY_WPS
#define CPI_SQUERY_WPS 2   // wavefronts per SIMD the lane-group kernels must leave room for (the build report shows what they got)
#endif

// The locator of the stream form (cpi_query_locate.hpp): query k names a run and an ABSOLUTE time.  The window is looked up among the
// run's update times, the interval among the patched stamps of its cut, and knot i is handed on as a plain window would hold it, so
// everything behind find is the window forms' code.  A run without update times has no window: the lanes read window 0 and store NaN.
// In the lane-group kernels every lane of a group runs the lookup (its loads are broadcasts).
struct StreamLocator {
    static __device__ __forceinline__ QueryAt find(const StreamQueryArgs &A, long long k, double tq) {
        QueryAt q;
        const long long u = squery_window(A.update, A.U, A.uoff, A.R, A.qrun ? A.qrun[k] : 0, tq, A.wtrips);
        q.none = u < 0;
        q.w = q.none ? 0 : u;
        const SWindow win = squery_cut(A.first, A.count, A.tstart, A.tend, q.w, A.N);
        q.n = win.n;
        q.i = squery_interval(A.stream, A.K, win, tq, A.trips);
        const double *kn = A.stream + squery_reading(win, A.K, q.i) * 7;
#pragma unroll
        for (int e = 0; e < 7; e++) q.kt[e] = kn[e];
        q.kt[0] = squery_stamp(A.stream, A.K, win, q.i);
        return q;
    }
    // A launch whose rows hold no means (rows.DT == NULL: the call asked for qwin_out alone) looks the windows up and stores nothing else.
    static __device__ __forceinline__ bool reads_rows(const StreamQueryArgs &A) { return A.N > 0 && A.rows.DT; }
    // the GLOBAL window found, -1 for a run without update times
    static __device__ __forceinline__ void note_window(const StreamQueryArgs &A, long long k, const QueryAt &at, bool on) {
        if (A.qwin_out && on) A.qwin_out[k] = at.none ? -1 : (int)at.w;
    }
};

template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_squery_mean_kernel(StreamQueryArgs A) {
    query_mean_body<MODEL, JAC, AVG, false, StreamLocator>(A, QueryBase());
}

template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_SQUERY_WPS) void cpi_squery_cov_kernel(StreamQueryArgs A, QueryCovNoise NZ) {
    constexpr bool OPEN = false;
    typedef StreamLocator Loc;
    const QueryBase B = QueryBase();
#include "cpi_covq_body.inc"
}

template <bool AVG>
__global__ __launch_bounds__(64, CPI_SQUERY_WPS) void cpi_squery_jac2_kernel(StreamQueryArgs A) {
    query_stj_body<AVG, false, StreamLocator>(A, QueryBase());
}

}  // namespace
#endif   // __HIPCC__
