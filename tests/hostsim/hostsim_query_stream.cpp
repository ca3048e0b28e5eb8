// hostsim_query_stream.cpp -- HOST build of the lookup helpers of cpi_query_stream_kernels.hpp (squery_window, squery_cut,
// squery_stamp, squery_interval): the very functions the kernels of cpi_query_stream_batch run in their prologue, compiled with the
// host compiler from the same header.  TEST INFRASTRUCTURE ONLY.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include "../../cpi_amd/csrc/cpi_query_stream_kernels.hpp"
using namespace cpi;

// qwin[k] = the window of query k (-1: a run without update times); uoff == NULL: one run
extern "C" int hqs_window(const double *update, long long U, const long long *uoff, int R, long long Q, const int *qrun,
                          const double *qtime, int trips, long long *qwin) {
    for (long long k = 0; k < Q; k++) qwin[k] = squery_window(update, U, uoff, R, qrun ? qrun[k] : 0, qtime[k], trips);
    return 0;
}
// stamps[0 .. N] of window u as the kernels see it (entries past n: NaN), *n = the clamped count, and i = squery_interval for tq
extern "C" int hqs_stamps(const double *stream, long long K, const long long *first, const int *count, const double *tstart,
                          const double *tend, long long u, int N, double tq, int trips, double *stamps, int *n, int *i,
                          long long *reading) {
    const SWindow w = squery_cut(first, count, tstart, tend, u, N);
    *n = w.n;
    for (int s = 0; s <= N; s++) stamps[s] = s <= w.n ? squery_stamp(stream, K, w, s) : __builtin_nan("");
    *i = squery_interval(stream, K, w, tq, trips);
    *reading = squery_reading(w, K, *i);
    return 0;
}
