// cpi_query_locate.hpp -- where a query lands: the record the three query bodies (query_mean_body of cpi_query_kernels.hpp,
// the covariance body of cpi_covq_body.hpp / .inc, query_stj_body of cpi_stj_kernels.hpp) start from, and the locator of the window forms.
// Included after cpi_args.hpp inside a kernel translation unit; no kernel is defined here.
//
// A body is stated once and serves three forms of call.  What a form changes is all on this page:
//   locator  a struct of static functions, a template parameter of the body (a type, so that the body does not depend on which
//            overloads happen to be declared before it):
//              find(A, k, tq)             query k -> QueryAt: its window, the interval that holds t_q and knot i;
//              reads_rows(A)              whether the launch has rows to gather from (the mean body asks; wave-uniform);
//              note_window(A, k, at, on)  tells the caller which window was found, from the lanes where `on` holds.
//            WindowLocator (below) serves cpi_query*_batch and cpi_query_open_batch, StreamLocator (cpi_query_stream_kernels.hpp)
//            cpi_query_stream_batch: there the window itself is looked up by absolute time and the stamps are patched at a cut.
//   OPEN     a flag of the body (cpi_query_open_batch): the window continues from a carried state, and the state before knot 0 is
//            row w base_N + base_N - 1 of QueryBase::rows instead of the zero state.  The i == 0 gather reads it (per lane: the
//            pointers are selected, the loads are the same) -- the mean body its state and Jacobians, the covariance body its P or,
//            without one, its P_sym, the transition-column body the carried columns read out instead of the cov_init state --, N == 0
//            reads nothing else, and a gathered state whose q[0] is NaN (the rows of a refused carry) gives NaN in every field.
// Everything behind the gather is the same code, so the forms agree bit for bit wherever they gather the same doubles.
// The argument blocks enter a body BY VALUE.  By reference, a per-lane choice among pointer fields (the transition-column body's
// J_b / H_b / O_b) becomes a choice among their ADDRESSES in the kernel-argument segment and a vector load of the chosen one: a
// dependent global load in front of the gather, where the by-value form selects among values the scalar unit has loaded.
#pragma once

namespace {

struct QueryAt {
    long long w;      // the window, clamped into range (a query without one reads window 0 and stores NaN)
    bool none;        // there is no window to ask: every requested field is NaN
    int n, i;         // the window's intervals, and the largest knot index in [0, n] with t_i <= t_q
    double kt[7];     // the stamp and the reading of knot i
};

// The window is named by the caller: w = qwin[k], clamped into [0, W).
//   search   i = the largest knot index in [0, n] with t_i <= t_q (0 when t_q lies before the window), by bisection over the
//            window's stamps.  The trip count ceil(log2(N + 1)) is a launch argument -- the same for every lane --, the sum of the
//            steps = 2^trips - 1 >= N reaches every index of [0, n], every probe is clamped into [0, n], and a probe past n never
//            moves i: whatever the stamps hold (the search assumes them finite and non-decreasing), no read leaves the knots
//            [k0, k0 + n].  A NaN t_q compares false everywhere: i = 0.
// Knot i is requested here and first used behind the gather of the base row, so the two are in flight together.
struct WindowLocator {
    static __device__ __forceinline__ QueryAt find(const QueryArgs &A, long long k, double tq) {
        const long long w = min(max((long long)A.qwin[k], 0ll), A.W - 1);
        const int n = A.count ? min(max(A.count[w], 0), A.N) : A.N;
        const double *kn = A.knots + (A.first ? A.first[w] : w * (long long)(A.N + 1)) * 7;
        int i = 0;
        for (int s = A.trips - 1; s >= 0; --s) {
            const int probe = i + (1 << s);
            const double t = kn[min(probe, n) * 7];
            i = (probe <= n && t <= tq) ? probe : i;
        }
        QueryAt q;
        q.w = w; q.none = false; q.n = n; q.i = i;
#pragma unroll
        for (int e = 0; e < 7; e++) q.kt[e] = kn[i * 7 + e];
        return q;
    }
    static __device__ __forceinline__ bool reads_rows(const QueryArgs &A) { return A.N > 0; }
    static __device__ __forceinline__ void note_window(const QueryArgs &, long long, const QueryAt &, bool) {}
};

}  // namespace
