// cpi_running_kernels.hpp -- the mean (+ model-1 analytic Jacobian) recursion with a row after EVERY interval
// (cpi_preintegrate_running): cpi_mean_running_kernel.
// Part of the translation unit cpi_running.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

// Row w N + i of the outputs = the measurement of window w after interval i.  Lane l of the L lanes of a window owns the ROWS
// [l per, (l + 1) per), per = ceil(N / L) -- rows, not intervals: an interval past the window's count (or a skipped one) is an
// exact no-op of the recursion, so its row repeats the state and needs no special case, and the trip count is wave-uniform.
//
//   pass 1 (L > 1)  every lane integrates its intervals from the identity (model 2: from the raw specific force with the
//                   segment's gravity response, mean_step_v2seg) -- what a lane of cpi_mean_kernel does;
//   scan            an ordered Hillis-Steele scan over the L summaries with mean_combine / grav_combine, shifted by one lane:
//                   the state at the lane's first knot (lane 0: the zero state).  For model 2 the gravity response is applied
//                   there (grav_apply), so the lane holds a TRUE prefix state in the window-start frame;
//   walk            the lane integrates its intervals again from that state with the ordinary mean_step and emits a row per
//                   interval;
//   fix-up          the leading rows of a lane whose first intervals are no-ops must repeat the PREVIOUS lane's last row bit for
//                   bit (the header's rule: a skipped interval repeats the previous row), but the scanned prefix and the walked
//                   state differ in the last bits.  Those rows are held back in the walk and written afterwards from the last
//                   row of the nearest earlier lane that integrated anything (none: the zero state, which the scan yields
//                   exactly).  Wave-uniformly skipped when no lane needs it.
//
// Stores.  A lane's rows are consecutive in memory, neighbouring lanes' rows lie N rows apart: a direct store per interval
// would touch 64 different 128-byte lines per instruction, 8 bytes each.  The means of T = CPI_RUN_T intervals are staged in LDS
// (one odd-pitched slab per output array) and leave as flat copies in which consecutive lanes write consecutive doubles of one
// lane-segment's run: T * 24 (alpha, beta), T * 32 (q), T * 8 (DT) contiguous bytes per run.  T = 6 keeps the slabs at 36 KB, four
// wavefronts per CU (T = 7 is 40 KB: exactly a quarter of the CU's LDS, nothing to spare).  Measured on MI355X, 1 M x 50 means only:
// stores straight from registers (no LDS, three wavefronts per SIMD) 4.22 ms, T = 3 3.08 ms, T = 4 2.67-2.70 ms, T = 6 2.48-2.55 ms
// (DESIGN.md 3.1c).  The Jacobian rows (five 72-byte matrices per row, 61 doubles of live state) are stored from registers.
// Knots are read straight into registers one interval ahead (the lines a lane touches stay in the L1 / L2 over the 2-3
// intervals that share them).
#ifndef CPI_RUN_T
#define CPI_RUN_T 6
#endif
#ifndef CPI_RUN_FLUSH_UNROLL
#define CPI_RUN_FLUSH_UNROLL 6
#endif
#define CPI_RUN_STR2(x) #x
#define CPI_RUN_STR(x) CPI_RUN_STR2(x)

template <bool JAC>
__device__ __forceinline__ MeanState<JAC> run_shfl_up(const MeanState<JAC> &s, int d) {
    MeanState<JAC> r;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) r.R.m[i][j] = __shfl_up(s.R.m[i][j], d);
    r.alpha = mk(__shfl_up(s.alpha.x, d), __shfl_up(s.alpha.y, d), __shfl_up(s.alpha.z, d));
    r.beta = mk(__shfl_up(s.beta.x, d), __shfl_up(s.beta.y, d), __shfl_up(s.beta.z, d));
    r.DT = __shfl_up(s.DT, d);
    if (JAC) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                r.Jq.m[i][j] = __shfl_up(s.Jq.m[i][j], d); r.Ja.m[i][j] = __shfl_up(s.Ja.m[i][j], d);
                r.Jb.m[i][j] = __shfl_up(s.Jb.m[i][j], d); r.Ha.m[i][j] = __shfl_up(s.Ha.m[i][j], d);
                r.Hb.m[i][j] = __shfl_up(s.Hb.m[i][j], d);
            }
        r.Oa = s.Oa; r.Ob = s.Ob;
    }
    return r;
}
__device__ __forceinline__ GravAcc run_shfl_up(const GravAcc &g, int d) {
    GravAcc r;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { r.Gam.m[i][j] = __shfl_up(g.Gam.m[i][j], d); r.Lam.m[i][j] = __shfl_up(g.Lam.m[i][j], d); }
    return r;
}
__device__ __forceinline__ M3 run_shfl(const M3 &A, int src) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) r.m[i][j] = __shfl(A.m[i][j], src);
    return r;
}

// One output array's slab -> memory.  Element idx = k 64 + lane of the flat copy belongs to lane-segment idx / (T F) at offset
// idx % (T F): consecutive lanes write consecutive doubles of one run.  Row t of segment s is written when lo[s] <= t < hi[s].
template <int F, int P>
__device__ __forceinline__ void run_flush(const double *slab, double *gp, const long long *rowbase, const int *lo, const int *hi,
                                          int tb, int lane) {
    constexpr int TF = CPI_RUN_T * F;
    // (fully unrolled, the compiler hoists every slab read above the first store: 100 more live registers and scratch)
    _Pragma(CPI_RUN_STR(unroll CPI_RUN_FLUSH_UNROLL))
    for (int k = 0; k < TF; ++k) {
        const int idx = k * 64 + lane;
        const int seg = idx / TF, off = idx - seg * TF;
        const int t = tb + off / F;
        if (t >= lo[seg] && t < hi[seg]) gp[(rowbase[seg] + tb) * F + off] = slab[seg * P + off];
    }
}

// The emitted means of one row
struct RunRow {
    double DT;
    V3 alpha, beta;
    Q4 q;
};

// MULTI: L > 1 lanes per window (L is a launch argument: the lane split costs no instantiation per lane count)
template <int MODEL, bool JAC, bool AVG, bool MULTI>
__global__ __launch_bounds__(64) void cpi_mean_running_kernel(PreArgs A, int L_arg) {
    constexpr bool CUT = false;
    constexpr bool CARRY = false;
    const CarryArgs CA = CarryArgs();
#include "cpi_running_body.inc"
}

// The same kernel for windows cut out of a stream in flight (cpi_preintegrate_stream[s]_running): window w is read in place
// through first / count / tstart / tend as cpi_cut_windows_kernel / cpi_cut_runs_kernel left them in the workspace (PreArgs).
// A kernel of its own name over the shared body, so that cpi_mean_running_kernel compiles to the code it had before.
template <int MODEL, bool JAC, bool AVG, bool MULTI>
__global__ __launch_bounds__(64) void cpi_mean_stream_running_kernel(PreArgs A, int L_arg) {
    constexpr bool CUT = true;
    constexpr bool CARRY = false;
    const CarryArgs CA = CarryArgs();
#include "cpi_running_body.inc"
}

// cpi_preintegrate_running_resume: cpi_mean_running_kernel from and to carry records (cpi_args.hpp: CarryArgs; this kernel always
// owns the tag, the means and -- JAC -- the Jacobian block of carry_out).  Lane 0 starts from the record instead of the zero state;
// a lane before which nothing was integrated shows the carried state itself; the record is stored from the walked state of the
// lane whose last row is row N - 1.  Again a kernel of its own name over the shared body.
template <int MODEL, bool JAC, bool AVG, bool MULTI>
__global__ __launch_bounds__(64) void cpi_mean_running_carry_kernel(PreArgs A, CarryArgs CA, int L_arg) {
    constexpr bool CUT = false;
    constexpr bool CARRY = true;
#include "cpi_running_body.inc"
}

}  // namespace
