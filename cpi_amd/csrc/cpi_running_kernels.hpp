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
    static_assert(!(JAC && MODEL == 2), "model 2's Jacobians are read out of the state transition matrix");
    constexpr int T = CPI_RUN_T;
    constexpr int P1 = T | 1, P3 = (3 * T) | 1, P4 = (4 * T) | 1;   // odd pitches: a lane's slots start in distinct banks
    constexpr bool GSEG = MULTI && MODEL == 2;
    __shared__ double sDT[64 * P1], sAl[64 * P3], sBe[64 * P3], sQ[64 * P4];
    __shared__ long long s_rowbase[64];
    __shared__ int s_lo[64], s_hi[64];

    const int lane = threadIdx.x;
    const int L = MULTI ? L_arg : 1;
    const int WPB = 64 / L;
    const int grp = lane / L, l = lane - grp * L;
    long long w = (long long)blockIdx.x * WPB + grp;
    const bool valid = (w < A.W) && (grp < WPB);       // L not a power of two leaves 64 - WPB L idle lanes
    if (grp >= WPB) w = (long long)blockIdx.x * WPB;
    if (w >= A.W) w = A.W - 1;
    const int n = A.count ? min(max(A.count[w], 0), A.N) : A.N;
    const long long k0 = A.first ? A.first[w] : w * (long long)(A.N + 1);
    const int per = (A.N + L - 1) / L;                 // rows per lane: wave-uniform
    const int r0 = min(A.N, l * per);
    const int nrows = valid ? min(A.N - r0, per) : 0;
    // knot i of the window, never past its last one (what lies behind belongs to the caller; the repeated knot gives dt = 0)
    auto knot = [&](int i) { return A.knots + (k0 + min(i, n)) * 7; };

    const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));

    MeanState<JAC> st;
    mean_init(st);
    int lead = 0;        // leading rows of this lane before its first integrated interval (held back for the fix-up)
    int src = -1;        // the wavefront lane whose last row those rows repeat (-1: none -- the scanned state is exact)
    if constexpr (MULTI) {
        GravAcc ga;
        grav_init(ga);
        double pk[7], nx[7];
        {
            const double *a = knot(r0), *b = knot(r0 + 1);
#pragma unroll
            for (int i = 0; i < 7; i++) { pk[i] = a[i]; nx[i] = b[i]; }
        }
        bool seen = false;
        for (int t = 0; t < per; ++t) {
            double q[7];
#pragma unroll
            for (int i = 0; i < 7; i++) q[i] = nx[i];
            {
                const double *b = knot(r0 + t + 2);
#pragma unroll
                for (int i = 0; i < 7; i++) nx[i] = b[i];
            }
            const bool act = t < nrows;
            const bool moves = act && (q[0] - pk[0] > 0);
            if (!seen && !moves && act) lead++;
            seen = seen || moves;
            if constexpr (GSEG)
                mean_step_v2seg<AVG>(st, ga, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                     mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, act);
            else
                mean_step<MODEL, JAC, AVG>(st, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                           mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, gk, act);
#pragma unroll
            for (int i = 0; i < 7; i++) pk[i] = q[i];
        }
        // ordered inclusive scan: lane l <- (l - d) o l, earlier on the left
        for (int d = 1; d < L; d <<= 1) {
            MeanState<JAC> B = run_shfl_up(st, d);
            GravAcc gB;
            if constexpr (GSEG) gB = run_shfl_up(ga, d);
            if (l >= d) {
                if constexpr (GSEG) { grav_combine(gB, B, ga, st); ga = gB; }   // before mean_combine: needs B.R and st.DT as they are
                mean_combine(B, st);
                st = B;
            }
        }
        // exclusive: the state at this lane's first knot
        {
            MeanState<JAC> B = run_shfl_up(st, 1);
            GravAcc gB;
            if constexpr (GSEG) gB = run_shfl_up(ga, 1);
            if (l == 0) { mean_init(B); if constexpr (GSEG) grav_init(gB); }
            st = B;
            if constexpr (GSEG) grav_apply(st, gB, gk);
        }
        // whose last row do the held-back rows repeat: the nearest earlier lane of the window that integrated anything
        const unsigned long long moved = __ballot(lead < nrows);
        const unsigned long long below = moved & ((1ull << lane) - 1ull) & ~((1ull << (grp * L)) - 1ull);
        src = below ? 63 - __builtin_clzll(below) : -1;
        if (src < 0) lead = 0;
    }

    s_rowbase[lane] = w * (long long)A.N + r0;
    s_lo[lane] = lead;
    s_hi[lane] = nrows;
    const bool wm = A.write_means != 0;
    auto stage = [&](int tt, const RunRow &r) {
        sDT[lane * P1 + tt] = r.DT;
        double *a = sAl + lane * P3 + tt * 3, *b = sBe + lane * P3 + tt * 3, *c = sQ + lane * P4 + tt * 4;
        a[0] = r.alpha.x; a[1] = r.alpha.y; a[2] = r.alpha.z;
        b[0] = r.beta.x; b[1] = r.beta.y; b[2] = r.beta.z;
        c[0] = r.q.x; c[1] = r.q.y; c[2] = r.q.z; c[3] = r.q.w;
    };
    auto flush = [&](int tb) {
        __syncthreads();
        if (A.out.DT) run_flush<1, P1>(sDT, A.out.DT, s_rowbase, s_lo, s_hi, tb, lane);
        if (A.out.alpha) run_flush<3, P3>(sAl, A.out.alpha, s_rowbase, s_lo, s_hi, tb, lane);
        if (A.out.beta) run_flush<3, P3>(sBe, A.out.beta, s_rowbase, s_lo, s_hi, tb, lane);
        if (A.out.q) run_flush<4, P4>(sQ, A.out.q, s_rowbase, s_lo, s_hi, tb, lane);
        __syncthreads();
    };
    auto store_jac = [&](long long row, const MeanState<JAC> &s) {
        if (A.out.J_q) stm3_cm(A.out.J_q + row * 9, s.Jq);
        if (A.out.J_a) stm3_cm(A.out.J_a + row * 9, s.Ja);
        if (A.out.J_b) stm3_cm(A.out.J_b + row * 9, s.Jb);
        if (A.out.H_a) stm3_cm(A.out.H_a + row * 9, s.Ha);
        if (A.out.H_b) stm3_cm(A.out.H_b + row * 9, s.Hb);
    };
    const long long row0 = w * (long long)A.N + r0;

    // ---- the walk: one row per interval
    RunRow last;
    {
        double pk[7], nx[7];
        {
            const double *a = knot(r0), *b = knot(r0 + 1);
#pragma unroll
            for (int i = 0; i < 7; i++) { pk[i] = a[i]; nx[i] = b[i]; }
        }
        for (int tb = 0; tb < per; tb += T) {
            const int te = min(T, per - tb);
#pragma unroll 1
            for (int tt = 0; tt < te; ++tt) {
                const int t = tb + tt;
                double q[7];
#pragma unroll
                for (int i = 0; i < 7; i++) q[i] = nx[i];
                {
                    const double *b = knot(r0 + t + 2);
#pragma unroll
                    for (int i = 0; i < 7; i++) nx[i] = b[i];
                }
                mean_step<MODEL, JAC, AVG>(st, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                           mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, gk, t < nrows);
#pragma unroll
                for (int i = 0; i < 7; i++) pk[i] = q[i];
                last.DT = st.DT; last.alpha = st.alpha; last.beta = st.beta; last.q = rot_2_quat(st.R);
                if (wm) stage(tt, last);
                if constexpr (JAC) {
                    if (A.write_jac && t >= lead && t < nrows) store_jac(row0 + t, st);
                }
            }
            if (wm) flush(tb);
        }
    }

    // ---- the fix-up: held-back rows repeat the last row of lane `src`
    if constexpr (MULTI) {
        if (__any(lead > 0)) {
            const int sl = max(src, 0);
            RunRow y;
            y.DT = __shfl(last.DT, sl);
            y.alpha = mk(__shfl(last.alpha.x, sl), __shfl(last.alpha.y, sl), __shfl(last.alpha.z, sl));
            y.beta = mk(__shfl(last.beta.x, sl), __shfl(last.beta.y, sl), __shfl(last.beta.z, sl));
            y.q.x = __shfl(last.q.x, sl); y.q.y = __shfl(last.q.y, sl); y.q.z = __shfl(last.q.z, sl); y.q.w = __shfl(last.q.w, sl);
            MeanState<JAC> ys;
            if constexpr (JAC) {
                ys.Jq = run_shfl(st.Jq, sl); ys.Ja = run_shfl(st.Ja, sl); ys.Jb = run_shfl(st.Jb, sl);
                ys.Ha = run_shfl(st.Ha, sl); ys.Hb = run_shfl(st.Hb, sl);
            }
            __syncthreads();
            s_lo[lane] = 0;
            s_hi[lane] = lead;
            const int maxlead = __builtin_amdgcn_readfirstlane(wave_max(lead));
            for (int tb = 0; tb < maxlead; tb += T) {
                if (wm) {
#pragma unroll 1
                    for (int tt = 0; tt < T; ++tt) stage(tt, y);
                    flush(tb);
                }
                if constexpr (JAC) {
                    if (A.write_jac)
                        for (int t = tb; t < min(tb + T, lead); ++t) store_jac(row0 + t, ys);
                }
            }
        }
    }
}

}  // namespace
