// cpi_query_kernels.hpp -- the measurement at arbitrary times inside a window (cpi_query_batch): query_mean_body and, over it,
// cpi_query_kernel.  The open form (cpi_query_open_kernels.hpp) and the stream form (cpi_query_stream_kernels.hpp) call the same body.
// Part of a kernel translation unit (included after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once
#include "cpi_query_locate.hpp"

namespace {

// Query k asks for the measurement of window w at time t_q = qtime[k].  The rows of cpi_preintegrate_running already hold the
// state after every interval, so a query is one gather and at most one partial interval:
//   search   the locator's (cpi_query_locate.hpp): the window, the interval i that holds t_q, and knot i;
//   gather   the base state = row w N + i - 1 (i == 0: the zero state) and knot i, both requested before either is used;
//   step     when t_i < t_q and i < n: feed_IMU(t_i, t_q, w_i, a_i, w_i, a_i) on the base state -- the reading held as the
//            reference holds it over a window's tail (GraphSolver_IMU.cpp:64-69) -- with the rotation rebuilt from the row's
//            quaternion.  Otherwise (t_q on a stamp, before t_0, at or past t_n) the row's own doubles are selected: they never pass
//            through quat_2_Rot / rot_2_quat, so the output is the row bit for bit.  The step runs for every lane (an inactive
//            one with dt = 0) and the selection is per lane: no divergence beyond what mean_step has itself;
//   store    one lane per query for the arithmetic, not for the stores: the 64 results of a wavefront are parked in LDS record-major
//            (pitch 11 doubles: odd, so the lanes' records start in distinct banks) and leave field by field as consecutive 16-byte
//            non-temporal stores -- every field of 64 consecutive queries is one contiguous run of the output array, as in
//            cpi_predict_kernel.  The Jacobians (five 72-byte matrices per query) take turns in the same area.
// A NaN t_q (no step), a query without a window and, OPEN, a NaN base row are turned into NaN in every requested field at the end.
// A launch without rows to read (reads_rows: N == 0, or a stream call that asked for qwin_out alone) gathers nothing.
constexpr int QRY_PITCH = 11;   // DT 1 + alpha 3 + beta 3 + q 4; a 3 x 3 matrix (9) fits as well

// Field of F doubles per query at offset `off` of the staged records -> the nq * F consecutive doubles of its output run.
template <int F>
__device__ __forceinline__ void query_flush(const double *stage, int off, double *field, long long q0, int nq, int lane) {
    double *dst = field + q0 * F;
    const int total = nq * F;
    auto at = [&](int e) { const int g = e / F; return stage[g * QRY_PITCH + off + (e - g * F)]; };
    for (int p = lane; 2 * p + 1 < total; p += 64) st16_nt(dst + 2 * p, at(2 * p), at(2 * p + 1));
    if ((total & 1) && lane == 0) dst[total - 1] = at(total - 1);
}

template <int MODEL, bool JAC, bool AVG, bool OPEN, class Loc, class Args>
__device__ __forceinline__ void query_mean_body(const Args A, const QueryBase B) {
    static_assert(!(JAC && MODEL == 2), "model 2's Jacobians are read out of the state transition matrix");
    static_assert(!(AVG && MODEL == 1), "with the reading held, model 1's averaging is the identity (x + x) * 0.5");
    __shared__ __attribute__((aligned(16))) double sOut[64 * QRY_PITCH];
    const int lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * 64;
    const int nq = (int)min(64ll, A.Q - q0);
    const long long k = q0 + min(lane, nq - 1);      // lanes past the last query redo it and store nothing
    const double tq = A.qtime[k];
    const QueryAt at = Loc::find(A, k, tq);
    const long long w = at.w;
    const int n = at.n, i = at.i;
    const double *kt = at.kt;
    Loc::note_window(A, k, at, lane < nq);

    // ---- the base row (knot i is in flight with it)
    const bool has = OPEN || i > 0;
    const bool fromb = OPEN && i == 0;               // the state before knot 0: the base row
    const cpi_outputs &R = A.rows, &RB = B.rows;
    MeanState<JAC> st;
    mean_init(st);
    double bDT = 0.0;
    V3 bal = mk(0, 0, 0), bbe = mk(0, 0, 0);
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    if (OPEN || Loc::reads_rows(A)) {                // wave-uniform.  Otherwise every query is the zero state
        const long long row = fromb ? w * (long long)B.N + (B.N - 1) : w * (long long)A.N + max(i - 1, 0);
        const double rDT = (fromb ? RB.DT : R.DT)[row];
        const V3 ral = ldv3((fromb ? RB.alpha : R.alpha) + row * 3), rbe = ldv3((fromb ? RB.beta : R.beta) + row * 3);
        const Q4 rq = ldq4((fromb ? RB.q : R.q) + row * 4);
        if (JAC) {
            const M3 rJq = ldm3_cm((fromb ? RB.J_q : R.J_q) + row * 9), rJa = ldm3_cm((fromb ? RB.J_a : R.J_a) + row * 9),
                     rJb = ldm3_cm((fromb ? RB.J_b : R.J_b) + row * 9), rHa = ldm3_cm((fromb ? RB.H_a : R.H_a) + row * 9),
                     rHb = ldm3_cm((fromb ? RB.H_b : R.H_b) + row * 9);
            if (has) { st.Jq = rJq; st.Ja = rJa; st.Jb = rJb; st.Ha = rHa; st.Hb = rHb; }
        }
        if (has) { bDT = rDT; bal = ral; bbe = rbe; bq = rq; }
    }
    st.DT = bDT; st.alpha = bal; st.beta = bbe;
    st.R = quat_2_Rot(bq);                           // [0 0 0 1] gives the identity exactly

    const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));

    // ---- the partial interval [t_i, t_q] with reading i held; inactive: an exact no-op (JAC: the state is not touched at all)
    const bool step = (i < n) && (tq > kt[0]);
    const V3 wi = mk(kt[1], kt[2], kt[3]), ai = mk(kt[4], kt[5], kt[6]);
    mean_step<MODEL, JAC, AVG>(st, kt[0], tq, wi, ai, wi, ai, bw, ba, gk, step);
    const Q4 sq = rot_2_quat(st.R);

    const bool bad = (tq != tq) || (OPEN && bq.x != bq.x) || at.none;
    const double qnan = __builtin_nan("");
    auto pick = [&](double stepped, double base) { return bad ? qnan : (step ? stepped : base); };
    {
        double *d = sOut + lane * QRY_PITCH;
        d[0] = pick(st.DT, bDT);
        d[1] = pick(st.alpha.x, bal.x); d[2] = pick(st.alpha.y, bal.y); d[3] = pick(st.alpha.z, bal.z);
        d[4] = pick(st.beta.x, bbe.x); d[5] = pick(st.beta.y, bbe.y); d[6] = pick(st.beta.z, bbe.z);
        d[7] = pick(sq.x, bq.x); d[8] = pick(sq.y, bq.y); d[9] = pick(sq.z, bq.z); d[10] = pick(sq.w, bq.w);
    }
    wave_lds_fence();
    if (A.out.DT) query_flush<1>(sOut, 0, A.out.DT, q0, nq, lane);
    if (A.out.alpha) query_flush<3>(sOut, 1, A.out.alpha, q0, nq, lane);
    if (A.out.beta) query_flush<3>(sOut, 4, A.out.beta, q0, nq, lane);
    if (A.out.q) query_flush<4>(sOut, 7, A.out.q, q0, nq, lane);
    if (JAC) {
        auto put = [&](double *field, const M3 &J) {
            if (!field) return;                      // wave-uniform
            wave_lds_fence();                        // in-order DS: the previous flush has read the area
            double *d = sOut + lane * QRY_PITCH;
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int r = 0; r < 3; r++) d[c * 3 + r] = bad ? qnan : J.m[r][c];
            wave_lds_fence();
            query_flush<9>(sOut, 0, field, q0, nq, lane);
        };
        put(A.out.J_q, st.Jq); put(A.out.J_a, st.Ja); put(A.out.J_b, st.Jb); put(A.out.H_a, st.Ha); put(A.out.H_b, st.Hb);
    }
}

template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_query_kernel(QueryArgs A) {
    query_mean_body<MODEL, JAC, AVG, false, WindowLocator>(A, QueryBase());
}

}  // namespace
