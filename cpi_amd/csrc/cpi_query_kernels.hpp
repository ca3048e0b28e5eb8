// cpi_query_kernels.hpp -- the measurement at arbitrary times inside a window (cpi_query_batch): cpi_query_kernel.
// Part of the translation unit cpi_query.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

// Query k asks for the measurement of window w = qwin[k] at time t_q = qtime[k].  The rows of cpi_preintegrate_running already
// hold the state after every interval, so a query is one gather and at most one partial interval:
//   search   i = the largest knot index in [0, n] with t_i <= t_q (0 when t_q lies before the window), by bisection over the
//            window's stamps.  The trip count ceil(log2(N + 1)) is a launch argument -- the same for every lane --, every probe is
//            clamped into [0, n], and a probe past n never moves i: whatever the stamps hold (the search assumes them finite and
//            non-decreasing), no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
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
// A NaN t_q compares false everywhere (i = 0, no step) and is turned into NaN in every requested field at the end.
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

template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_query_kernel(QueryArgs A) {
    static_assert(!(JAC && MODEL == 2), "model 2's Jacobians are read out of the state transition matrix");
    static_assert(!(AVG && MODEL == 1), "with the reading held, model 1's averaging is the identity (x + x) * 0.5");
    __shared__ __attribute__((aligned(16))) double sOut[64 * QRY_PITCH];
    const int lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * 64;
    const int nq = (int)min(64ll, A.Q - q0);
    const long long k = q0 + min(lane, nq - 1);      // lanes past the last query redo it and store nothing
    const long long w = min(max((long long)A.qwin[k], 0ll), A.W - 1);
    const double tq = A.qtime[k];
    const int n = A.count ? min(max(A.count[w], 0), A.N) : A.N;
    const double *kn = A.knots + (A.first ? A.first[w] : w * (long long)(A.N + 1)) * 7;

    // ---- the interval: sum of the steps = 2^trips - 1 >= N, so every index of [0, n] is reachable
    int i = 0;
    for (int s = A.trips - 1; s >= 0; --s) {
        const int probe = i + (1 << s);
        const double t = kn[min(probe, n) * 7];
        i = (probe <= n && t <= tq) ? probe : i;
    }

    // ---- knot i and the base row, in flight together
    double kt[7];
#pragma unroll
    for (int j = 0; j < 7; j++) kt[j] = kn[i * 7 + j];
    const bool has = i > 0;
    MeanState<JAC> st;
    mean_init(st);
    double bDT = 0.0;
    V3 bal = mk(0, 0, 0), bbe = mk(0, 0, 0);
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    if (A.N > 0) {                                   // wave-uniform.  N == 0: rows is not read, every query is the zero state
        const long long row = w * (long long)A.N + max(i - 1, 0);
        const double rDT = A.rows.DT[row];
        const V3 ral = ldv3(A.rows.alpha + row * 3), rbe = ldv3(A.rows.beta + row * 3);
        const Q4 rq = ldq4(A.rows.q + row * 4);
        if (JAC) {
            const M3 rJq = ldm3_cm(A.rows.J_q + row * 9), rJa = ldm3_cm(A.rows.J_a + row * 9), rJb = ldm3_cm(A.rows.J_b + row * 9),
                     rHa = ldm3_cm(A.rows.H_a + row * 9), rHb = ldm3_cm(A.rows.H_b + row * 9);
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

    const bool bad = tq != tq;
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

}  // namespace
