// cpi_query_stream_kernels.hpp -- the query family by ABSOLUTE time over IMU stream(s) read in place (cpi_query_stream_batch):
// cpi_squery_mean_kernel, cpi_squery_cov_kernel, cpi_squery_jac2_kernel.
// Part of the translation unit cpi_query_stream.hip (included there after cpi_math.hpp / cpi_device_util.hpp and cpi_query_kernels.hpp,
// whose staged store path the mean kernel shares).  The lookup helpers at the top are plain inline functions: the
// CPU emulation (tests/hostsim/hostsim_query_stream.cpp) includes this header after cpi_math.hpp and runs the code the kernels run.
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

// sigma^2 of the four diagonal blocks of Q_c (PreArgs::q4), an argument of the covariance kernel alone
struct SQueryNoise { double q4[4]; };

// What the three kernels share: query k -> its window, its interval and knot i as a plain window would hold it.
struct SQuery {
    long long w;      // the window, clamped into [0, U) (an empty run reads window 0 and stores NaN)
    bool none;        // the run has no update times
    int n, i;
    double kt[7];     // stamp(i) and the reading of knot i
};
__device__ __forceinline__ SQuery squery_find(const StreamQueryArgs &A, long long k, double tq) {
    SQuery q;
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

// cpi_query_kernel over stream(s): the prologue is squery_find, everything behind it is that kernel's (cpi_query_kernels.hpp).
// A launch whose rows hold no means (rows.DT == NULL: the call asked for qwin_out alone) looks the windows up and stores nothing else.
template <int MODEL, bool JAC, bool AVG>
__global__ __launch_bounds__(64) void cpi_squery_mean_kernel(StreamQueryArgs A) {
    static_assert(!(JAC && MODEL == 2), "model 2's Jacobians are read out of the state transition matrix");
    static_assert(!(AVG && MODEL == 1), "with the reading held, model 1's averaging is the identity (x + x) * 0.5");
    __shared__ __attribute__((aligned(16))) double sOut[64 * QRY_PITCH];
    const int lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * 64;
    const int nq = (int)min(64ll, A.Q - q0);
    const long long k = q0 + min(lane, nq - 1);      // lanes past the last query redo it and store nothing
    const double tq = A.qtime[k];
    const SQuery sq_ = squery_find(A, k, tq);
    const long long w = sq_.w;
    const int n = sq_.n, i = sq_.i;
    const double *kt = sq_.kt;
    if (A.qwin_out && lane < nq) A.qwin_out[k] = sq_.none ? -1 : (int)w;

    const bool has = i > 0;
    MeanState<JAC> st;
    mean_init(st);
    double bDT = 0.0;
    V3 bal = mk(0, 0, 0), bbe = mk(0, 0, 0);
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    if (A.N > 0 && A.rows.DT) {                      // wave-uniform.  N == 0: rows is not read, every query is the zero state
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

    const bool bad = (tq != tq) || sq_.none;
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

// cpi_query_cov_kernel over stream(s) (cpi_query_cov_kernels.hpp): one lane group per query, every lane of a group runs the lookup
// (its loads are broadcasts).
template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_SQUERY_WPS) void cpi_squery_cov_kernel(StreamQueryArgs A, SQueryNoise NZ) {
    static_assert(!(AVG && MODEL == 1), "with the reading held, model 1's averaging is the identity (x + x) * 0.5");
    typedef CovDims<MODEL> D;
    constexpr int GROUP = D::GROUP;   // lanes per query
    constexpr int G = 64 / GROUP;     // queries per wavefront
    constexpr int EP = EXCH_PITCH;
    constexpr int IRD = IrPitch<MODEL>::V;
    constexpr int R0 = 10;            // pitch of a group's start rotation (9 doubles, rows kept 16-B aligned)
    __shared__ __attribute__((aligned(16))) double irs[G * IRD];               // the interval record of each group
    __shared__ __attribute__((aligned(256))) double exch[exch_doubles(G)];   // transpose exchange (placement: cpi_math.hpp)
    __shared__ __attribute__((aligned(16))) double r0s[G * R0];                // rotation at the start of the interval

    const int lane = threadIdx.x;
    const int g = lane / GROUP, j = lane % GROUP;
    const long long q0 = (long long)blockIdx.x * G;
    const bool valid = q0 + g < A.Q;
    const long long k = min(q0 + g, A.Q - 1);        // groups past the last query redo it and store nothing
    const double tq = A.qtime[k];
    const SQuery sq_ = squery_find(A, k, tq);
    const long long w = sq_.w;
    const int n = sq_.n, i = sq_.i;
    const double *kt = sq_.kt;
    if (A.qwin_out && valid && j == 0) A.qwin_out[k] = sq_.none ? -1 : (int)w;

    const double q4[4] = { NZ.q4[0], NZ.q4[1], NZ.q4[2], NZ.q4[3] };
    const int jl = cov_col_of_lane<MODEL>(j);
    const int jj = (jl < D::NPCOL) ? jl : D::NCOL;                  // column owned by this lane; NCOL = idle
    const int cs = (MODEL == 2 && jj >= 15 && jj < D::NPCOL) ? jj - 15 : jj;   // the column of the 15 x 15 row it starts from
    CovLane<MODEL> Ln;
    cov_init(Ln, jj, q4);

    // ---- the base row's quaternion and this lane's column of S
    const bool has = i > 0;
    double S[D::NR];
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    if (A.N > 0) {                                   // wave-uniform.  N == 0: rows is not read, S is zero
        const long long row = w * (long long)A.N + max(i - 1, 0);
        const Q4 rq = ldq4(A.rows.q + row * 4);
        const int c = min(cs, 14);                   // idle lanes load column 14 and drop it
        const bool own = has && cs < 15;
        if (A.rows.P) {
            const double *p = A.rows.P + row * 225 + c * 15;
#pragma unroll
            for (int r = 0; r < 15; r++) S[r] = own ? p[r] : 0.0;
        } else {
            const double *p = A.rows.P_sym + row * CPI_TRI_DOUBLES;
#pragma unroll
            for (int r = 0; r < 15; r++) S[r] = own ? p[(r <= c) ? r + c * (c + 1) / 2 : c + r * (r + 1) / 2] : 0.0;
        }
        if (has) bq = rq;
    } else {
#pragma unroll
        for (int r = 0; r < 15; r++) S[r] = 0.0;
    }
    if (MODEL == 2) {
        constexpr int o = (D::NR >= 18) ? 15 : 0;    // (model 1 never takes this branch)
        S[o] = S[0]; S[o + 1] = S[1]; S[o + 2] = S[2];
    }
#pragma unroll
    for (int r = 0; r < D::NR; r++) Ln.P0[r] = S[r];

    double *ex_g = exch + g * EXCH_WIN;
    const double *ex_row = exch + (cov_row_off<MODEL>(G, g, jj) & ~1);   // 16-B aligned rows, said explicitly (cov_body)
    const int hoff = cov_h_offset<MODEL>(jj);        // ZERO: no lane owns a theta_klin transition column
    double *ir = irs + g * IRD;
    double *r0 = r0s + g * R0;
    for (int e = lane; e < exch_doubles(G); e += 64) exch[e] = 0.0;
    __syncthreads();
    cov_exch_init<MODEL>(exch, G, jj, q4);

    // ---- the record of the partial interval [t_i, t_q] with reading i held; no step: dt = 0, an exact no-op of the recursion
    const bool step = (i < n) && (tq > kt[0]);
    if (j == 0) {
        const M3 R_old = quat_2_Rot(bq);             // [0 0 0 1] gives the identity exactly
        const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
        V3 gk = mk(0, 0, 0);
        if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));
        const V3 wi = mk(kt[1], kt[2], kt[3]), ai = mk(kt[4], kt[5], kt[6]);
        const SampleRec r = make_sample_rec<MODEL, AVG>(kt[0], step ? tq : kt[0], wi, ai, wi, ai, bw, ba);
        finish_interval<MODEL, AVG>(r, R_old, gk, ir);
        rec_put_mat(r0, 0, R_old);
    }
    wave_lds_fence();

    // ---- one interval of cov_body's phase C: F x is lane-local, P F^T arrives through the exchange rows
    cov_begin<MODEL>(Ln, ir, hoff);
    M3 Rs = rec_mat(r0, 0);
#pragma unroll
    for (int stg = 0; stg < 4; ++stg) {
        double M[9];
        if (stg == 1 || stg == 3) Rs = cov_stage_rotation<MODEL>(ir, stg);   // stages 1 and 2 share R_mid
        cov_stage_M(Ln, stg, Rs, M);
        if (jj < D::NPCOL) {
#pragma unroll
            for (int rr = 0; rr < CovExchRows<MODEL>::V; rr++) ex_g[rr * EP + exch_pos<MODEL>(jj)] = M[rr];
        }
        wave_lds_fence();   // a wave's DS instructions execute in issue order: only the compiler must not reorder them
        if constexpr (CovPBySymmetry<MODEL>::V) {
            double mt[D::NR];
            const double *Xs = cov_stage_X(Ln, stg);
#pragma unroll
            for (int r = 0; r < D::NR; r++)
                mt[r] = (MODEL == 1) ? dpp_shr6_bank3(ex_row[exch_pos<MODEL>(r)], Xs[r])
                                     : dpp_shr6_bank3_oddrows(ex_row[exch_pos<MODEL>(r)], Xs[r]);
            cov_stage_finish_regs(Ln, stg, M, mt);
        } else {
            cov_stage_finish(Ln, stg, M, ex_row);
        }
    }

    // ---- columns jj < 15: the stepped column, or the gathered one bit for bit
    if (!valid || jj >= 15) return;
    const bool bad = (tq != tq) || sq_.none;
    double v[15];
#pragma unroll
    for (int r = 0; r < 15; r++) v[r] = bad ? __builtin_nan("") : (step ? Ln.P0[r] : S[r]);
    if (A.out.P) {
        double *p = A.out.P + k * 225 + jj * 15;
#pragma unroll
        for (int r = 0; r < 15; r++) p[r] = v[r];
    }
    if (A.out.P_sym) {   // rows 0 .. jj of the same column: the packed upper triangle (CPI_TRI_INDEX)
        double *p = A.out.P_sym + k * CPI_TRI_DOUBLES + jj * (jj + 1) / 2;
#pragma unroll
        for (int r = 0; r < 15; r++) if (r <= jj) p[r] = v[r];
    }
}

// cpi_query_stj_kernel over stream(s) (cpi_stj_kernels.hpp): 16 lanes per query, nine of them live, four queries per wavefront.
template <bool AVG>
__global__ __launch_bounds__(64, CPI_SQUERY_WPS) void cpi_squery_jac2_kernel(StreamQueryArgs A) {
    constexpr int MODEL = 2;
    typedef CovDims<MODEL> D;
    constexpr int GROUP = 16;         // lanes per query
    constexpr int G = 64 / GROUP;     // queries per wavefront
    constexpr int IRD = IrPitch<MODEL>::V;
    constexpr int R0 = 10;            // pitch of a group's start rotation (9 doubles, rows kept 16-B aligned)
    static_assert(D::NDCOL <= GROUP, "one lane per transition column");
    __shared__ __attribute__((aligned(16))) double irs[G * IRD];   // the interval record of each group
    __shared__ __attribute__((aligned(16))) double r0s[G * R0];    // rotation at the start of the interval

    const int lane = threadIdx.x;
    const int g = lane / GROUP, j = lane % GROUP;
    const long long q0 = (long long)blockIdx.x * G;
    const bool valid = q0 + g < A.Q;
    const long long k = min(q0 + g, A.Q - 1);        // groups past the last query redo it and store nothing
    const double tq = A.qtime[k];
    const SQuery sq_ = squery_find(A, k, tq);
    const long long w = sq_.w;
    const int n = sq_.n, i = sq_.i;
    const double *kt = sq_.kt;
    if (A.qwin_out && valid && j == 0) A.qwin_out[k] = sq_.none ? -1 : (int)w;

    const bool live = j < D::NDCOL;
    const int jj = live ? D::NPCOL + j : D::NCOL;    // column owned by this lane; NCOL = idle (a zero column)
    const int d = min(j, D::NDCOL - 1) / 3, c = min(j, D::NDCOL - 1) % 3;   // idle lanes load what lane 8 loads and drop it
    const double q4[4] = { 0.0, 0.0, 0.0, 0.0 };     // process noise enters covariance columns only
    CovLane<MODEL> Ln;
    cov_init(Ln, jj, q4);

    // ---- the base row's quaternion and the blocks of this lane's column
    const bool has = i > 0;
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    V3 bt = mk(0, 0, 0), bv = mk(0, 0, 0), bp = mk(0, 0, 0);   // the base row as stored: J_q | J_b H_b O_b | J_a H_a O_a
    if (A.N > 0 && has) {                            // N == 0 or i == 0: rows is not read
        const long long row = w * (long long)A.N + (i - 1);
        bq = ldq4(A.rows.q + row * 4);
        const long long o = row * 9 + c * 3;
        const double *pv = (d == 0) ? A.rows.J_b : ((d == 1) ? A.rows.H_b : A.rows.O_b);
        const double *pp = (d == 0) ? A.rows.J_a : ((d == 1) ? A.rows.H_a : A.rows.O_a);
        bv = ldv3(pv + o);
        bp = ldv3(pp + o);
        if (d == 0) bt = ldv3(A.rows.J_q + o);
    }
    if (live && has) {                               // i == 0: the cov_init state stands
        const V3 th = -bt;                           // J_q = -theta; the b_a / theta_klin columns have no theta block
        Ln.P0[0] = th.x; Ln.P0[1] = th.y; Ln.P0[2] = th.z;
        Ln.P0[6] = bv.x; Ln.P0[7] = bv.y; Ln.P0[8] = bv.z;
        Ln.P0[12] = bp.x; Ln.P0[13] = bp.y; Ln.P0[14] = bp.z;
        Ln.P0[15] = th.x; Ln.P0[16] = th.y; Ln.P0[17] = th.z;
    }

    const int hoff = cov_h_offset<MODEL>(jj);
    double *ir = irs + g * IRD;
    double *r0 = r0s + g * R0;

    // ---- the record of the partial interval [t_i, t_q] with reading i held; no step: dt = 0 (and the result is not used)
    const bool step = (i < n) && (tq > kt[0]);
    if (j == 0) {
        const M3 R_old = quat_2_Rot(bq);             // [0 0 0 1] gives the identity exactly
        const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
        const V3 gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));
        const V3 wi = mk(kt[1], kt[2], kt[3]), ai = mk(kt[4], kt[5], kt[6]);
        const SampleRec r = make_sample_rec<MODEL, AVG>(kt[0], step ? tq : kt[0], wi, ai, wi, ai, bw, ba);
        finish_interval<MODEL, AVG>(r, R_old, gk, ir);
        rec_put_mat(r0, 0, R_old);
    }
    wave_lds_fence();

    // ---- one interval of cov_body's phase C for a column whose Mt is the zero row: F x is lane-local, nothing is exchanged
    double zrow[EXCH_PITCH];
#pragma unroll
    for (int e = 0; e < EXCH_PITCH; e++) zrow[e] = 0.0;
    cov_begin<MODEL>(Ln, ir, hoff);
    M3 Rs = rec_mat(r0, 0);
#pragma unroll
    for (int stg = 0; stg < 4; ++stg) {
        double M[9];
        if (stg == 1 || stg == 3) Rs = cov_stage_rotation<MODEL>(ir, stg);   // stages 1 and 2 share R_mid
        cov_stage_M(Ln, stg, Rs, M);
        cov_stage_finish(Ln, stg, M, zrow);
    }

    // ---- the read-out of cov_body: the stepped column, or the base row bit for bit
    if (!valid || !live) return;
    const bool bad = (tq != tq) || sq_.none;
    const double x = __builtin_nan("");
    V3 ot = step ? -mk(Ln.P0[0], Ln.P0[1], Ln.P0[2]) : bt;
    V3 ov = step ? mk(Ln.P0[6], Ln.P0[7], Ln.P0[8]) : bv;
    V3 op = step ? mk(Ln.P0[12], Ln.P0[13], Ln.P0[14]) : bp;
    if (bad) { ot = mk(x, x, x); ov = ot; op = ot; }
    const long long o = k * 9 + c * 3;
    if (d == 0) {
        if (A.out.J_q) stv3(A.out.J_q + o, ot);
        if (A.out.J_a) stv3(A.out.J_a + o, op);
        if (A.out.J_b) stv3(A.out.J_b + o, ov);
    } else if (d == 1) {
        if (A.out.H_a) stv3(A.out.H_a + o, op);
        if (A.out.H_b) stv3(A.out.H_b + o, ov);
    } else {
        if (A.out.O_a) stv3(A.out.O_a + o, op);
        if (A.out.O_b) stv3(A.out.O_b + o, ov);
    }
}

}  // namespace
#endif   // __HIPCC__
