// cpi_query_cov_kernels.hpp -- the covariance at arbitrary times inside a window (cpi_query_cov_batch): cpi_query_cov_kernel.
// Part of the translation unit cpi_query_cov.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

// sigma^2 of the four diagonal blocks of Q_c (PreArgs::q4).  A kernel argument of its own, so that QueryArgs -- and with it
// cpi_query_kernel -- stays as it was.
struct QueryCovNoise { double q4[4]; };

#ifndef CPI_QUERY_COV_WPS
#define CPI_QUERY_COV_WPS 2   // wavefronts per SIMD the register allocation must leave room for (the build report shows what it got)
#endif

// Query k asks for the covariance of window w = qwin[k] at time t_q = qtime[k].  The rows of cpi_preintegrate_running hold P
// after every interval, so a query is the covariance recursion of cov_body (cpi_cov_kernels.hpp) run for exactly ONE partial
// interval from a gathered row.  One lane group per query (CovDims<MODEL>::GROUP lanes, cov_col_of_lane: a lane owns a column):
//   search   as cpi_query_kernel: i = the largest knot index in [0, n] with t_i <= t_q, by bisection with clamped probes; every lane
//            of a group runs it (the loads are broadcasts), so no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
//   gather   column jj of S = row w N + i - 1 of rows.P (15 contiguous doubles), or, when only rows.P_sym is given, its entries
//            (min(r, jj), max(r, jj)); i == 0: zeros.  Model 2 carries 18 rows and columns; at a row boundary the reference has just
//            cloned and marginalised (Pbig = Bk Pbig Bk^T, CpiV2.h:436-443; cov_end + the column clone in cov_body), so rows 15..17 of
//            every column are its rows 0..2 and columns 15..17 are columns 0..2: the clone lanes load the theta columns.  The nine
//            Discrete_J_b transition columns never feed P: their lanes idle as zero columns (index NCOL);
//   step     lane 0 of the group builds the interval record of [t_i, t_q] with reading i held (make_sample_rec / finish_interval,
//            the rotation at its start = quat_2_Rot of the row's q as in cpi_query_kernel) into LDS; then the four RK4 stages of
//            cov_body through the same exchange rows.  A query without a step (t_q on a stamp, before t_0, at or past t_n, NaN)
//            runs the stages with dt = 0 and its lanes SELECT the gathered column, so the copy is bit for bit the row;
//   store    columns jj < 15, rows 0..14, as cov_body stores them (cov_end and the column clone after the interval would only refresh
//            rows / columns 15..17, which no output reads: they are left out).
// LDS per wavefront: one record per group + the exchange rows = 8.0 KB (model 1), 4.8 KB (model 2).
template <int MODEL, bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_COV_WPS) void cpi_query_cov_kernel(QueryArgs A, QueryCovNoise NZ) {
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
    const long long w = min(max((long long)A.qwin[k], 0ll), A.W - 1);
    const double tq = A.qtime[k];
    const int n = A.count ? min(max(A.count[w], 0), A.N) : A.N;
    const double *kn = A.knots + (A.first ? A.first[w] : w * (long long)(A.N + 1)) * 7;

    // ---- the interval (cpi_query_kernel): sum of the steps = 2^trips - 1 >= N, every probe clamped into [0, n]
    int i = 0;
    for (int s = A.trips - 1; s >= 0; --s) {
        const int probe = i + (1 << s);
        const double t = kn[min(probe, n) * 7];
        i = (probe <= n && t <= tq) ? probe : i;
    }

    const double q4[4] = { NZ.q4[0], NZ.q4[1], NZ.q4[2], NZ.q4[3] };
    const int jl = cov_col_of_lane<MODEL>(j);
    const int jj = (jl < D::NPCOL) ? jl : D::NCOL;                  // column owned by this lane; NCOL = idle
    const int cs = (MODEL == 2 && jj >= 15 && jj < D::NPCOL) ? jj - 15 : jj;   // the column of the 15 x 15 row it starts from
    CovLane<MODEL> Ln;
    cov_init(Ln, jj, q4);

    // ---- knot i, the base row's quaternion and this lane's column of S, in flight together
    double kt[7];
#pragma unroll
    for (int c = 0; c < 7; c++) kt[c] = kn[i * 7 + c];
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
    const bool bad = tq != tq;
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

}  // namespace
