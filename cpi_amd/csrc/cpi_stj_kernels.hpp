// cpi_stj_kernels.hpp -- model 2's bias Jacobians at arbitrary times inside a window (cpi_query_stj_batch): query_stj_body and, over
// it, cpi_query_stj_kernel.  The open form (cpi_query_open_kernels.hpp) and the stream form (cpi_query_stream_kernels.hpp) call the
// same body.  Part of a kernel translation unit (included after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once
#include "cpi_query_locate.hpp"

namespace {

#ifndef CPI_QUERY_STJ_WPS
#define CPI_QUERY_STJ_WPS 2   // wavefronts per SIMD the register allocation must leave room for (the build report shows what it got)
#endif

// Query k asks for J_q ... O_b of window w at time t_q = qtime[k].  The rows of cpi_running_stj_batch hold the
// read-out of the nine Discrete_J_b transition columns (b_w, b_a, theta_klin) after every interval, and at a row boundary that
// read-out determines the columns: cov_end has just set rows 15..17 to rows 0..2, the bias rows are the unit / zero blocks of
// cov_init (F has no bias rows), and the theta rows of the b_a and theta_klin columns are exactly zero ((F x)_theta = -w x x_theta
// - x_bw keeps a zero theta block zero when x_bw is zero).  So a query rebuilds the columns from row w N + i - 1 and advances them by
// the ONE partial interval [t_i, t_q] of cov_body's phase C (cpi_cov_kernels.hpp) with reading i held:
//   b_w column c        [-J_q[:,c] | e_c | J_b[:,c] | 0   | J_a[:,c] | -J_q[:,c]]
//   b_a column c        [ 0        | 0   | H_b[:,c] | e_c | H_a[:,c] |  0       ]
//   theta_klin column c [ 0        | 0   | O_b[:,c] | 0   | O_a[:,c] |  0       ]   (its unit entry enters through h, cov_h_offset)
// i == 0: the cov_init state.  A transition column has no transposed contribution (its Mt is the zero row), so nothing is exchanged
// between lanes: one group of 16 lanes per query, nine of them live, four queries per wavefront, and the only LDS is the interval
// record lane 0 of a group builds for it (make_sample_rec / finish_interval; the rotation at the start = quat_2_Rot of the row's q
// as in query_mean_body).
//   search   the locator's (cpi_query_locate.hpp), as in query_mean_body; every lane of a group runs it (the loads are
//            broadcasts), so no read leaves the knots [k0, k0 + n] or the rows [w N, w N + N);
//   step     the four RK4 stages of cov_body with the zero row as Mt.  A query without a step (t_q on a stamp, before t_0, at or
//            past t_n, NaN) stores what it loaded from the base row, bit for bit (zeros when i == 0);
//   store    the read-out of cov_body (J_q = -theta of the b_w columns, ...), 24 bytes per lane and field, for the fields of out
//            that are set.
// LDS per wavefront: 4 records of 42 doubles + 4 rotations = 1.6 KB.
template <bool AVG, bool OPEN, class Loc, class Args>
__device__ __forceinline__ void query_stj_body(const Args A, const QueryBase B) {
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
    const QueryAt at = Loc::find(A, k, tq);
    const long long w = at.w;
    const int n = at.n, i = at.i;
    const double *kt = at.kt;
    Loc::note_window(A, k, at, valid && j == 0);

    const bool live = j < D::NDCOL;
    const int jj = live ? D::NPCOL + j : D::NCOL;    // column owned by this lane; NCOL = idle (a zero column)
    const int d = min(j, D::NDCOL - 1) / 3, c = min(j, D::NDCOL - 1) % 3;   // idle lanes load what lane 8 loads and drop it
    const double q4[4] = { 0.0, 0.0, 0.0, 0.0 };     // process noise enters covariance columns only
    CovLane<MODEL> Ln;
    cov_init(Ln, jj, q4);

    // ---- the base row's quaternion and the blocks of this lane's column (knot i is in flight with them)
    const bool has = OPEN || i > 0;
    const bool fromb = OPEN && i == 0;               // the state before knot 0: the base row
    const cpi_outputs &R = A.rows, &RB = B.rows;
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    V3 bt = mk(0, 0, 0), bv = mk(0, 0, 0), bp = mk(0, 0, 0);   // the base row as stored: J_q | J_b H_b O_b | J_a H_a O_a
    if (OPEN || (A.N > 0 && has)) {                  // N == 0 or i == 0: rows is not read (OPEN: the base row is)
        const long long row = fromb ? w * (long long)B.N + (B.N - 1) : w * (long long)A.N + (i - 1);
        bq = ldq4((fromb ? RB.q : R.q) + row * 4);
        const long long o = row * 9 + c * 3;
        const double *pv = (d == 0) ? (fromb ? RB.J_b : R.J_b) : ((d == 1) ? (fromb ? RB.H_b : R.H_b) : (fromb ? RB.O_b : R.O_b));
        const double *pp = (d == 0) ? (fromb ? RB.J_a : R.J_a) : ((d == 1) ? (fromb ? RB.H_a : R.H_a) : (fromb ? RB.O_a : R.O_a));
        bv = ldv3(pv + o);
        bp = ldv3(pp + o);
        if (d == 0) bt = ldv3((fromb ? RB.J_q : R.J_q) + o);
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
    const bool bad = (tq != tq) || (OPEN && bq.x != bq.x) || at.none;
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

template <bool AVG>
__global__ __launch_bounds__(64, CPI_QUERY_STJ_WPS) void cpi_query_stj_kernel(QueryArgs A) {
    query_stj_body<AVG, false, WindowLocator>(A, QueryBase());
}

}  // namespace
