// cpi_merge_kernels.hpp -- consecutive preintegrated windows joined into one measurement (cpi_merge_batch): cpi_merge_kernel.
//
// Nothing here reads IMU data: the operands are MEASUREMENT rows (DT, alpha, beta, q, the five bias Jacobians, P) of windows
// [t0, t1], [t1, t2], ... that were preintegrated at ONE linearisation point, and the result is the measurement of [t0, tn].
// Model 1 only.  For A (earlier) followed by B (later), with R_X = quat_2_Rot(q_X), error-state order [theta b_g v b_a p]:
//   means                 mean_combine of cpi_math.hpp (R = R_B R_A, beta = beta_A + R_A^T beta_B, ...);
//   Jacobians             the Jacobian lines of mean_combine, one COLUMN per lane: jac_col_combine;
//   covariance            P = Phi~ P_A Phi~^T + T P_B T^T, then 0.5 (P + P^T), with T = blkdiag(I, I, R_A^T, I, R_A^T) and
//                         Phi~ = T Phi(B) T^T, Phi(B) the state transition over B rebuilt from B's PUBLIC fields:
//                           (theta,theta) R_B   (theta,b_g) -J_q   (v,theta) -[beta x]   (v,b_g) J_b   (v,b_a) H_b
//                           (p,theta) -[alpha x]   (p,b_g) J_a   (p,v) DT I   (p,b_a) H_a   and the unit diagonal.
//                         Phi~ keeps that sparsity ((v,v) and (p,p) stay I, (p,v) stays DT I; the v and p rows of the other
//                         blocks gain R_A^T from the left), so Phi~ x is five 3-vectors of a few 3x3 products: phi_apply.
// The first part of this header is CPI_HD arithmetic that tests/hostsim/hostsim_merge.cpp compiles for the host; the kernel
// itself follows under __HIPCC__.  Part of the translation unit cpi_merge.hip (included there after cpi_math.hpp /
// cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace cpi {
namespace merge {

// an operand row as it is staged: the nine small fields back to back (matrices column-major, as in cpi_outputs)
static const int OP_DT = 0, OP_ALPHA = 1, OP_BETA = 4, OP_Q = 7,
                 OP_JQ = 11, OP_JA = 20, OP_JB = 29, OP_HA = 38, OP_HB = 47, OP_DOUBLES = 56;
static const int LANES = 16;                    // lanes per output row: lane c < 15 owns column c of P
static const int STAGE_P = OP_DOUBLES;          // the operand's P (225 dense or 120 packed), later one exchange matrix
static const int STAGE_X = STAGE_P + 225;       // the other exchange matrix
static const int STAGE_DOUBLES = STAGE_X + 225; // per lane group, requests with the covariance

// rows [f, f + n) of group j: count clamped into [0, G], first into [0, in_rows], the group clipped at in_rows -- first and
// count live in device memory, so a wrong value gives a wrong row, never a read outside the input
CPI_HD void group_range(long long j, int G, long long in_rows, const long long *first, const int *count, long long &f, int &n) {
    f = first ? first[j] : j * (long long)G;
    n = count ? count[j] : G;
    n = (n < 0) ? 0 : ((n > G) ? G : n);
    f = (f < 0) ? 0 : ((f > in_rows) ? in_rows : f);
    if (in_rows - f < (long long)n) n = (int)(in_rows - f);
}

CPI_HD M3 m3_cm(const double *p) {   // column-major 3x3
    M3 A;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) A.m[i][j] = p[j * 3 + i];
    return A;
}
CPI_HD Q4 op_quat(const double *op) { Q4 q; q.x = op[OP_Q]; q.y = op[OP_Q + 1]; q.z = op[OP_Q + 2]; q.w = op[OP_Q + 3]; return q; }
// a staged operand as a composable state: the rotation is rebuilt from the row's quaternion
template <bool JAC>
CPI_HD void load_state(MeanState<JAC> &s, const double *op) {
    s.DT = op[OP_DT];
    s.alpha = mk(op[OP_ALPHA], op[OP_ALPHA + 1], op[OP_ALPHA + 2]);
    s.beta = mk(op[OP_BETA], op[OP_BETA + 1], op[OP_BETA + 2]);
    s.R = quat_2_Rot(op_quat(op));
    if (JAC) {
        s.Jq = m3_cm(op + OP_JQ); s.Ja = m3_cm(op + OP_JA); s.Jb = m3_cm(op + OP_JB);
        s.Ha = m3_cm(op + OP_HA); s.Hb = m3_cm(op + OP_HB);
        s.Oa = zero3(); s.Ob = zero3();
    }
}
// one column (or row) of a 15 x 15 matrix over [theta b_g v b_a p]
struct Col15 { V3 t, g, v, a, p; };
CPI_HD Col15 col_zero() { Col15 c; c.t = c.g = c.v = c.a = c.p = mk(0, 0, 0); return c; }
CPI_HD V3 ld3s(const double *p, int s) { return mk(p[0], p[s], p[2 * s]); }
CPI_HD void st3s(double *p, int s, V3 v) { p[0] = v.x; p[s] = v.y; p[2 * s] = v.z; }
// entries p[0], p[s], ..., p[14 s]: s = 1 walks a column of a column-major matrix, s = 15 a row
CPI_HD Col15 col_load(const double *p, int s) {
    Col15 c;
    c.t = ld3s(p, s); c.g = ld3s(p + 3 * s, s); c.v = ld3s(p + 6 * s, s); c.a = ld3s(p + 9 * s, s); c.p = ld3s(p + 12 * s, s);
    return c;
}
CPI_HD void col_store(double *p, int s, const Col15 &c) {
    st3s(p, s, c.t); st3s(p + 3 * s, s, c.g); st3s(p + 6 * s, s, c.v); st3s(p + 9 * s, s, c.a); st3s(p + 12 * s, s, c.p);
}
CPI_HD double tri_at(const double *t, int r, int c) { return (r <= c) ? t[CPI_TRI_INDEX(r, c)] : t[CPI_TRI_INDEX(c, r)]; }
// column c of the symmetric matrix whose packed upper triangle is t
CPI_HD Col15 col_load_tri(const double *t, int c) {
    Col15 x;
    x.t = mk(tri_at(t, 0, c), tri_at(t, 1, c), tri_at(t, 2, c));
    x.g = mk(tri_at(t, 3, c), tri_at(t, 4, c), tri_at(t, 5, c));
    x.v = mk(tri_at(t, 6, c), tri_at(t, 7, c), tri_at(t, 8, c));
    x.a = mk(tri_at(t, 9, c), tri_at(t, 10, c), tri_at(t, 11, c));
    x.p = mk(tri_at(t, 12, c), tri_at(t, 13, c), tri_at(t, 14, c));
    return x;
}
CPI_HD Col15 col_add(const Col15 &a, const Col15 &b) {
    Col15 c;
    c.t = a.t + b.t; c.g = a.g + b.g; c.v = a.v + b.v; c.a = a.a + b.a; c.p = a.p + b.p;
    return c;
}
// 0.5 (a + b): the symmetrisation, commutative to the bit, so entry (i, j) and entry (j, i) come out equal
CPI_HD Col15 col_mean(const Col15 &a, const Col15 &b) {
    Col15 c;
    c.t = 0.5 * (a.t + b.t); c.g = 0.5 * (a.g + b.g); c.v = 0.5 * (a.v + b.v); c.a = 0.5 * (a.a + b.a); c.p = 0.5 * (a.p + b.p);
    return c;
}
// y = Phi~ x = T Phi(B) T^T x, RA = R_A, op = the staged operand B: the block sparsity of the header comment, nothing dense, one
// block row per routine (the b_g and b_a rows are the identity).  B is consumed a matrix at a time: the fences keep the loads of
// the next matrix from being hoisted over the arithmetic of the one before, so a few doubles of B are live at once, not 56.
CPI_HD V3 phi_theta(const double *op, const Col15 &x) {
    V3 y = mul(quat_2_Rot(op_quat(op)), x.t);
    CPI_SCHED_FENCE();
    y = y - mul(m3_cm(op + OP_JQ), x.g);
    CPI_SCHED_FENCE();
    return y;
}
// the v row (o_j = OP_JB, o_h = OP_HB, o_m = OP_BETA) and the p row (OP_JA, OP_HA, OP_ALPHA) without their unit / DT blocks
CPI_HD V3 phi_vp(const M3 &RA, const double *op, const Col15 &x, int o_j, int o_h, int o_m) {
    V3 t = mul(m3_cm(op + o_j), x.g);
    CPI_SCHED_FENCE();
    t = (t + mul(m3_cm(op + o_h), x.a)) - cross(ld3s(op + o_m, 1), x.t);
    CPI_SCHED_FENCE();
    return mulT(RA, t);
}
CPI_HD V3 phi_v(const M3 &RA, const double *op, const Col15 &x) { return x.v + phi_vp(RA, op, x, OP_JB, OP_HB, OP_BETA); }
CPI_HD V3 phi_p(const M3 &RA, const double *op, const Col15 &x) { return x.p + (op[OP_DT] * x.v + phi_vp(RA, op, x, OP_JA, OP_HA, OP_ALPHA)); }
CPI_HD Col15 phi_apply(const M3 &RA, const double *op, const Col15 &x) {
    Col15 y;
    y.t = phi_theta(op, x);
    y.g = x.g;
    y.a = x.a;
    y.v = phi_v(RA, op, x);
    y.p = phi_p(RA, op, x);
    return y;
}
// y = T x
CPI_HD Col15 t_apply(const M3 &RA, const Col15 &x) {
    Col15 y;
    y.t = x.t; y.g = x.g; y.a = x.a;
    y.v = mulT(RA, x.v);
    y.p = mulT(RA, x.p);
    return y;
}
// The covariance of A o B, one column per lane, in the halves that exchanges separate.  With column c of P_A and of P_B:
//   left    u = Phi~ P_A[:, c],  v = T P_B[:, c]           -> written as column c of U and of V
//   right   row c of U and of V read back (= column c of U^T, V^T):  Phi~ U^T[:, c] + T V^T[:, c] = column c of
//           (Phi~ P_A Phi~^T + T P_B T^T)^T
//   and a third exchange symmetrises: col_mean(column c, row c).
// The five bias Jacobians, column by column.  Column i of (J_q, J_b, J_a) composes as
//   J_q' = R_B J_q + J_q^B,   J_b' = J_b + R_A^T (J_b^B + beta_B x J_q),   J_a' = J_a + DT_B J_b + R_A^T (J_a^B + alpha_B x J_q)
// and column i of (H_b, H_a) as the last two lines with a zero first member -- so ONE routine over a triple (x1, x2, x3) serves
// both: lanes 0..2 carry column l of (J_q, J_b, J_a), lanes 3..5 column l - 3 of (0, H_b, H_a).  The operations per entry are
// those of mean_combine<true>.
struct JacCol { V3 x1, x2, x3; };
CPI_HD JacCol jac_col_zero() { JacCol x; x.x1 = x.x2 = x.x3 = mk(0, 0, 0); return x; }
// where lane l's triple sits in a staged operand; o1 < 0: the zero member.  Lanes past 5 shadow lane 0.
CPI_HD void jac_col_offsets(int l, int &o1, int &o2, int &o3) {
    const bool h = (l >= 3 && l < 6);
    const int i = (l < 3) ? l : (h ? l - 3 : 0);
    o1 = h ? -1 : OP_JQ + 3 * i;
    o2 = (h ? OP_HB : OP_JB) + 3 * i;
    o3 = (h ? OP_HA : OP_JA) + 3 * i;
}
CPI_HD JacCol jac_col_load(const double *op, int o1, int o2, int o3) {
    JacCol x;
    x.x1 = (o1 >= 0) ? ld3s(op + o1, 1) : mk(0, 0, 0);
    x.x2 = ld3s(op + o2, 1);
    x.x3 = ld3s(op + o3, 1);
    return x;
}
// X = X o XB, with the means of A (its rotation RA) BEFORE mean_combine replaces them
CPI_HD void jac_col_combine(JacCol &X, const M3 &RA, const MeanState<false> &B, const JacCol &XB) {
    const V3 n2 = mulT(RA, XB.x2 + cross(B.beta, X.x1));
    const V3 n3 = mulT(RA, XB.x3 + cross(B.alpha, X.x1));
    X.x3 = (X.x3 + B.DT * X.x2) + n3;
    X.x2 = X.x2 + n2;
    X.x1 = mul(B.R, X.x1) + XB.x1;
}

}  // namespace merge
}  // namespace cpi

#if defined(__HIPCC__)
namespace {

using namespace cpi::merge;

// Wavefronts per SIMD the register allocation must leave room for (the build report shows what it got).  The requests with the
// covariance hold R_A, the Jacobian columns, a column of P, the block row of Phi~ in flight and the 19 to 24 prefetched doubles of
// the next operand: 266 to 296 registers, so they take the whole file of ONE wavefront rather than spill at two.
#ifndef CPI_MERGE_WPS
#define CPI_MERGE_WPS 2
#endif
#ifndef CPI_MERGE_COV_WPS
#define CPI_MERGE_COV_WPS 1
#endif

// One lane group (16 lanes, four per wavefront) per output row folds the rows [f, f + n) of its group in order.
//   fetch    the group's lanes fetch the next operand TOGETHER: lane l element l of each of the four mean fields (and of the five
//            Jacobian fields), and -- requests with the covariance only -- elements l + 16 s of P (225) or P_sym (120): every
//            load instruction of a group reads one contiguous burst.  The loads of operand k + 1 are issued before operand k is
//            folded in (registers), and written to the group's LDS stage at the top of the next trip.  A request without the covariance never touches P, a
//            request for the means alone reads the four mean fields alone.
//   state    registers: every lane of the group keeps the accumulated means (R, alpha, beta, DT; the same arithmetic on every
//            lane), lanes 0..5 one column of the accumulated Jacobians (jac_col_combine), lane c < 15 column c of the accumulated P.
//   fold     trip 0 takes the operand as it is; trip k > 0: the left half of the covariance, exchange, the right half, exchange,
//            symmetrise, then the Jacobian columns -- all with R_A BEFORE mean_combine replaces it.  The trip count is the largest n of the wavefront; a
//            group that is done (k >= n) skips the fold as a whole (the exchanges stay inside a lane group) and keeps its state.
//   store    n == 0: the zero state; n == 1: the operand's fields came through untouched, and q is the row's own (read again: no
//            requantisation); n > 1: q = rot_2_quat(R).  Lane 0 writes the means, lanes 0..5 their Jacobian columns, lane c column
//            c of P and / or its run of P_sym.
// LDS per wavefront: 4 x 506 doubles = 15.8 KB with the covariance, 4 x 56 doubles without.
template <bool JAC, bool COV>
__global__ __launch_bounds__(64, COV ? CPI_MERGE_COV_WPS : CPI_MERGE_WPS) void cpi_merge_kernel(MergeArgs A) {
    constexpr bool OPJ = JAC || COV;                       // the operands' Jacobians are read
    constexpr int STAGE = COV ? STAGE_DOUBLES : OP_DOUBLES;
    __shared__ double lds[4 * STAGE];
    const int lane = threadIdx.x, g = lane >> 4, l = lane & (LANES - 1);
    const int c = (l < 15) ? l : 14;                       // lane 15 shadows lane 14 and stores nothing
    const long long j = (long long)blockIdx.x * 4 + g;
    double *st = lds + g * STAGE;
    long long f = 0;
    int n = 0;
    if (j < A.M) group_range(j, A.G, A.in_rows, A.first, A.count, f, n);
    const int nmax = wave_max(n);
    const bool tri = COV && A.in.P == nullptr;             // the operands' covariance arrives as P_sym

    const double *pin = tri ? A.in.P_sym : A.in.P;
    const int plen = tri ? CPI_TRI_DOUBLES : 225;
    int o1, o2, o3;
    jac_col_offsets(l, o1, o2, o3);

    // element l of every small field of the next operand (lane l < the field's row length), and elements l + 16 s of its P
    constexpr int NF = OPJ ? 9 : 4;
    double nop[NF], npp[15];
    auto issue = [&](int k) {
        const long long row = (k < n) ? f + k : 0;        // a group that is done re-reads row 0 (nmax > 0: it exists)
        nop[0] = (l < 1) ? A.in.DT[row] : 0.0;
        nop[1] = (l < 3) ? A.in.alpha[row * 3 + l] : 0.0;
        nop[2] = (l < 3) ? A.in.beta[row * 3 + l] : 0.0;
        nop[3] = (l < 4) ? A.in.q[row * 4 + l] : 0.0;
        if (OPJ) {
            nop[4] = (l < 9) ? A.in.J_q[row * 9 + l] : 0.0;
            nop[5] = (l < 9) ? A.in.J_a[row * 9 + l] : 0.0;
            nop[6] = (l < 9) ? A.in.J_b[row * 9 + l] : 0.0;
            nop[7] = (l < 9) ? A.in.H_a[row * 9 + l] : 0.0;
            nop[8] = (l < 9) ? A.in.H_b[row * 9 + l] : 0.0;
        }
        if (COV) {
#pragma unroll
            for (int s = 0; s < 15; s++) {
                const int idx = l + LANES * s;
                npp[s] = (idx < plen) ? pin[row * plen + idx] : 0.0;
            }
        }
    };
    auto stage = [&]() {
        if (l < 1) st[OP_DT] = nop[0];
        if (l < 3) { st[OP_ALPHA + l] = nop[1]; st[OP_BETA + l] = nop[2]; }
        if (l < 4) st[OP_Q + l] = nop[3];
        if (OPJ && l < 9) { st[OP_JQ + l] = nop[4]; st[OP_JA + l] = nop[5]; st[OP_JB + l] = nop[6]; st[OP_HA + l] = nop[7]; st[OP_HB + l] = nop[8]; }
        if (COV) {
#pragma unroll
            for (int s = 0; s < 15; s++) {
                const int idx = l + LANES * s;
                if (idx < plen) st[STAGE_P + idx] = npp[s];
            }
        }
    };

    MeanState<false> S;
    mean_init(S);
    JacCol X = jac_col_zero();
    Col15 pa = col_zero();
    if (nmax > 0) issue(0);
    for (int k = 0; k < nmax; k++) {
        stage();
        wave_lds_fence();
        if (k + 1 < nmax) issue(k + 1);
        const bool act = k < n;
        Col15 pb = col_zero();
        if (COV) pb = tri ? col_load_tri(st + STAGE_P, c) : col_load(st + STAGE_P + c * 15, 1);
        wave_lds_fence();                                  // the operand's P is in registers: its area is free for the exchange
        if (k == 0) {
            if (act) {
                load_state(S, st);
                if (JAC) X = jac_col_load(st, o1, o2, o3);
                pa = pb;
            }
        } else if (act) {                                  // a whole lane group takes the branch or none of it does
            if constexpr (COV) {
                if (l < 15) col_store(st + STAGE_P + c * 15, 1, t_apply(S.R, pb));
                {   // u = Phi~ pa, stored block row by block row
                    double *ux = st + STAGE_X + c * 15;
                    const V3 ut = phi_theta(st, pa);
                    if (l < 15) { st3s(ux, 1, ut); st3s(ux + 3, 1, pa.g); st3s(ux + 9, 1, pa.a); }
                    const V3 uv = phi_v(S.R, st, pa);
                    if (l < 15) st3s(ux + 6, 1, uv);
                    const V3 up = phi_p(S.R, st, pa);
                    if (l < 15) st3s(ux + 12, 1, up);
                }
                wave_lds_fence();
                Col15 pn = phi_apply(S.R, st, col_load(st + STAGE_X + c, 15));
                CPI_SCHED_FENCE();
                pn = col_add(pn, t_apply(S.R, col_load(st + STAGE_P + c, 15)));
                wave_lds_fence();
                if (l < 15) col_store(st + STAGE_X + c * 15, 1, pn);
                wave_lds_fence();
                pa = col_mean(pn, col_load(st + STAGE_X + c, 15));
            }
            MeanState<false> B;
            load_state(B, st);
            if (JAC) jac_col_combine(X, S.R, B, jac_col_load(st, o1, o2, o3));
            mean_combine(S, B);
        }
        wave_lds_fence();                                  // the stage is read: the next trip may write over it
    }
    if (j >= A.M) return;

    const cpi_outputs &o = A.out;
    if (l == 0) {
        Q4 q; q.x = 0; q.y = 0; q.z = 0; q.w = 1;
        if (n == 1) q = ldq4(A.in.q + f * 4);              // the row's own quaternion, not rot_2_quat(quat_2_Rot(q))
        else if (n > 1) q = rot_2_quat(S.R);
        if (o.DT) o.DT[j] = S.DT;
        if (o.alpha) stv3(o.alpha + j * 3, S.alpha);
        if (o.beta) stv3(o.beta + j * 3, S.beta);
        if (o.q) { double *p = o.q + j * 4; p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }
    }
    if constexpr (JAC) {
        if (l < 3) {
            if (o.J_q) stv3(o.J_q + j * 9 + 3 * l, X.x1);
            if (o.J_b) stv3(o.J_b + j * 9 + 3 * l, X.x2);
            if (o.J_a) stv3(o.J_a + j * 9 + 3 * l, X.x3);
        } else if (l < 6) {
            if (o.H_b) stv3(o.H_b + j * 9 + 3 * (l - 3), X.x2);
            if (o.H_a) stv3(o.H_a + j * 9 + 3 * (l - 3), X.x3);
        }
    }
    if constexpr (COV) {
        if (l < 15) {
            if (o.P) col_store(o.P + j * 225 + c * 15, 1, pa);
            if (o.P_sym) {
                // entries (i, c), i <= c: the run [c (c + 1) / 2, c (c + 1) / 2 + c] of the packed triangle
                double col[15];
                col_store(col, 1, pa);
                double *p = o.P_sym + j * CPI_TRI_DOUBLES + c * (c + 1) / 2;
#pragma unroll
                for (int i = 0; i < 15; i++)
                    if (i <= c) p[i] = col[i];
            }
        }
    }
}

}  // namespace
#endif
