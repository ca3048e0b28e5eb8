// hostsim_stj.cpp -- HOST emulation of model 2's running / query-time bias Jacobians (cpi_cov_running_stj_kernel,
// cpi_query_stj_kernel), built on cpi_math.hpp the way hostsim_running.cpp is.  TEST INFRASTRUCTURE ONLY.
//
// The nine Discrete_J_b transition columns of cov_body read no other column (their transposed contribution Mt is the zero row of
// the exchange buffer), so the emulation carries those nine lanes alone: hss_rows runs them over all N intervals (those past the
// count staged as no-ops) with the Jacobian read-out after every cov_end; hss_query REBUILDS the nine columns from one such row
// (or takes the cov_init state), advances them by one partial interval with the reading held, and reads them out -- the
// reconstruction cpi_query_stj_kernel relies on.  Rows have the layout of hs_mean / hs_cov (308 doubles; q at 7, J_q at 20 ...
// O_b at 74, column-major).
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <algorithm>
using namespace cpi;

namespace {
const int OUTD = 308, OFF_Q = 7, OFF_JQ = 20, OFF_JA = 29, OFF_JB = 38, OFF_HA = 47, OFF_HB = 56, OFF_OA = 65, OFF_OB = 74;
typedef CovDims<2> D;
V3 ld3(const double *p) { return mk(p[0], p[1], p[2]); }
Q4 ldq(const double *p) { Q4 q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3]; return q; }
void st3(double *p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// the read-out of Discrete_J_b at the end of cov_body (CpiV2.h:450-458), lane j = transition column NPCOL + j
void read_out(const CovLane<2> *lane, double *o) {
    for (int j = 0; j < D::NDCOL; j++) {
        const int d = j / 3, c = j % 3;
        const double *P0 = lane[j].P0;
        const V3 th = mk(P0[0], P0[1], P0[2]), vv = mk(P0[6], P0[7], P0[8]), pp = mk(P0[12], P0[13], P0[14]);
        if (d == 0) { st3(o + OFF_JQ + c * 3, -th); st3(o + OFF_JA + c * 3, pp); st3(o + OFF_JB + c * 3, vv); }
        else if (d == 1) { st3(o + OFF_HA + c * 3, pp); st3(o + OFF_HB + c * 3, vv); }
        else { st3(o + OFF_OA + c * 3, pp); st3(o + OFF_OB + c * 3, vv); }
    }
}
// one interval of phase C for the nine lanes: Mt = the zero row
void step(CovLane<2> *lane, const double *ir, const M3 &R_old) {
    const double zrow[EXCH_PITCH] = { 0 };
    for (int j = 0; j < D::NDCOL; j++) {
        cov_begin<2>(lane[j], ir, cov_h_offset<2>(D::NPCOL + j));
        for (int stg = 0; stg < 4; stg++) {
            double M[9];
            cov_stage_M(lane[j], stg, (stg == 0) ? R_old : cov_stage_rotation<2>(ir, stg), M);
            cov_stage_finish(lane[j], stg, M, zrow);
        }
        cov_end(lane[j]);
    }
}

template <bool AVG>
void rows_of(int N, int n, const double *kn, const double *lin, const double *qk, const double *grav, double *rows) {
    const V3 bw = ld3(lin), ba = ld3(lin + 3);
    const V3 gk = mul(quat_2_Rot(ldq(qk)), ld3(grav));
    const double q4[4] = { 0, 0, 0, 0 };
    n = std::min(std::max(n, 0), N);
    CovLane<2> lane[D::NDCOL];
    for (int j = 0; j < D::NDCOL; j++) cov_init(lane[j], D::NPCOL + j, q4);
    M3 R = eye();
    double ir[IrPitch<2>::V];
    for (int s = 0; s < N; s++) {
        SampleRec r;
        if (s < n) {
            const double *k0 = kn + 7 * s, *k1 = kn + 7 * (s + 1);
            r = make_sample_rec<2, AVG>(k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba);
        } else {
            r.dt = 0; r.w = mk(0, 0, 0); r.a0 = mk(0, 0, 0); r.a1 = mk(0, 0, 0);
            r.f1 = r.f2 = r.f3 = r.f4 = 0; r.Rstep = eye(); r.Rhalf = eye();
        }
        (void)finish_interval<2, AVG>(r, R, gk, ir);
        step(lane, ir, R);
        R = cov_stage_rotation<2>(ir, 3);
        double *o = rows + (size_t)s * OUTD;
        const Q4 q = rot_2_quat(R);
        o[OFF_Q] = q.x; o[OFF_Q + 1] = q.y; o[OFF_Q + 2] = q.z; o[OFF_Q + 3] = q.w;
        read_out(lane, o);
    }
}

template <bool AVG>
void query_of(const double *row, const double *knot, double tq, const double *lin, const double *qk, const double *grav, double *out) {
    const V3 bw = ld3(lin), ba = ld3(lin + 3);
    const V3 gk = mul(quat_2_Rot(ldq(qk)), ld3(grav));
    const double q4[4] = { 0, 0, 0, 0 };
    CovLane<2> lane[D::NDCOL];
    Q4 bq; bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    for (int j = 0; j < D::NDCOL; j++) {
        cov_init(lane[j], D::NPCOL + j, q4);   // the bias rows: unit / zero blocks
        if (!row) continue;
        const int d = j / 3, c = j % 3;
        const V3 th = (d == 0) ? -ld3(row + OFF_JQ + c * 3) : mk(0, 0, 0);
        const V3 vv = ld3(row + ((d == 0) ? OFF_JB : (d == 1) ? OFF_HB : OFF_OB) + c * 3);
        const V3 pp = ld3(row + ((d == 0) ? OFF_JA : (d == 1) ? OFF_HA : OFF_OA) + c * 3);
        double *P0 = lane[j].P0;
        st3(P0, th); st3(P0 + 6, vv); st3(P0 + 12, pp); st3(P0 + 15, th);
    }
    if (row) bq = ldq(row + OFF_Q);
    const M3 R_old = quat_2_Rot(bq);
    const V3 wi = ld3(knot + 1), ai = ld3(knot + 4);
    const SampleRec r = make_sample_rec<2, AVG>(knot[0], tq, wi, ai, wi, ai, bw, ba);
    double ir[IrPitch<2>::V];
    (void)finish_interval<2, AVG>(r, R_old, gk, ir);
    step(lane, ir, R_old);
    read_out(lane, out);
}
}  // namespace

// rows[N][308]: q and the seven Jacobian fields after every interval; kn: the window's n + 1 knots (n is clamped into [0, N])
extern "C" int hss_rows(int avg, int N, int n, const double *kn, const double *lin, const double *qk, const double *grav, double *rows) {
    if (avg) rows_of<true>(N, n, kn, lin, qk, grav, rows); else rows_of<false>(N, n, kn, lin, qk, grav, rows);
    return 0;
}
// out[308]: the seven Jacobian fields at tq, from row (the row behind knot i; NULL: i == 0) and knot i, reading i held over [t_i, tq]
extern "C" int hss_query(int avg, const double *row, const double *knot, double tq, const double *lin, const double *qk,
                         const double *grav, double *out) {
    if (avg) query_of<true>(row, knot, tq, lin, qk, grav, out); else query_of<false>(row, knot, tq, lin, qk, grav, out);
    return 0;
}
