// hostsim_carry.cpp -- HOST emulation of the carry path of cpi_preintegrate_resume (cpi_mean_carry_kernel /
// cpi_cov_carry_kernel), built on cpi_math.hpp the way hostsim.cpp is.  TEST INFRASTRUCTURE ONLY.
//
// One window segment per call: the recursion starts from a carry record (or the zero state) and writes the record it ends
// in, in the device layout of cpi_args.hpp (namespace carry; the offsets are restated below).  The mean emulation
// follows the kernel's lane split: lane 0 -- the earliest segment -- starts from the carried state and the ordered tree
// composes the lanes; for model 2 mean-only with several lanes (GSEG) lane 0 integrates in the window-start frame with its
// gravity response starting at zero.  The covariance emulation is the column-lane recursion of hostsim.cpp with the
// rotation / means (gs) and every lane's column P0 taken from the record.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <algorithm>
#include <vector>
using namespace cpi;

namespace {
// cpi_args.hpp, namespace carry
const int C_TAG = 0, C_DT = 1, C_ALPHA = 2, C_BETA = 5, C_R = 8, C_JAC = 17;
int c_cov_off(int model) { return C_JAC + (model == 2 ? 63 : 45); }
int c_doubles(int model) { return model == 1 ? 288 : c_cov_off(2) + 27 * 18; }

const int OUTD = 308;  // DT1 alpha3 beta3 q4 R9 Jq9 Ja9 Jb9 Ha9 Hb9 Oa9 Ob9 P225 (oracle_py.OUT_FIELDS)
V3 ld3(const double *p) { return mk(p[0], p[1], p[2]); }
M3 ld_cm(const double *p) { M3 A; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A.m[i][j] = p[j * 3 + i]; return A; }
void put_cm(double *dst, const M3 &A) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) dst[j * 3 + i] = A.m[i][j]; }
void put_means(double *o, double DT, V3 alpha, V3 beta, const M3 &R) {
    o[0] = DT;
    o[1] = alpha.x; o[2] = alpha.y; o[3] = alpha.z;
    o[4] = beta.x; o[5] = beta.y; o[6] = beta.z;
    const Q4 q = rot_2_quat(R);
    o[7] = q.x; o[8] = q.y; o[9] = q.z; o[10] = q.w;
    put_cm(o + 11, R);
}

template <int MODEL, bool JAC>
void load_mean(MeanState<JAC> &s, const double *c) {
    s.DT = c[C_DT]; s.alpha = ld3(c + C_ALPHA); s.beta = ld3(c + C_BETA); s.R = ld_cm(c + C_R);
    if (JAC) {
        s.Jq = ld_cm(c + C_JAC); s.Ja = ld_cm(c + C_JAC + 9); s.Jb = ld_cm(c + C_JAC + 18);
        s.Ha = ld_cm(c + C_JAC + 27); s.Hb = ld_cm(c + C_JAC + 36);
        if (MODEL == 2) { s.Oa = ld_cm(c + C_JAC + 45); s.Ob = ld_cm(c + C_JAC + 54); }
    }
}
template <int MODEL, bool JAC>
void store_mean(double *c, const MeanState<JAC> &s) {
    c[C_TAG] = 1.0;
    c[C_DT] = s.DT;
    c[C_ALPHA] = s.alpha.x; c[C_ALPHA + 1] = s.alpha.y; c[C_ALPHA + 2] = s.alpha.z;
    c[C_BETA] = s.beta.x; c[C_BETA + 1] = s.beta.y; c[C_BETA + 2] = s.beta.z;
    put_cm(c + C_R, s.R);
    if (JAC) {
        put_cm(c + C_JAC, s.Jq); put_cm(c + C_JAC + 9, s.Ja); put_cm(c + C_JAC + 18, s.Jb);
        put_cm(c + C_JAC + 27, s.Ha); put_cm(c + C_JAC + 36, s.Hb);
        if (MODEL == 2) { put_cm(c + C_JAC + 45, s.Oa); put_cm(c + C_JAC + 54, s.Ob); }
    }
}

template <int MODEL, bool JAC, bool AVG>
void mean_seg(int L, int n, const double *kn, const double *lin, const double *qk, const double *grav, const double *cin,
              double *cout, double *o) {
    const V3 bw = ld3(lin), ba = ld3(lin + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq(qk)), ld3(grav));
    const int per = (n + L - 1) / L;
    constexpr bool GSEGABLE = (MODEL == 2) && !JAC;
    const bool gseg = GSEGABLE && L > 1;
    std::vector<MeanState<JAC>> seg(L);
    std::vector<GravAcc> ga(L);
    for (int l = 0; l < L; l++) {
        mean_init(seg[l]); grav_init(ga[l]);
        if (l == 0 && cin) load_mean<MODEL, JAC>(seg[0], cin);
        const int s0 = std::min(n, l * per), s1 = std::min(n, s0 + per);
        for (int s = s0; s < s1; s++) {
            const double *k0 = kn + 7 * s, *k1 = kn + 7 * (s + 1);
            if constexpr (GSEGABLE) {
                if (gseg) {
                    mean_step_v2seg<AVG>(seg[l], ga[l], k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba);
                    continue;
                }
            }
            mean_step<MODEL, JAC, AVG>(seg[l], k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba, gk);
        }
    }
    for (int st = 1; st < L; st *= 2)
        for (int l = 0; l + st < L; l += 2 * st) {
            if constexpr (GSEGABLE) { if (gseg) grav_combine(ga[l], seg[l], ga[l + st], seg[l + st]); }
            mean_combine(seg[l], seg[l + st]);
        }
    if constexpr (GSEGABLE) { if (gseg) grav_apply(seg[0], ga[0], gk); }
    const MeanState<JAC> &s = seg[0];
    put_means(o, s.DT, s.alpha, s.beta, s.R);
    if (JAC) {
        put_cm(o + 20, s.Jq); put_cm(o + 29, s.Ja); put_cm(o + 38, s.Jb); put_cm(o + 47, s.Ha); put_cm(o + 56, s.Hb);
        if (MODEL == 2) { put_cm(o + 65, s.Oa); put_cm(o + 74, s.Ob); }
    }
    store_mean<MODEL, JAC>(cout, s);
}

template <int MODEL, bool AVG>
void cov_seg(int n, const double *kn, const double *lin, const double *qk, const double *sig, const double *grav,
             const double *cin, double *cout, double *o) {
    typedef CovDims<MODEL> D;
    const int CO = c_cov_off(MODEL);
    const V3 bw = ld3(lin), ba = ld3(lin + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq(qk)), ld3(grav));
    const double q4[4] = { sig[0] * sig[0], sig[1] * sig[1], sig[2] * sig[2], sig[3] * sig[3] };
    const int NL = D::GROUP, CH = D::GROUP;
    std::vector<CovLane<MODEL>> lane(NL);
    const int IRD = IrPitch<MODEL>::V;
    std::vector<double> exch(exch_doubles(1), 0.0), irs(CH * IRD, 0.0);
    double gs[GS_DOUBLES];
    cov_gs_init(gs);
    if (cin) {
        rec_put_mat(gs, GS_R, ld_cm(cin + C_R));
        put3(gs + GS_ALPHA, ld3(cin + C_ALPHA));
        put3(gs + GS_BETA, ld3(cin + C_BETA));
        gs[GS_DT] = cin[C_DT];
    }
    std::vector<int> colof(NL);
    for (int j = 0; j < NL; j++) {
        colof[j] = cov_col_of_lane<MODEL>(j);
        cov_init(lane[j], colof[j], q4);
        cov_exch_init<MODEL>(exch.data(), 1, colof[j], q4);
        if (cin && colof[j] < D::NCOL)
            for (int i = 0; i < D::NR; i++) lane[j].P0[i] = cin[CO + colof[j] * D::NR + i];
    }
    for (int base = 0; base < n; base += CH) {
        std::vector<SampleRec> r(CH);
        std::vector<M3> inc(CH);
        for (int sl = 0; sl < CH; sl++) {
            const int s = base + sl;
            if (s < n) {
                const double *k0 = kn + 7 * s, *k1 = kn + 7 * (s + 1);
                r[sl] = make_sample_rec<MODEL, AVG>(k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba);
            } else {
                r[sl].dt = 0; r[sl].w = mk(0, 0, 0); r[sl].a0 = mk(0, 0, 0); r[sl].a1 = mk(0, 0, 0);
                r[sl].f1 = r[sl].f2 = r[sl].f3 = r[sl].f4 = 0; r[sl].Rstep = eye(); r[sl].Rhalf = eye();
            }
            inc[sl] = r[sl].Rstep;
        }
        for (int d = 1; d < CH; d <<= 1) {
            std::vector<M3> prev = inc;
            for (int sl = d; sl < CH; sl++) inc[sl] = mm(prev[sl], prev[sl - d]);
        }
        const M3 Rc = rec_mat(gs, GS_R);
        std::vector<MeanInc> mi(CH);
        for (int sl = 0; sl < CH; sl++) {
            const M3 pre = (sl == 0) ? eye() : inc[sl - 1];
            mi[sl] = finish_interval<MODEL, AVG>(r[sl], mm(pre, Rc), gk, irs.data() + sl * IRD);
        }
        for (int d = 1; d < CH; d <<= 1)
            for (int sl = 0; sl + d < CH; sl += 2 * d) mi[sl] = inc_combine(mi[sl], mi[sl + d]);
        gs_apply_inc(gs, mi[0]);
        rec_put_mat(gs, GS_R, mm(inc[CH - 1], Rc));
        const int cnt = std::min(CH, n - base);
        M3 Rs = Rc;
        for (int sl = 0; sl < cnt; sl++) {
            const double *ir = irs.data() + sl * IRD;
            for (int j = 0; j < NL; j++) cov_begin<MODEL>(lane[j], ir, cov_h_offset<MODEL>(colof[j]));
            for (int st = 0; st < 4; st++) {
                double M[32][9];
                for (int j = 0; j < NL; j++) {
                    cov_stage_M(lane[j], st, (st == 0) ? Rs : cov_stage_rotation<MODEL>(ir, st), M[j]);
                    if (colof[j] < D::NPCOL)
                        for (int rr = 0; rr < CovExchRows<MODEL>::V; rr++) exch[rr * EXCH_PITCH + exch_pos<MODEL>(colof[j])] = M[j][rr];
                }
                if (CovPBySymmetry<MODEL>::V) {
                    double mt[32][D::NR];
                    for (int j = 0; j < NL; j++) {
                        const double *row = exch.data() + cov_row_off<MODEL>(1, 0, colof[j]);
                        for (int i = 0; i < D::NR; i++) mt[j][i] = row[exch_pos<MODEL>(i)];
                    }
                    for (int j = CovPLanes<MODEL>::FIRST; j < CovPLanes<MODEL>::FIRST + 4 && j < NL; j++)
                        for (int i = 0; i < D::NR; i++) mt[j][i] = cov_stage_X(lane[j - CovPLanes<MODEL>::SHIFT], st)[i];
                    for (int j = 0; j < NL; j++) cov_stage_finish_regs(lane[j], st, M[j], mt[j]);
                } else {
                    for (int j = 0; j < NL; j++)
                        cov_stage_finish(lane[j], st, M[j], exch.data() + cov_row_off<MODEL>(1, 0, colof[j]));
                }
            }
            Rs = cov_stage_rotation<MODEL>(ir, 3);
            for (int j = 0; j < NL; j++) cov_end(lane[j]);
            if (MODEL == 2)
                for (int b = 0; b < 4; b++) for (int i = 0; i < D::NR; i++) lane[4 + b].P0[i] = lane[b].P0[i];
        }
    }
    const M3 Rfin = rec_mat(gs, GS_R);
    put_means(o, gs[GS_DT], rec_v3(gs, GS_ALPHA), rec_v3(gs, GS_BETA), Rfin);
    std::vector<int> laneof(D::NCOL + 1, 0);
    for (int j = 0; j < NL; j++) if (colof[j] < D::NCOL) laneof[colof[j]] = j;
    for (int c = 0; c < 15; c++) for (int i = 0; i < 15; i++) o[83 + c * 15 + i] = lane[laneof[c]].P0[i];
    if (MODEL == 2) {
        for (int c = 0; c < 3; c++) {
            const CovLane<MODEL> &g = lane[laneof[D::NPCOL + c]], &a = lane[laneof[D::NPCOL + 3 + c]], &l = lane[laneof[D::NPCOL + 6 + c]];
            for (int i = 0; i < 3; i++) {
                o[20 + c * 3 + i] = -g.P0[0 + i];
                o[29 + c * 3 + i] = g.P0[12 + i];
                o[38 + c * 3 + i] = g.P0[6 + i];
                o[47 + c * 3 + i] = a.P0[12 + i];
                o[56 + c * 3 + i] = a.P0[6 + i];
                o[65 + c * 3 + i] = l.P0[12 + i];
                o[74 + c * 3 + i] = l.P0[6 + i];
            }
        }
    }
    // the record the covariance kernel leaves: means (gs) and every lane's column
    cout[C_TAG] = 1.0;
    cout[C_DT] = gs[GS_DT];
    put3(cout + C_ALPHA, rec_v3(gs, GS_ALPHA));
    put3(cout + C_BETA, rec_v3(gs, GS_BETA));
    put_cm(cout + C_R, Rfin);
    for (int j = 0; j < NL; j++)
        if (colof[j] < D::NCOL)
            for (int i = 0; i < D::NR; i++) cout[CO + colof[j] * D::NR + i] = lane[j].P0[i];
}
}  // namespace

extern "C" int hsc_carry_doubles(int model) { return c_doubles(model); }
// One segment of n intervals (knots kn[n + 1][7]) of ONE window; cin = NULL: the zero state.  out[308] as hs_mean / hs_cov.
extern "C" void hsc_mean(int model, int jac, int avg, int L, int n, const double *kn, const double *lin, const double *qk,
                         const double *grav, const double *cin, double *cout, double *out) {
#define GO(M, J, A) mean_seg<M, J, A>(L, n, kn, lin, qk, grav, cin, cout, out)
    if (model == 1) { if (jac) { if (avg) GO(1, true, true); else GO(1, true, false); } else { if (avg) GO(1, false, true); else GO(1, false, false); } }
    else            { if (jac) { if (avg) GO(2, true, true); else GO(2, true, false); } else { if (avg) GO(2, false, true); else GO(2, false, false); } }
#undef GO
}
extern "C" void hsc_cov(int model, int avg, int n, const double *kn, const double *lin, const double *qk, const double *sig,
                        const double *grav, const double *cin, double *cout, double *out) {
    if (model == 1) { if (avg) cov_seg<1, true>(n, kn, lin, qk, sig, grav, cin, cout, out); else cov_seg<1, false>(n, kn, lin, qk, sig, grav, cin, cout, out); }
    else            { if (avg) cov_seg<2, true>(n, kn, lin, qk, sig, grav, cin, cout, out); else cov_seg<2, false>(n, kn, lin, qk, sig, grav, cin, cout, out); }
}
