// hostsim_running_resume.cpp -- HOST emulation of cpi_preintegrate_running_resume (cpi_mean_running_carry_kernel /
// cpi_cov_running_carry_kernel), built on cpi_math.hpp the way hostsim_running.cpp and hostsim_carry.cpp are.
// TEST INFRASTRUCTURE ONLY.
//
// One window segment per call: a row after every interval (rows[N][308], the layout of hs_mean / hs_cov), from a carry record
// (or the zero state) to the record the segment ends in (device layout: cpi_args.hpp, namespace carry, restated below).
// The mean emulation is hostsim_running.cpp's with the carried head of the kernel: lane 0 integrates from the record in pass 1,
// so the ordered scan hands every later lane `carried o everything before it`; a lane before which nothing was integrated
// (lane 0 always) takes the record itself instead of the scanned `carried o identity`; after the walk the record is stored
// from the WALKED state of the last lane that integrated anything -- the lane whose last row row N - 1 repeats -- or, when
// none did, from lane 0's untouched carried state.  The covariance emulation is the column-lane recursion of
// hostsim_running.cpp started from the record's rotation and columns, with the columns written back after the last interval.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <algorithm>
#include <cstring>
#include <vector>
using namespace cpi;

namespace {
// cpi_args.hpp, namespace carry
const int C_TAG = 0, C_DT = 1, C_ALPHA = 2, C_BETA = 5, C_R = 8, C_JAC = 17;
int c_cov_off(int model) { return C_JAC + (model == 2 ? 63 : 45); }
int c_doubles(int model) { return model == 1 ? 288 : c_cov_off(2) + 27 * 18; }

const int OUTD = 308;  // DT1 alpha3 beta3 q4 R9 Jq9 Ja9 Jb9 Ha9 Hb9 Oa9 Ob9 P225 (oracle_py.OUT_FIELDS)
V3 ld3(const double *p) { return mk(p[0], p[1], p[2]); }
Q4 ld4(const double *p) { Q4 q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3]; return q; }
M3 ld_cm(const double *p) { M3 A; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A.m[i][j] = p[j * 3 + i]; return A; }
void put_cm(double *dst, const M3 &A) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) dst[j * 3 + i] = A.m[i][j]; }

template <bool JAC>
void put_row(double *o, const MeanState<JAC> &s) {
    o[0] = s.DT;
    o[1] = s.alpha.x; o[2] = s.alpha.y; o[3] = s.alpha.z;
    o[4] = s.beta.x; o[5] = s.beta.y; o[6] = s.beta.z;
    const Q4 q = rot_2_quat(s.R);
    o[7] = q.x; o[8] = q.y; o[9] = q.z; o[10] = q.w;
    put_cm(o + 11, s.R);
    if (JAC) { put_cm(o + 20, s.Jq); put_cm(o + 29, s.Ja); put_cm(o + 38, s.Jb); put_cm(o + 47, s.Ha); put_cm(o + 56, s.Hb); }
}
template <bool JAC>
void load_mean(MeanState<JAC> &s, const double *c) {   // carry_load_mean (model 1's Jacobians only: model 2 has no running ones)
    s.DT = c[C_DT]; s.alpha = ld3(c + C_ALPHA); s.beta = ld3(c + C_BETA); s.R = ld_cm(c + C_R);
    if (JAC) {
        s.Jq = ld_cm(c + C_JAC); s.Ja = ld_cm(c + C_JAC + 9); s.Jb = ld_cm(c + C_JAC + 18);
        s.Ha = ld_cm(c + C_JAC + 27); s.Hb = ld_cm(c + C_JAC + 36);
    }
}
template <bool JAC>
void store_mean(double *c, const MeanState<JAC> &s) {  // carry_store_mean
    c[C_TAG] = 1.0;
    c[C_DT] = s.DT;
    c[C_ALPHA] = s.alpha.x; c[C_ALPHA + 1] = s.alpha.y; c[C_ALPHA + 2] = s.alpha.z;
    c[C_BETA] = s.beta.x; c[C_BETA + 1] = s.beta.y; c[C_BETA + 2] = s.beta.z;
    put_cm(c + C_R, s.R);
    if (JAC) {
        put_cm(c + C_JAC, s.Jq); put_cm(c + C_JAC + 9, s.Ja); put_cm(c + C_JAC + 18, s.Jb);
        put_cm(c + C_JAC + 27, s.Ha); put_cm(c + C_JAC + 36, s.Hb);
    }
}

template <int MODEL, bool JAC, bool AVG>
void mean_rows(int L, int N, int n, const double *kn, const double *lin, const double *qk, const double *grav, const double *cin,
               double *cout, double *rows) {
    const V3 bw = ld3(lin), ba = ld3(lin + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ld4(qk)), ld3(grav));
    n = std::min(std::max(n, 0), N);
    auto knot = [&](int i) { return kn + 7 * std::min(i, n); };
    const int per = (N + L - 1) / L;
    const bool multi = L > 1;
    constexpr bool GSEGABLE = (MODEL == 2) && !JAC;
    std::vector<MeanState<JAC>> st(L);
    std::vector<GravAcc> ga(L);
    std::vector<int> r0(L), nrows(L), lead(L, 0), src(L, -1);
    for (int l = 0; l < L; l++) {
        r0[l] = std::min(N, l * per);
        nrows[l] = std::min(N - r0[l], per);
        mean_init(st[l]); grav_init(ga[l]);
    }
    if (cin) load_mean<JAC>(st[0], cin);          // the carried head: pass 1 of lane 0 and (one lane) the walk start from it
    int owner = 0;
    if (multi) {
        for (int l = 0; l < L; l++) {   // pass 1
            bool seen = false;
            for (int t = 0; t < per; t++) {
                const double *k0 = knot(r0[l] + t), *k1 = knot(r0[l] + t + 1);
                const bool act = t < nrows[l];
                const bool moves = act && (k1[0] - k0[0] > 0);
                if (!seen && !moves && act) lead[l]++;
                seen = seen || moves;
                if constexpr (GSEGABLE)
                    mean_step_v2seg<AVG>(st[l], ga[l], k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba, act);
                else
                    mean_step<MODEL, JAC, AVG>(st[l], k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba, gk, act);
            }
        }
        for (int d = 1; d < L; d <<= 1) {   // ordered inclusive scan: lane l <- (l - d) o l
            const std::vector<MeanState<JAC>> ps = st;
            const std::vector<GravAcc> pg = ga;
            for (int l = d; l < L; l++) {
                MeanState<JAC> B = ps[l - d];
                GravAcc gB = pg[l - d];
                if constexpr (GSEGABLE) grav_combine(gB, B, pg[l], ps[l]);
                mean_combine(B, ps[l]);
                st[l] = B; ga[l] = gB;
            }
        }
        {   // exclusive, gravity applied
            const std::vector<MeanState<JAC>> ps = st;
            const std::vector<GravAcc> pg = ga;
            for (int l = 0; l < L; l++) {
                if (l == 0) { mean_init(st[0]); grav_init(ga[0]); } else { st[l] = ps[l - 1]; ga[l] = pg[l - 1]; }
                if constexpr (GSEGABLE) grav_apply(st[l], ga[l], gk);
            }
        }
        for (int l = 0; l < L; l++) {
            if (lead[l] < nrows[l]) owner = l;    // the last lane that integrated anything (none: lane 0)
            for (int m = l - 1; m >= 0; m--) if (lead[m] < nrows[m]) { src[l] = m; break; }
        }
        for (int l = 0; l < L; l++) {
            if (src[l] >= 0) continue;
            lead[l] = 0;
            if (cin) load_mean<JAC>(st[l], cin);  // nothing integrated before this lane: the carried state itself
        }
    }
    for (int l = 0; l < L; l++) {   // the walk
        for (int t = 0; t < nrows[l]; t++) {
            const double *k0 = knot(r0[l] + t), *k1 = knot(r0[l] + t + 1);
            mean_step<MODEL, JAC, AVG>(st[l], k0[0], k1[0], ld3(k0 + 1), ld3(k0 + 4), ld3(k1 + 1), ld3(k1 + 4), bw, ba, gk, true);
            if (t >= lead[l]) put_row<JAC>(rows + (size_t)(r0[l] + t) * OUTD, st[l]);
        }
    }
    store_mean<JAC>(cout, st[owner]);
    for (int l = 0; l < L; l++)     // the fix-up: held-back rows repeat the last row of lane src
        for (int t = 0; t < lead[l]; t++) {
            const int m = src[l];
            std::memcpy(rows + (size_t)(r0[l] + t) * OUTD, rows + (size_t)(r0[m] + nrows[m] - 1) * OUTD, 83 * sizeof(double));
        }
}

template <int MODEL, bool AVG>
void cov_rows(int N, int n, const double *kn, const double *lin, const double *qk, const double *sig, const double *grav,
              const double *cin, double *cout, double *rows) {
    typedef CovDims<MODEL> D;
    const int CO = c_cov_off(MODEL);
    const V3 bw = ld3(lin), ba = ld3(lin + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ld4(qk)), ld3(grav));
    n = std::min(std::max(n, 0), N);
    const double q4[4] = { sig[0] * sig[0], sig[1] * sig[1], sig[2] * sig[2], sig[3] * sig[3] };
    const int NL = D::GROUP;
    const int CH = (MODEL == 1) ? 14 : 23;   // intervals per phase-A pass (cpi_cov_kernels.hpp)
    std::vector<CovLane<MODEL>> lane(NL);
    const int IRD = IrPitch<MODEL>::V;
    std::vector<double> exch(exch_doubles(1), 0.0), irs(CH * IRD, 0.0);
    double gs[GS_DOUBLES];
    cov_gs_init(gs);
    if (cin) rec_put_mat(gs, GS_R, ld_cm(cin + C_R));   // (the means of gs are not read out here: they belong to the mean kernel)
    std::vector<int> colof(NL);
    for (int j = 0; j < NL; j++) {
        colof[j] = cov_col_of_lane<MODEL>(j);
        cov_init(lane[j], colof[j], q4);
        cov_exch_init<MODEL>(exch.data(), 1, colof[j], q4);
        if (cin && colof[j] < D::NCOL)
            for (int i = 0; i < D::NR; i++) lane[j].P0[i] = cin[CO + colof[j] * D::NR + i];
    }
    std::vector<int> laneof(D::NCOL + 1, 0);
    for (int j = 0; j < NL; j++) if (colof[j] < D::NCOL) laneof[colof[j]] = j;
    for (int base = 0; base < N; base += CH) {
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
        for (int sl = 0; sl < CH; sl++) {
            const M3 pre = (sl == 0) ? eye() : inc[sl - 1];
            (void)finish_interval<MODEL, AVG>(r[sl], mm(pre, Rc), gk, irs.data() + sl * IRD);
        }
        rec_put_mat(gs, GS_R, mm(inc[CH - 1], Rc));
        const int cnt = std::min(CH, N - base);
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
            double *o = rows + (size_t)(base + sl) * OUTD;   // the read-out of the end, after every interval
            for (int c = 0; c < 15; c++) for (int i = 0; i < 15; i++) o[83 + c * 15 + i] = lane[laneof[c]].P0[i];
        }
    }
    // the covariance block of the record: the columns as row N - 1 has just read them out (N = 0: the carried ones)
    for (int j = 0; j < NL; j++)
        if (colof[j] < D::NCOL)
            for (int i = 0; i < D::NR; i++) cout[CO + colof[j] * D::NR + i] = lane[j].P0[i];
}
}  // namespace

extern "C" int hsrr_carry_doubles(int model) { return c_doubles(model); }
// rows[N][308]; kn: the segment's n + 1 knots (n is clamped into [0, N]); cin = NULL: the zero state; cout: the tag, the means
// and (jac, model 1) the Jacobian block of the record the segment ends in
extern "C" int hsrr_mean(int model, int jac, int avg, int L, int N, int n, const double *kn, const double *lin, const double *qk,
                         const double *grav, const double *cin, double *cout, double *rows) {
    if (L < 1 || L > 64 || (model == 2 && jac)) return 1;
#define GO(M, J, A) mean_rows<M, J, A>(L, N, n, kn, lin, qk, grav, cin, cout, rows)
    if (model == 1 && jac) { if (avg) GO(1, true, true); else GO(1, true, false); }
    else if (model == 1)   { if (avg) GO(1, false, true); else GO(1, false, false); }
    else                   { if (avg) GO(2, false, true); else GO(2, false, false); }
#undef GO
    return 0;
}
// the P rows and the covariance block of cout (the rest of cout is left alone)
extern "C" int hsrr_cov(int model, int avg, int N, int n, const double *kn, const double *lin, const double *qk, const double *sig,
                        const double *grav, const double *cin, double *cout, double *rows) {
#define GO(M, A) cov_rows<M, A>(N, n, kn, lin, qk, sig, grav, cin, cout, rows)
    if (model == 1) { if (avg) GO(1, true); else GO(1, false); }
    else            { if (avg) GO(2, true); else GO(2, false); }
#undef GO
    return 0;
}
