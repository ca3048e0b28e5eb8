// hostsim_merge.cpp -- HOST emulation of cpi_merge_kernel (cpi_amd/csrc/cpi_merge_kernels.hpp), built on its CPI_HD arithmetic the way
// hostsim_stj.cpp is built on cov_body's.  TEST INFRASTRUCTURE ONLY.
//
// One output row at a time, the kernel's orchestration with loops where the kernel has lanes: the operand is staged into the group's
// stage (the 56 small doubles, then P dense or packed), the 15 covariance lanes read their column, the left half writes U and V over
// the exchange areas, the right half reads their rows back, a third exchange symmetrises; lanes 0..5 carry their Jacobian triple; the
// means go through mean_combine.  Every "all lanes read before any lane writes" of the kernel's fences is a loop boundary here.
// Rows (in and out) are 401 doubles: the staged operand layout (DT 0, alpha 1, beta 4, q 7, J_q 11, J_a 20, J_b 29, H_a 38, H_b 47,
// column-major), P at 56 (225), P_sym at 281 (120).
//
// With -DHOSTSIM_MERGE_MAIN the file is a stand-alone program (seeded rows, ragged groups, self-checks), the one to build with
// -fsanitize=address,undefined.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include "../../include/cpi_amd.h"
#include "../../cpi_amd/csrc/cpi_merge_kernels.hpp"
#include <string.h>
using namespace cpi;
using namespace cpi::merge;

namespace {
const int ROW = 401, ROW_P = 56, ROW_PSYM = 281;

void merge_row(long long j, int G, long long in_rows, const double *in, bool tri, const long long *first, const int *count,
               bool jac, bool cov, double *o) {
    long long f;
    int n;
    group_range(j, G, in_rows, first, count, f, n);
    MeanState<false> S;
    mean_init(S);
    JacCol X[6];
    for (int l = 0; l < 6; l++) X[l] = jac_col_zero();
    Col15 pa[15], pb[15], pn[15];
    for (int c = 0; c < 15; c++) pa[c] = col_zero();
    double st[STAGE_DOUBLES];
    for (int k = 0; k < n; k++) {
        const double *row = in + (size_t)(f + k) * ROW;
        memcpy(st, row, OP_DOUBLES * sizeof(double));
        if (cov) memcpy(st + STAGE_P, row + (tri ? ROW_PSYM : ROW_P), (tri ? CPI_TRI_DOUBLES : 225) * sizeof(double));
        if (cov)
            for (int c = 0; c < 15; c++) pb[c] = tri ? col_load_tri(st + STAGE_P, c) : col_load(st + STAGE_P + c * 15, 1);
        if (k == 0) {
            load_state(S, st);
            for (int l = 0; l < 6 && jac; l++) {
                int o1, o2, o3;
                jac_col_offsets(l, o1, o2, o3);
                X[l] = jac_col_load(st, o1, o2, o3);
            }
            for (int c = 0; c < 15; c++) pa[c] = pb[c];
            continue;
        }
        if (cov) {
            for (int c = 0; c < 15; c++) {
                col_store(st + STAGE_P + c * 15, 1, t_apply(S.R, pb[c]));
                col_store(st + STAGE_X + c * 15, 1, phi_apply(S.R, st, pa[c]));
            }
            for (int c = 0; c < 15; c++)
                pn[c] = col_add(phi_apply(S.R, st, col_load(st + STAGE_X + c, 15)), t_apply(S.R, col_load(st + STAGE_P + c, 15)));
            for (int c = 0; c < 15; c++) col_store(st + STAGE_X + c * 15, 1, pn[c]);
            for (int c = 0; c < 15; c++) pa[c] = col_mean(pn[c], col_load(st + STAGE_X + c, 15));
        }
        MeanState<false> B;
        load_state(B, st);
        for (int l = 0; l < 6 && jac; l++) {
            int o1, o2, o3;
            jac_col_offsets(l, o1, o2, o3);
            jac_col_combine(X[l], S.R, B, jac_col_load(st, o1, o2, o3));
        }
        mean_combine(S, B);
    }
    Q4 q; q.x = 0; q.y = 0; q.z = 0; q.w = 1;
    if (n == 1) q = op_quat(in + (size_t)f * ROW);
    else if (n > 1) q = rot_2_quat(S.R);
    o[OP_DT] = S.DT;
    st3s(o + OP_ALPHA, 1, S.alpha);
    st3s(o + OP_BETA, 1, S.beta);
    o[OP_Q] = q.x; o[OP_Q + 1] = q.y; o[OP_Q + 2] = q.z; o[OP_Q + 3] = q.w;
    if (jac) {
        for (int l = 0; l < 3; l++) { st3s(o + OP_JQ + 3 * l, 1, X[l].x1); st3s(o + OP_JB + 3 * l, 1, X[l].x2); st3s(o + OP_JA + 3 * l, 1, X[l].x3); }
        for (int l = 3; l < 6; l++) { st3s(o + OP_HB + 3 * (l - 3), 1, X[l].x2); st3s(o + OP_HA + 3 * (l - 3), 1, X[l].x3); }
    }
    if (cov)
        for (int c = 0; c < 15; c++) {
            double col[15];
            col_store(col, 1, pa[c]);
            for (int i = 0; i < 15; i++) {
                o[ROW_P + c * 15 + i] = col[i];
                if (i <= c) o[ROW_PSYM + CPI_TRI_INDEX(i, c)] = col[i];
            }
        }
}
}  // namespace

// out[M][401] from in[in_rows][401]; tri: the operands' covariance is read from their P_sym; first / count may be NULL as in
// cpi_merge_batch.  Fields that are not asked for (jac / cov == 0) are left as they are.
extern "C" int hsm_merge(long long M, int G, long long in_rows, const double *in, int tri, const long long *first, const int *count,
                         int jac, int cov, double *out) {
    if (G < 1 || M < 0 || in_rows < 0) return 1;
    for (long long j = 0; j < M; j++) merge_row(j, G, in_rows, in, tri != 0, first, count, jac != 0, cov != 0, out + (size_t)j * ROW);
    return 0;
}

#ifdef HOSTSIM_MERGE_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>
// seeded rows (small rotations, a symmetric positive covariance), dense and ragged groups, the contract's corners as self-checks
int main() {
    const long long in_rows = 37;
    const int G = 5;
    std::vector<double> in((size_t)in_rows * ROW);
    srand(7);
    auto rnd = []() { return rand() / (double)RAND_MAX - 0.5; };
    for (long long r = 0; r < in_rows; r++) {
        double *p = in.data() + (size_t)r * ROW;
        for (int i = 0; i < ROW_P; i++) p[i] = 0.1 * rnd();
        p[OP_DT] = 0.05;
        const V3 w = mk(0.2 * rnd(), 0.2 * rnd(), 0.2 * rnd());
        const Q4 q = rot_2_quat(Exp_so3(w));
        p[OP_Q] = q.x; p[OP_Q + 1] = q.y; p[OP_Q + 2] = q.z; p[OP_Q + 3] = q.w;
        double L[15][15];
        for (int i = 0; i < 15; i++) for (int k = 0; k < 15; k++) L[i][k] = (k <= i) ? 1e-3 * rnd() + (i == k ? 1e-2 : 0) : 0;
        for (int i = 0; i < 15; i++)
            for (int k = 0; k <= i; k++) {
                double s = 0;
                for (int m = 0; m < 15; m++) s += L[i][m] * L[k][m];
                p[ROW_P + i * 15 + k] = p[ROW_P + k * 15 + i] = s;
                p[ROW_PSYM + CPI_TRI_INDEX(k, i)] = s;
            }
    }
    const long long M = 9;
    const long long first[M] = { 0, 3, 3, 36, 30, 37, -4, 100, 10 };
    const int count[M] = { 5, 1, 0, 5, 9, 3, 2, -1, 4 };
    std::vector<double> a((size_t)M * ROW, -1.0), b((size_t)M * ROW, -1.0), d((size_t)8 * ROW, -1.0);
    int bad = 0;
    bad += hsm_merge(M, G, in_rows, in.data(), 0, first, count, 1, 1, a.data());
    bad += hsm_merge(M, G, in_rows, in.data(), 1, first, count, 1, 1, b.data());
    bad += hsm_merge(8, G, in_rows, in.data(), 0, nullptr, nullptr, 1, 1, d.data());   // dense: the last group is clipped to 2 rows
    bad += memcmp(a.data(), b.data(), a.size() * sizeof(double)) != 0;                  // P_sym in == P in
    bad += memcmp(a.data() + ROW, in.data() + 3 * ROW, ROW * sizeof(double)) != 0;      // count 1: the row itself
    bad += memcmp(a.data() + 3 * ROW, in.data() + 36 * ROW, ROW * sizeof(double)) != 0; // clipped to one row
    for (int i = 0; i < ROW; i++) bad += a[2 * ROW + i] != ((i == OP_Q + 3) ? 1.0 : 0.0);   // count 0: the zero state
    for (int i = 0; i < ROW; i++) bad += a[5 * ROW + i] != ((i == OP_Q + 3) ? 1.0 : 0.0);   // first == in_rows: nothing left
    for (int i = 0; i < ROW; i++) bad += a[7 * ROW + i] != ((i == OP_Q + 3) ? 1.0 : 0.0);   // count < 0
    for (long long j = 0; j < M; j++)
        for (int i = 0; i < 15; i++)
            for (int k = 0; k < 15; k++) bad += a[j * ROW + ROW_P + i * 15 + k] != a[j * ROW + ROW_P + k * 15 + i];
    printf("hostsim_merge self-check: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
#endif
