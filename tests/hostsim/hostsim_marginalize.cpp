// hostsim_marginalize.cpp -- HOST restatement of the arithmetic of cpi_marginalize_kernel
// (cpi_amd/csrc/cpi_marginalize_kernels.hpp): chn::marginalize_chain of cpi_math.hpp, whose lane-mapped form the kernel is, one chain
// at a time in the layout of cpi_chain_marginalize_batch.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma().  With
// -DHOSTSIM_MARGINALIZE_MAIN the file is a stand-alone program (seeded chains; the carried prior reproduces the Schur complement
// computed densely in long double; a refused chain with status == NULL; failures with an m of its own per chain), the one to build
// with -fsanitize=address,undefined.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <stdint.h>
#include <vector>
using namespace cpi;

// the states of chain c, clamped as the entries clamp them (cpi_chain_util.hpp: chain_states)
static void states_of(long long G, long long S, const long long *first, const int *count, long long c, long long &f, long long &n) {
    f = first ? first[c] : c * G;
    n = count ? count[c] : G;
    n = n < 0 ? 0 : (n > G ? G : n);
    f = f < 0 ? 0 : (f > S ? S : f);
    if (S - f < n) n = S - f;
}

extern "C" {

// cpi_chain_marginalize_batch on host arrays.  Returns 0.
int hsz_chain_marginalize(long long C, long long G, long long S, long long F, const long long *first, const int *count,
                          const long long *ffirst, const double *hess, const double *prior, int M, const int *drop, double *out, int *status) {
    for (long long c = 0; c < C; c++) {
        long long f, n;
        states_of(G, S, first, count, c, f, n);
        const long long ff = ffirst ? ffirst[c] : f - c;
        const int m = drop ? drop[c] : M;
        int st;
        if ((n > 1 && (ff < 0 || ff > F - (n - 1))) || m < 0 || m >= n) {
            st = -1;
            for (int i = 0; i < chn::PRIOR_D; i++) out[c * chn::PRIOR_D + i] = NAN;
        } else {
            st = chn::marginalize_chain((int)n, m, m > 0 ? hess + ff * chn::HESS_D : nullptr, prior ? prior + f * chn::PRIOR_D : nullptr,
                                        out + c * chn::PRIOR_D);
        }
        if (status) status[c] = st;
    }
    return 0;
}

}  // extern "C"

#ifdef HOSTSIM_MARGINALIZE_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(11);
    const int n = 7, C = 3, m = 4, N = 15 * m;
    const long long S = C * n, F = C * (n - 1);
    // the arrays end where the chains end: a read past the eliminated part of the LAST chain is a read past the allocation
    std::vector<double> hess(F * 496), prior(S * 136, 0.0), out(C * 136, -7.0);
    std::vector<int> status(C, 99), drop = {m, 0, n - 1};
    for (long long k = 0; k < F; k++) {                       // hess row = packed M^T M, M = [-Phi, I + E, r] with small perturbations
        double Mx[15][31];
        for (int i = 0; i < 15; i++)
            for (int j = 0; j < 31; j++) Mx[i][j] = 0.05 * rnd() + (j == i ? -1.0 : 0.0) + (j == 15 + i ? 1.0 : 0.0);
        for (int d = 0; d < 31; d++)
            for (int i = 0; i <= d; i++) {
                double a = 0;
                for (int r = 0; r < 15; r++) a += Mx[r][i] * Mx[r][d];
                hess[k * 496 + chn::tri(d) + i] = a;
            }
    }
    for (long long s = 0; s < S; s++)
        for (int i = 0; i < 15; i++) { prior[s * 136 + chn::tri(i) + i] = 0.1; prior[s * 136 + chn::tri(15) + i] = 0.01 * rnd(); }
    if (hsz_chain_marginalize(C, n, S, F, nullptr, nullptr, nullptr, hess.data(), prior.data(), 0, drop.data(), out.data(), status.data())) return 2;
    // chain 0, densely in long double: [A_EE | A_Em g_E] by Gauss-Jordan without pivoting (positive definite), then the complement
    static long double A[60][60 + 16];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N + 16; j++) A[i][j] = 0;
    for (int k = 0; k < m; k++) {
        const double *H = hess.data() + k * 496;
        for (int i = 0; i < 15; i++) {
            for (int j = 0; j < 15; j++) {
                A[15 * k + i][15 * k + j] += chn::sym_at(H, i, j);
                if (k + 1 < m) {
                    A[15 * k + i][15 * k + 15 + j] += chn::sym_at(H, i, 15 + j);
                    A[15 * k + 15 + i][15 * k + j] += chn::sym_at(H, 15 + i, j);
                    A[15 * k + 15 + i][15 * k + 15 + j] += chn::sym_at(H, 15 + i, 15 + j);
                } else {
                    A[15 * k + i][N + j] += chn::sym_at(H, i, 15 + j);
                }
                A[15 * k + i][15 * k + j] += chn::sym_at(prior.data() + k * 136, i, j);
            }
            A[15 * k + i][N + 15] += chn::sym_at(H, i, 30) + prior[k * 136 + chn::tri(15) + i];
            if (k + 1 < m) A[15 * k + 15 + i][N + 15] += chn::sym_at(H, 15 + i, 30);
        }
    }
    for (int p = 0; p < N; p++) {
        const long double d = A[p][p];
        for (int j = 0; j < N + 16; j++) A[p][j] /= d;
        for (int i = 0; i < N; i++)
            if (i != p) {
                const long double l = A[i][p];
                for (int j = 0; j < N + 16; j++) A[i][j] -= l * A[p][j];
            }
    }
    const double *H = hess.data() + (m - 1) * 496, *Pm = prior.data() + m * 136;
    double worst = 0;
    for (int j = 0; j < 16; j++)
        for (int i = 0; i < 15 && i <= j; i++) {
            long double v = chn::sym_at(H, 15 + i, j < 15 ? 15 + j : 30) + Pm[chn::tri(j) + i];
            for (int k = 0; k < 15; k++) v -= (long double)chn::sym_at(H, k, 15 + i) * A[N - 15 + k][N + j];
            worst = fmax(worst, fabs((double)(v - out[chn::tri(j) + i])) / fmax(1.0, fabs((double)v)));
        }
    bool same = out[135] == 0.0 && out[136 + 135] == 0.0;     // chain 1, m = 0: the prior row as it is
    for (int i = 0; i < 135; i++) same = same && out[136 + i] == prior[n * 136 + i];
    printf("status %d %d %d, |out - Schur complement| %.3g, m = 0 passes the prior through: %d\n", status[0], status[1], status[2], worst, (int)same);
    bool ok = status[0] == 0 && status[1] == 0 && status[2] == 0 && worst < 1e-9 && same;

    // one refused chain (m = n on the LAST chain: what a lax rule would read lies past both allocations) and status == NULL: the row
    // of the refused chain is NaN, the others are the rows of the call above
    std::vector<double> out2(C * 136, -7.0);
    std::vector<int> drop2 = {m, 0, n};
    if (hsz_chain_marginalize(C, n, S, F, nullptr, nullptr, nullptr, hess.data(), prior.data(), 0, drop2.data(), out2.data(), nullptr)) return 2;
    bool refused = true, kept = true;
    for (int i = 0; i < 136; i++) {
        refused = refused && out2[2 * 136 + i] != out2[2 * 136 + i];
        kept = kept && out2[i] == out[i] && out2[136 + i] == out[136 + i];
    }
    printf("m = n with status == NULL: the row is NaN: %d, the other rows are kept: %d\n", (int)refused, (int)kept);
    ok = ok && refused && kept;

    // failures with an m of its own per chain: 8 chains of 4 states (arrays of their own, the factor rows above repeated), pivot k of
    // the block of state s of chain c made -1e12; status = s + 1 if s < m_c, else 0, a failed row is NaN and every other row is finite
    {
        const int C8 = 8, n4 = 4;
        const int fail_s[C8] = {0, 0, 3, 2, -1, 3, 1, -1}, fail_k[C8] = {0, 14, 14, 7, 0, 0, 14, 0};
        const int drops[2][C8] = {{1, 3, 0, 2, 3, 1, 2, 0}, {3, 1, 2, 3, 0, 3, 1, 2}};
        std::vector<double> h8(C8 * (n4 - 1) * 496), p8(C8 * n4 * 136, 0.0), o8(C8 * 136);
        for (size_t i = 0; i < h8.size(); i++) h8[i] = hess[i % hess.size()];
        for (int s = 0; s < C8 * n4; s++)
            for (int i = 0; i < 15; i++) { p8[s * 136 + chn::tri(i) + i] = 0.1; p8[s * 136 + chn::tri(15) + i] = 0.01 * rnd(); }
        for (int c = 0; c < C8; c++)
            if (fail_s[c] >= 0) p8[(c * n4 + fail_s[c]) * 136 + chn::tri(fail_k[c]) + fail_k[c]] = -1e12;
        for (int r = 0; r < 2; r++) {
            std::vector<int> st8(C8, 99), d8(drops[r], drops[r] + C8);
            for (size_t i = 0; i < o8.size(); i++) o8[i] = -7.0;
            if (hsz_chain_marginalize(C8, n4, C8 * n4, C8 * (n4 - 1), nullptr, nullptr, nullptr, h8.data(), p8.data(), 0, d8.data(), o8.data(), st8.data())) return 2;
            bool law = true;
            printf("drop");
            for (int c = 0; c < C8; c++) printf(" %d", d8[c]);
            printf(": status");
            for (int c = 0; c < C8; c++) {
                const int want = (fail_s[c] >= 0 && fail_s[c] < d8[c]) ? fail_s[c] + 1 : 0;
                printf(" %d", st8[c]);
                law = law && st8[c] == want;
                for (int i = 0; i < 136; i++) {
                    const double v = o8[c * 136 + i];
                    law = law && (want ? v != v : (v == v && v != -7.0));
                }
            }
            printf(", the rule holds: %d\n", (int)law);
            ok = ok && law;
        }
    }
    return ok ? 0 : 1;
}
#endif
