// hostsim_marginalize.cpp -- HOST restatement of the arithmetic of cpi_marginalize_kernel
// (cpi_amd/csrc/cpi_marginalize_kernels.hpp): chn::marginalize_chain of cpi_math.hpp, whose lane-mapped form the kernel is, one chain
// at a time in the layout of cpi_chain_marginalize_batch.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma().  With
// -DHOSTSIM_MARGINALIZE_MAIN the file is a stand-alone program (seeded chains; the carried prior reproduces the Schur complement
// computed densely in long double), the one to build with -fsanitize=address,undefined.
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
    return (status[0] == 0 && status[1] == 0 && status[2] == 0 && worst < 1e-9 && same) ? 0 : 1;
}
#endif
