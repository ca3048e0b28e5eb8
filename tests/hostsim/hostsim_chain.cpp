// hostsim_chain.cpp -- HOST restatement of the arithmetic of cpi_chain_solve_kernel (cpi_amd/csrc/cpi_chain_kernels.hpp): the CPI_HD
// functions of namespace chn in cpi_math.hpp, whose lane-mapped form the kernel is, one chain at a time in the layout of
// cpi_chain_solve_batch.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma().  With
// -DHOSTSIM_CHAIN_MAIN the file is a stand-alone program (seeded chains, residual check), the one to build with
// -fsanitize=address,undefined.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <stdint.h>
#include <vector>
using namespace cpi;

extern "C" {

// the entry's arguments on host arrays; workspace: S * chn::WS_D doubles.  Returns 0.
int hsc_chain_solve(long long C, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst,
                    const double *hess, const double *prior, const double *lambda, int diagonal, double *delta, int *status,
                    double *workspace) {
    for (long long c = 0; c < C; c++) {
        long long f = first ? first[c] : c * G;
        long long n = count ? count[c] : G;
        n = n < 0 ? 0 : (n > G ? G : n);
        f = f < 0 ? 0 : (f > S ? S : f);
        if (S - f < n) n = S - f;
        const long long ff = ffirst ? ffirst[c] : f - c;
        int st = 0;
        if (n > 1 && (ff < 0 || ff > F - (n - 1))) {
            st = -1;
            for (long long i = 0; i < n * 15; i++) delta[f * 15 + i] = NAN;
        } else if (n > 0) {
            st = chn::solve_chain((int)n, n > 1 ? hess + ff * chn::HESS_D : nullptr, prior ? prior + f * chn::PRIOR_D : nullptr,
                                  lambda ? lambda[c] : 0.0, diagonal, workspace + f * chn::WS_D, delta + f * 15);
        }
        if (status) status[c] = st;
    }
    return 0;
}

int hsc_ws_doubles() { return chn::WS_D; }

}  // extern "C"

#ifdef HOSTSIM_CHAIN_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(11);
    const int n = 7, C = 3;
    const long long S = C * n, F = C * (n - 1);
    std::vector<double> hess(F * 496), prior(S * 136, 0.0), delta(S * 15, -7.0), ws(S * chn::WS_D);
    std::vector<int> status(C, 99);
    for (long long k = 0; k < F; k++) {                       // hess row = packed M^T M, M = [-Phi, I + E, r] with small perturbations
        double M[15][31];
        for (int i = 0; i < 15; i++)
            for (int j = 0; j < 31; j++) M[i][j] = 0.05 * rnd() + (j == i ? -1.0 : 0.0) + (j == 15 + i ? 1.0 : 0.0);
        for (int d = 0; d < 31; d++)
            for (int i = 0; i <= d; i++) {
                double a = 0;
                for (int r = 0; r < 15; r++) a += M[r][i] * M[r][d];
                hess[k * 496 + chn::tri(d) + i] = a;
            }
    }
    for (long long s = 0; s < S; s++)
        for (int i = 0; i < 15; i++) { prior[s * 136 + chn::tri(i) + i] = 0.1; prior[s * 136 + chn::tri(15) + i] = 0.01 * rnd(); }
    if (hsc_chain_solve(C, n, S, F, nullptr, nullptr, nullptr, hess.data(), prior.data(), nullptr, 0, delta.data(), status.data(), ws.data())) return 2;
    // residual of block row 0 of chain 0: D_0 d_0 + U_0 d_1 - g_0
    double worst = 0;
    for (int i = 0; i < 15; i++) {
        double r = -(hess[chn::tri(30) + i] + prior[chn::tri(15) + i]);
        for (int j = 0; j < 15; j++) {
            r += (chn::sym_at(hess.data(), i, j) + chn::sym_at(prior.data(), i, j)) * delta[j];
            r += hess[chn::tri(15 + j) + i] * delta[15 + j];
        }
        worst = fmax(worst, fabs(r));
    }
    printf("status %d %d %d, residual of block row 0: %.3g\n", status[0], status[1], status[2], worst);
    return (status[0] == 0 && status[1] == 0 && status[2] == 0 && worst < 1e-10) ? 0 : 1;
}
#endif
