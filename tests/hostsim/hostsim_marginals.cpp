// hostsim_marginals.cpp -- HOST restatement of the arithmetic of cpi_marginals_kernel (cpi_amd/csrc/cpi_marginals_kernels.hpp):
// chn::marginals_chain of cpi_math.hpp, whose lane-mapped form the kernel is, beside chn::solve_chain, which leaves the workspace
// records it reads; one chain at a time in the layout of cpi_chain_marginals_batch.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma().  With
// -DHOSTSIM_MARGINALS_MAIN the file is a stand-alone program (seeded chains, Sigma A = I on the first block row), the one to build
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

// The solve on host arrays (hostsim_chain.cpp: hsc_chain_solve), leaving the workspace.  solve_chain DOES write a W record for a
// chain's last state; poison_last overwrites it with NaN afterwards, as a witness that marginals_chain does not read it.
int hsm_chain_solve(long long C, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst,
                    const double *hess, const double *prior, const double *lambda, int diagonal, double *delta, int *status,
                    double *workspace, int poison_last) {
    for (long long c = 0; c < C; c++) {
        long long f, n;
        states_of(G, S, first, count, c, f, n);
        const long long ff = ffirst ? ffirst[c] : f - c;
        int st = 0;
        if (n > 1 && (ff < 0 || ff > F - (n - 1))) {
            st = -1;
            for (long long i = 0; i < n * 15; i++) delta[f * 15 + i] = NAN;
        } else if (n > 0) {
            st = chn::solve_chain((int)n, n > 1 ? hess + ff * chn::HESS_D : nullptr, prior ? prior + f * chn::PRIOR_D : nullptr,
                                  lambda ? lambda[c] : 0.0, diagonal, workspace + f * chn::WS_D, delta + f * 15);
            if (poison_last)
                for (int i = 0; i < 225; i++) workspace[(f + n - 1) * chn::WS_D + chn::WS_R + i] = NAN;
        }
        if (status) status[c] = st;
    }
    return 0;
}

// cpi_chain_marginals_batch on host arrays.  Returns 0.
int hsm_chain_marginals(long long C, long long G, long long S, const long long *first, const int *count, const int *status,
                        const double *workspace, double *cov, double *cross) {
    for (long long c = 0; c < C; c++) {
        long long f, n;
        states_of(G, S, first, count, c, f, n);
        if (n <= 0) continue;
        if (status && status[c] != 0) {
            for (long long i = 0; i < n * 120; i++) cov[f * 120 + i] = NAN;
            if (cross)
                for (long long i = 0; i < (n - 1) * 225; i++) cross[f * 225 + i] = NAN;
            continue;
        }
        chn::marginals_chain((int)n, workspace + f * chn::WS_D, cov + f * 120, cross ? cross + f * 225 : nullptr);
    }
    return 0;
}

int hsm_ws_doubles() { return chn::WS_D; }

}  // extern "C"

#ifdef HOSTSIM_MARGINALS_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(11);
    const int n = 7, C = 3;
    const long long S = C * n, F = C * (n - 1);
    std::vector<double> hess(F * 496), prior(S * 136, 0.0), delta(S * 15, -7.0), ws(S * chn::WS_D), cov(S * 120, -7.0), cross(S * 225, -7.0);
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
    if (hsm_chain_solve(C, n, S, F, nullptr, nullptr, nullptr, hess.data(), prior.data(), nullptr, 0, delta.data(), status.data(), ws.data(), 1)) return 2;
    if (hsm_chain_marginals(C, n, S, nullptr, nullptr, status.data(), ws.data(), cov.data(), cross.data())) return 2;
    // block row 0 of chain 0 of A Sigma = I, column block 0: D_0 Sigma[0][0] + U_0 Sigma[0][1]^T = I
    double worst = 0;
    for (int i = 0; i < 15; i++)
        for (int j = 0; j < 15; j++) {
            double r = (i == j) ? -1.0 : 0.0;
            for (int k = 0; k < 15; k++) {
                r += (chn::sym_at(hess.data(), i, k) + chn::sym_at(prior.data(), i, k)) * chn::sym_at(cov.data(), k, j);
                r += hess[chn::tri(15 + k) + i] * cross[j + 15 * k];
            }
            worst = fmax(worst, fabs(r));
        }
    const bool kept = cross[(n - 1) * 225] == -7.0;          // the cross row of the last state is not written
    printf("status %d %d %d, |A Sigma - I| on block (0, 0): %.3g, last cross row kept: %d\n", status[0], status[1], status[2], worst, (int)kept);
    return (status[0] == 0 && status[1] == 0 && status[2] == 0 && worst < 1e-9 && kept) ? 0 : 1;
}
#endif
