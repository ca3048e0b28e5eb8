// hostsim_condense.cpp -- HOST restatement of the arithmetic of cpi_condense_kernel and cpi_expand_kernel
// (cpi_amd/csrc/cpi_condense_kernels.hpp): chn::condense_segment, chn::condense_separator and chn::expand_segment of cpi_math.hpp,
// whose lane-mapped forms the kernels are, one segment at a time in the layouts of cpi_chain_condense_batch / cpi_chain_expand_batch.
// TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma().  With
// -DHOSTSIM_CONDENSE_MAIN the file is a stand-alone program (seeded chains whose arrays end where the chains end; condense, the
// solve's restatement on the reduced chain, expand: the full chain's solve to rounding, for several K and both dampings; K = 1 is a
// copy; a failed interior), the one to build with -fsanitize=address,undefined.
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
static long long reduced_states(long long n, long long K) { return n >= 2 ? (n - 2) / K + 2 : n; }

extern "C" {

long long hsc_condense_states(long long G, long long K) { return reduced_states(G, K); }
long long hsc_condense_workspace_doubles(long long S) { return S > 0 ? S * chn::CS_D : 1; }

// cpi_chain_condense_batch on host arrays.  Returns 0.
int hsc_chain_condense(long long C, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst,
                       const double *hess, const double *prior, const double *lambda, int diagonal, long long K, double *rhess,
                       double *rprior, int *rcount, int *status, double *workspace) {
    const long long Gr = reduced_states(G, K);
    for (long long c = 0; c < C; c++) {
        long long f, n;
        states_of(G, S, first, count, c, f, n);
        const long long ff = ffirst ? ffirst[c] : f - c, m = reduced_states(n, K);
        const bool bad = n > 1 && (ff < 0 || ff > F - (n - 1));
        const double lam = lambda ? lambda[c] : 0.0;
        rcount[c] = (int)m;
        for (long long j = 0; j < m; j++) {                                  // the separators
            const long long s = (j < m - 1) ? j * K : n - 1;
            chn::condense_separator((!bad && s > 0) ? hess + (ff + s - 1) * chn::HESS_D : nullptr, (!bad && s < n - 1) ? hess + (ff + s) * chn::HESS_D : nullptr,
                                    prior ? prior + (f + s) * chn::PRIOR_D : nullptr, lambda != nullptr, lam, diagonal, rprior + (c * Gr + j) * chn::PRIOR_D);
        }
        for (long long j = 0; j + 1 < Gr; j++) {
            int st = 0;
            if (j + 1 < m) {
                const long long a = j * K, b = (n - 1 - a < K) ? n - 1 : a + K;
                double *out = rhess + (c * (Gr - 1) + j) * chn::HESS_D;
                if (bad) {
                    st = -1;
                    for (int i = 0; i < chn::HESS_D; i++) out[i] = NAN;
                } else {
                    const int t = chn::condense_segment((int)(b - a), hess + (ff + a) * chn::HESS_D, prior ? prior + (f + a) * chn::PRIOR_D : nullptr, lam,
                                                        diagonal, workspace + (f + a) * chn::CS_D, out);
                    st = t ? (int)(a + t + 1) : 0;
                }
            }
            if (status) status[c * (Gr - 1) + j] = st;
        }
    }
    return 0;
}

// cpi_chain_expand_batch on host arrays.  Returns 0.
int hsc_chain_expand(long long C, long long G, long long S, const long long *first, const int *count, long long K, const double *rdelta,
                     const double *workspace, double *delta) {
    const long long Gr = reduced_states(G, K);
    for (long long c = 0; c < C; c++) {
        long long f, n;
        states_of(G, S, first, count, c, f, n);
        const long long m = reduced_states(n, K);
        for (long long j = 0; j < m; j++) {
            const long long s = (j < m - 1) ? j * K : n - 1;
            for (int i = 0; i < 15; i++) delta[(f + s) * 15 + i] = rdelta[(c * Gr + j) * 15 + i];
        }
        for (long long j = 0; j + 1 < m; j++) {
            const long long a = j * K, b = (n - 1 - a < K) ? n - 1 : a + K;
            chn::expand_segment((int)(b - a), workspace + (f + a) * chn::CS_D, rdelta + (c * Gr + j) * 15, rdelta + (c * Gr + j + 1) * 15, delta + (f + a) * 15);
        }
    }
    return 0;
}

// cpi_chain_solve_batch on host arrays (chn::solve_chain), for the reduced chain between the two calls above.  Returns 0.
int hsc_chain_solve(long long C, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst,
                    const double *hess, const double *prior, const double *lambda, int diagonal, double *delta, int *status) {
    std::vector<double> ws((size_t)(G > 0 ? G : 1) * chn::WS_D);
    for (long long c = 0; c < C; c++) {
        long long f, n;
        states_of(G, S, first, count, c, f, n);
        const long long ff = ffirst ? ffirst[c] : f - c;
        int st = 0;
        if (n > 1 && (ff < 0 || ff > F - (n - 1))) {
            st = -1;
            for (long long i = 0; i < n * 15; i++) delta[f * 15 + i] = NAN;
        } else if (n > 0) {
            st = chn::solve_chain((int)n, n > 1 ? hess + ff * chn::HESS_D : nullptr, prior ? prior + f * chn::PRIOR_D : nullptr, lambda ? lambda[c] : 0.0,
                                  diagonal, ws.data(), delta + f * 15);
        }
        if (status) status[c] = st;
    }
    return 0;
}

}  // extern "C"

#ifdef HOSTSIM_CONDENSE_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(13);
    const int C = 3, G = 11;
    const int counts[C] = {11, 6, 1};
    const long long S = C * G, F = C * (G - 1);
    std::vector<double> hess(F * 496), prior(S * 136, 0.0), lam = {0.5, 0.25, 2.0};
    std::vector<int> count(counts, counts + C);
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
    bool ok = true;
    for (int diagonal = 0; diagonal < 2; diagonal++) {
        std::vector<double> full(S * 15, -7.0);
        std::vector<int> fst(C, 99);
        if (hsc_chain_solve(C, G, S, F, nullptr, count.data(), nullptr, hess.data(), prior.data(), lam.data(), diagonal, full.data(), fst.data())) return 2;
        for (long long K : {1, 2, 3, 4, 7, 10, 40}) {
            const long long Gr = hsc_condense_states(G, K);
            std::vector<double> rh((Gr - 1) * C * 496, -7.0), rp(Gr * C * 136, -7.0), ws(hsc_condense_workspace_doubles(S), -7.0), rd(Gr * C * 15, -7.0), delta(S * 15, -7.0);
            std::vector<int> rc(C, 99), sst(C * (Gr - 1), 99), rst(C, 99);
            if (hsc_chain_condense(C, G, S, F, nullptr, count.data(), nullptr, hess.data(), prior.data(), lam.data(), diagonal, K, rh.data(), rp.data(), rc.data(), sst.data(), ws.data())) return 2;
            if (hsc_chain_solve(C, Gr, C * Gr, C * (Gr - 1), nullptr, rc.data(), nullptr, rh.data(), rp.data(), nullptr, 0, rd.data(), rst.data())) return 2;
            if (hsc_chain_expand(C, G, S, nullptr, count.data(), K, rd.data(), ws.data(), delta.data())) return 2;
            double worst = 0, scale = 0;
            bool untouched = true, copied = true;
            for (int c = 0; c < C; c++) {
                for (long long s = 0; s < G; s++)
                    for (int i = 0; i < 15; i++) {
                        const double got = delta[(c * G + s) * 15 + i], want = full[(c * G + s) * 15 + i];
                        if (s < counts[c]) { worst = fmax(worst, fabs(got - want)); scale = fmax(scale, fabs(want)); }
                        else untouched = untouched && got == -7.0;
                    }
                if (K == 1)
                    for (int k = 0; k + 1 < counts[c]; k++)
                        for (int i = 0; i < 496; i++) copied = copied && rh[(c * (Gr - 1) + k) * 496 + i] == hess[(c * (G - 1) + k) * 496 + i];
            }
            bool st0 = true;
            for (int v : sst) st0 = st0 && v == 0;
            for (int v : rst) st0 = st0 && v == 0;
            printf("damping %d K %lld: Gr %lld, rcount %d %d %d, |segmented - full| %.3g of %.3g, rows of no state untouched: %d, K = 1 copies: %d, status 0: %d\n",
                   diagonal, K, Gr, rc[0], rc[1], rc[2], worst, scale, (int)untouched, (int)copied, (int)st0);
            ok = ok && worst <= 1e-10 * scale && untouched && copied && st0;
        }
    }
    {   // a failed interior: state 5 of chain 0 (K = 4: the second segment, states 4 .. 8); its row is NaN, the others are as before
        const long long K = 4, Gr = hsc_condense_states(G, K);
        std::vector<double> rh((Gr - 1) * C * 496, -7.0), rh2 = rh, rp(Gr * C * 136), ws(hsc_condense_workspace_doubles(S));
        std::vector<int> rc(C), s1(C * (Gr - 1), 99), s2 = s1;
        hsc_chain_condense(C, G, S, F, nullptr, count.data(), nullptr, hess.data(), prior.data(), nullptr, 0, K, rh.data(), rp.data(), rc.data(), s1.data(), ws.data());
        std::vector<double> p2 = prior;
        p2[5 * 136 + chn::tri(7) + 7] = -1e12;
        hsc_chain_condense(C, G, S, F, nullptr, count.data(), nullptr, hess.data(), p2.data(), nullptr, 0, K, rh2.data(), rp.data(), rc.data(), s2.data(), ws.data());
        bool law = s2[1] == 6;
        for (size_t i = 0; i < rh.size(); i++) {
            const bool in = i / 496 == 1;
            law = law && (in ? rh2[i] != rh2[i] : (rh2[i] == rh[i]));
        }
        for (size_t i = 0; i < s1.size(); i++) law = law && (i == 1 || s2[i] == s1[i]);
        printf("a failed interior: status %d, the rule holds: %d\n", s2[1], (int)law);
        ok = ok && law;
    }
    return ok ? 0 : 1;
}
#endif
