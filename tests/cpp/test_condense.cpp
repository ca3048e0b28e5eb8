// test_condense.cpp -- GPU: cpi_host::chain_condense / chain_expand / chain_solve_segmented end to end, product only.  The chains of
// test_marginalize.cpp, whose answer is known in closed form: every factor is [A1 A2] = [-I, I] with a zero residual and the first state
// carries the prior Lam = I, eta_i = i + 1 + c -- a random walk of unit steps from a unit prior, so every state's delta is eta.  Checks
// itself (the closed form, the plain solve, the layout of the reduced chain), then prints every entry of delta as a hexadecimal double
// (one state per line) for the caller to compare with the device form's bits.
//   test_condense
#include <cmath>
#include <cstdio>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

int main() {
    try {
        Context ctx;
        const int64_t C = 3, G = 12, K = 4;
        std::vector<double> hess((size_t)(C * (G - 1)) * 496, 0.0), prior((size_t)(C * G) * 136, 0.0);
        auto at = [](int i, int d) { return (size_t)(i + d * (d + 1) / 2); };
        for (int64_t c = 0; c < C; c++) {
            for (int i = 0; i < 15; i++) { prior[(size_t)(c * G) * 136 + at(i, i)] = 1.0; prior[(size_t)(c * G) * 136 + at(i, 15)] = (double)(i + 1 + c); }
            for (int64_t k = 0; k < G - 1; k++) {
                double *H = hess.data() + (size_t)(c * (G - 1) + k) * 496;
                for (int i = 0; i < 15; i++) { H[at(i, i)] = 1.0; H[at(15 + i, 15 + i)] = 1.0; H[at(i, 15 + i)] = -1.0; }   // [-I I]^T [-I I]
            }
        }
        int bad = 0;
        const CondensedChains r = chain_condense(ctx, C, G, K, hess, prior);
        if (r.Gr != 4 || r.rhess.size() != (size_t)(C * 3) * 496 || r.rprior.size() != (size_t)(C * 4) * 136 || r.status.size() != (size_t)(C * 3)) {
            printf("the reduced layout: Gr %lld, %zu, %zu, %zu\n", (long long)r.Gr, r.rhess.size(), r.rprior.size(), r.status.size());
            return 1;
        }
        for (int64_t c = 0; c < C; c++) {
            if (r.rcount[(size_t)c] != 4) { printf("chain %lld: rcount %d\n", (long long)c, r.rcount[(size_t)c]); bad++; }
            for (int j = 0; j < 3; j++)
                if (r.status[(size_t)(c * 3 + j)] != 0) { printf("chain %lld segment %d: status %d\n", (long long)c, j, r.status[(size_t)(c * 3 + j)]); bad++; }
            // a run of L unit steps is one step of information 1 / L: segments of 4, 4 and 3 factors
            for (int j = 0; j < 3; j++) {
                const double w = 1.0 / (j < 2 ? 4 : 3);
                const double *M = r.rhess.data() + (size_t)(c * 3 + j) * 496;
                for (int i = 0; i < 15; i++)
                    if (!(std::fabs(M[at(i, i)] - w) <= 1e-12 && std::fabs(M[at(15 + i, 15 + i)] - w) <= 1e-12 && std::fabs(M[at(i, 15 + i)] + w) <= 1e-12)) {
                        printf("chain %lld segment %d entry %d: %.17g %.17g %.17g, expected %.17g\n", (long long)c, j, i, M[at(i, i)], M[at(15 + i, 15 + i)], M[at(i, 15 + i)], w);
                        bad++;
                    }
            }
        }
        std::vector<int32_t> status, status2;
        const std::vector<double> delta = chain_solve_segmented(ctx, C, G, K, hess, prior, {}, false, &status);
        const std::vector<double> plain = chain_solve(ctx, C, G, hess, prior, {}, false, &status2);
        if (delta.size() != (size_t)(C * G) * 15) { printf("delta has %zu entries\n", delta.size()); return 1; }
        for (int64_t c = 0; c < C; c++) {
            if (status[(size_t)c] != 0 || status2[(size_t)c] != 0) { printf("chain %lld: status %d %d\n", (long long)c, status[(size_t)c], status2[(size_t)c]); bad++; }
            for (int64_t s = 0; s < G; s++)
                for (int i = 0; i < 15; i++) {
                    const double want = (double)(i + 1 + c), got = delta[(size_t)(c * G + s) * 15 + i], pl = plain[(size_t)(c * G + s) * 15 + i];
                    if (!(std::fabs(got - want) <= 1e-11 && std::fabs(got - pl) <= 1e-11)) {
                        printf("chain %lld state %lld entry %d: %.17g, plain %.17g, expected %.17g\n", (long long)c, (long long)s, i, got, pl, want);
                        bad++;
                    }
                }
        }
        try { chain_condense(ctx, C, G, 0, hess, prior); printf("K = 0 was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        try { chain_condense(ctx, C, G, K, std::vector<double>(7)); printf("a short hess was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        try { chain_expand(ctx, C, G, K, std::vector<double>(7), r.workspace); printf("a short rdelta was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        if (bad) return 1;
        for (int64_t s = 0; s < C * G; s++) {
            for (int i = 0; i < 15; i++) printf("%a ", delta[(size_t)s * 15 + i]);
            printf("\n");
        }
        printf("test_condense ok %lld %lld %lld\n", (long long)C, (long long)G, (long long)K);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
