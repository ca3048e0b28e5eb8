// test_marginalize.cpp -- GPU: cpi_host::chain_marginalize end to end, product only.  The chains of test_marginals.cpp, whose answer is
// known in closed form: every factor is [A1 A2] = [-I, I] and the first state carries the prior Lam = I, eta_i = i + 1 -- a random walk
// of unit steps from a unit prior, so the first state that stays after `drop` states have left carries Lam = I / (drop + 1) and
// eta = eta_0 / (drop + 1).  Checks itself, then prints every entry of the result as a hexadecimal double (one chain per line) for the
// caller to compare with the device form's bits.
//   test_marginalize
#include <cmath>
#include <cstdio>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

int main() {
    try {
        Context ctx;
        const int64_t C = 5, G = 4;
        const int32_t drop = 2;
        std::vector<double> hess((size_t)(C * (G - 1)) * 496, 0.0), prior((size_t)(C * G) * 136, 0.0);
        auto at = [](int i, int d) { return (size_t)(i + d * (d + 1) / 2); };
        for (int64_t c = 0; c < C; c++) {
            for (int i = 0; i < 15; i++) { prior[(size_t)(c * G) * 136 + at(i, i)] = 1.0; prior[(size_t)(c * G) * 136 + at(i, 15)] = (double)(i + 1 + c); }
            for (int64_t k = 0; k < G - 1; k++) {
                double *H = hess.data() + (size_t)(c * (G - 1) + k) * 496;
                for (int i = 0; i < 15; i++) { H[at(i, i)] = 1.0; H[at(15 + i, 15 + i)] = 1.0; H[at(i, 15 + i)] = -1.0; }   // [-I I]^T [-I I]
            }
        }
        std::vector<int32_t> status;
        const std::vector<double> out = chain_marginalize(ctx, C, G, hess, prior, drop, &status);
        int bad = 0;
        if (out.size() != (size_t)C * 136) { printf("out has %zu entries\n", out.size()); return 1; }
        for (int64_t c = 0; c < C; c++) {
            if (status[(size_t)c] != 0) { printf("chain %lld: status %d\n", (long long)c, status[(size_t)c]); bad++; }
            for (int j = 0; j < 16; j++)
                for (int i = 0; i <= j && i < 15; i++) {
                    const double want = (j == 15) ? (double)(i + 1 + c) / (drop + 1) : ((i == j) ? 1.0 / (drop + 1) : 0.0);
                    const double got = out[(size_t)c * 136 + at(i, j)];
                    if (!(std::fabs(got - want) <= 1e-12)) { printf("chain %lld (%d, %d): %.17g, expected %.17g\n", (long long)c, i, j, got, want); bad++; }
                }
            if (out[(size_t)c * 136 + 135] != 0.0) { printf("chain %lld: entry 135 is %.17g\n", (long long)c, out[(size_t)c * 136 + 135]); bad++; }
        }
        try { chain_marginalize(ctx, C, G, std::vector<double>(7)); printf("a short hess was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        try { chain_marginalize(ctx, C, G, hess, prior, (int32_t)G); printf("drop = G was accepted\n"); bad++; } catch (const std::exception &) {}
        if (bad) return 1;
        for (int64_t c = 0; c < C; c++) {
            for (int i = 0; i < 136; i++) printf("%a ", out[(size_t)c * 136 + i]);
            printf("\n");
        }
        printf("test_marginalize ok %lld %lld %d\n", (long long)C, (long long)G, (int)drop);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
