// test_chain.cpp -- GPU: cpi_host::chain_solve end to end, product only.  Chains of identity-like factors whose solution is known in
// closed form: every factor is [A1 A2 b] = [-I, I, r] and the first state carries the prior Lam = I, eta = 0, so
// delta_0 = 0 and delta_{s+1} = delta_s + r_s exactly (the system is block bidiagonal after elimination; small integers, no rounding).
// Checks itself.
//   test_chain
#include <cmath>
#include <cstdio>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

int main() {
    try {
        Context ctx;
        const int64_t C = 5, G = 4;
        std::vector<double> hess((size_t)(C * (G - 1)) * 496, 0.0), prior((size_t)(C * G) * 136, 0.0);
        auto at = [](int i, int d) { return (size_t)(i + d * (d + 1) / 2); };
        for (int64_t c = 0; c < C; c++) {
            for (int i = 0; i < 15; i++) prior[(size_t)(c * G) * 136 + at(i, i)] = 1.0;
            for (int64_t k = 0; k < G - 1; k++) {
                double *H = hess.data() + (size_t)(c * (G - 1) + k) * 496;
                for (int i = 0; i < 15; i++) {
                    const double r = (double)(1 + (i + k + c) % 3);
                    H[at(i, i)] = 1.0; H[at(15 + i, 15 + i)] = 1.0; H[at(i, 15 + i)] = -1.0;     // [-I I]^T [-I I]
                    H[at(i, 30)] = -r; H[at(15 + i, 30)] = r;                                    // A^T b
                }
            }
        }
        std::vector<int32_t> status;
        const std::vector<double> delta = chain_solve(ctx, C, G, hess, prior, {}, false, &status);
        int bad = 0;
        for (int64_t c = 0; c < C; c++) {
            if (status[(size_t)c] != 0) { printf("chain %lld: status %d\n", (long long)c, status[(size_t)c]); bad++; }
            for (int i = 0; i < 15; i++) {
                double want = 0.0;
                for (int64_t s = 0; s < G; s++) {
                    const double got = delta[(size_t)((c * G + s) * 15 + i)];
                    if (!(std::fabs(got - want) <= 1e-12)) { printf("chain %lld state %lld entry %d: %.17g, expected %.17g\n", (long long)c, (long long)s, i, got, want); bad++; }
                    if (s < G - 1) want += (double)(1 + (i + s + c) % 3);
                }
            }
        }
        try { chain_solve(ctx, C, G, std::vector<double>(7)); printf("a short hess was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        if (bad) return 1;
        printf("test_chain ok %lld %lld\n", (long long)C, (long long)G);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
