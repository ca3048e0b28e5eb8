// test_marginals.cpp -- GPU: cpi_host::chain_marginals end to end, product only.  The chains of test_chain.cpp, whose inverse is known
// in closed form: every factor is [A1 A2] = [-I, I] and the first state carries the prior Lam = I -- a random walk of unit steps from
// a unit prior, so Sigma[s][s] = (s + 1) I and Sigma[s][s + 1] = (s + 1) I (small integers).  Checks itself.
//   test_marginals
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
                for (int i = 0; i < 15; i++) { H[at(i, i)] = 1.0; H[at(15 + i, 15 + i)] = 1.0; H[at(i, 15 + i)] = -1.0; }   // [-I I]^T [-I I]
            }
        }
        std::vector<int32_t> status;
        std::vector<double> cross;
        const std::vector<double> cov = chain_marginals(ctx, C, G, hess, prior, &cross, &status);
        int bad = 0;
        for (int64_t c = 0; c < C; c++) {
            if (status[(size_t)c] != 0) { printf("chain %lld: status %d\n", (long long)c, status[(size_t)c]); bad++; }
            for (int64_t s = 0; s < G; s++)
                for (int j = 0; j < 15; j++)
                    for (int i = 0; i < 15; i++) {
                        const double want = (i == j) ? (double)(s + 1) : 0.0;
                        if (i <= j) {
                            const double got = cov[(size_t)(c * G + s) * 120 + at(i, j)];
                            if (!(std::fabs(got - want) <= 1e-12)) { printf("chain %lld state %lld cov (%d, %d): %.17g, expected %.17g\n", (long long)c, (long long)s, i, j, got, want); bad++; }
                        }
                        const double x = cross[(size_t)(c * G + s) * 225 + (size_t)(i + 15 * j)];
                        if (!(std::fabs(x - (s < G - 1 ? want : 0.0)) <= 1e-12)) { printf("chain %lld state %lld cross (%d, %d): %.17g\n", (long long)c, (long long)s, i, j, x); bad++; }
                    }
        }
        try { chain_marginals(ctx, C, G, std::vector<double>(7)); printf("a short hess was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        if (bad) return 1;
        printf("test_marginals ok %lld %lld\n", (long long)C, (long long)G);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
