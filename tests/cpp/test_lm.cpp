// test_lm.cpp -- GPU: cpi_host::prior_relinearize, chain_cost and chain_accept end to end, product only.  C chains of G states whose
// answers are known in closed form: every chain's first state carries a Gaussian prior Lam = diag(1 .. 15), eta0 = 0, centred on an
// anchor that differs from the state by d in the additive entries (and has the state's quaternion), so xi = [0 0 0, d], eta = Lam xi
// and pcost = 0.5 sum Lam_ii xi_i^2; chi2 are small integers, so every cost is exact whatever the summation order.  Even chains get a
// trial that is cheaper and are accepted, odd ones a dearer one and are rejected.  Checks itself, then prints eta, pcost, the costs
// and the state after the decision as hexadecimal doubles (one chain per line) for the caller to compare with the device forms' bits.
//   test_lm
#include <cmath>
#include <cstdio>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

int main() {
    try {
        Context ctx;
        const int64_t C = 5, G = 4, S = C * G, F = C * (G - 1);
        auto at = [](int i, int d) { return (size_t)(i + d * (d + 1) / 2); };
        std::vector<double> states((size_t)S * 16, 0.0), anchor((size_t)C * 16, 0.0), prior0((size_t)C * 136, 0.0), chi2((size_t)F), chi2_new((size_t)F);
        std::vector<int32_t> idx((size_t)C);
        for (int64_t s = 0; s < S; s++) {
            states[(size_t)s * 16 + 3] = 1.0;                                  // the identity quaternion
            for (int i = 4; i < 16; i++) states[(size_t)s * 16 + i] = (double)(s + i);
        }
        for (int64_t c = 0; c < C; c++) {
            idx[(size_t)c] = (int32_t)(c * G);
            for (int i = 0; i < 16; i++) anchor[(size_t)c * 16 + i] = states[(size_t)(c * G) * 16 + i];
            for (int i = 4; i < 16; i++) anchor[(size_t)c * 16 + i] += 0.25 * (double)(c + 1);   // d = (c + 1) / 4 in every additive entry
            for (int i = 0; i < 15; i++) prior0[(size_t)c * 136 + at(i, i)] = (double)(i + 1);
            for (int64_t k = 0; k < G - 1; k++) {
                chi2[(size_t)(c * (G - 1) + k)] = (double)(2 * (k + 1 + c));
                chi2_new[(size_t)(c * (G - 1) + k)] = (double)(2 * (k + 1 + c)) + ((c % 2) ? 4.0 : -2.0);
            }
        }
        int bad = 0;
        const PriorRows pr = prior_relinearize(ctx, states, anchor, prior0, idx);
        const std::vector<double> cost = chain_cost(ctx, C, G, chi2, pr.pcost), cost_new = chain_cost(ctx, C, G, chi2_new, pr.pcost);
        for (int64_t c = 0; c < C; c++) {
            const double d = 0.25 * (double)(c + 1);
            double want_p = 0.0, want_c = 0.0;
            for (int i = 3; i < 15; i++) want_p += 0.5 * (double)(i + 1) * d * d;
            for (int64_t k = 0; k < G - 1; k++) want_c += (double)(k + 1 + c);
            const double *row = pr.prior.data() + (size_t)(c * G) * 136;
            for (int i = 0; i < 15; i++) {
                const double want = (i < 3) ? 0.0 : (double)(i + 1) * d;
                if (row[at(i, 15)] != want || row[at(i, i)] != (double)(i + 1)) { printf("chain %lld row %d: eta %.17g, expected %.17g\n", (long long)c, i, row[at(i, 15)], want); bad++; }
            }
            if (pr.pcost[(size_t)(c * G)] != want_p) { printf("chain %lld: pcost %.17g, expected %.17g\n", (long long)c, pr.pcost[(size_t)(c * G)], want_p); bad++; }
            if (cost[(size_t)c] != want_c + want_p) { printf("chain %lld: cost %.17g, expected %.17g\n", (long long)c, cost[(size_t)c], want_c + want_p); bad++; }
            for (int64_t s = 1; s < G; s++)
                if (pr.pcost[(size_t)(c * G + s)] != 0.0 || pr.prior[(size_t)(c * G + s) * 136] != 0.0) { printf("a row without a record was written\n"); bad++; }
        }
        LmState st;
        st.cost = cost; st.states = states; st.chi2 = chi2; st.lambda.assign((size_t)C, 1.0); st.phase.assign((size_t)C, CPI_LM_RUNNING);
        std::vector<double> trial(states);
        for (auto &v : trial) v += 0.5;
        const std::vector<int32_t> acc = chain_accept(ctx, C, G, chi2_new, pr.pcost, trial, st);
        for (int64_t c = 0; c < C; c++) {
            const bool up = (c % 2) == 0;
            if (acc[(size_t)c] != (up ? 1 : 0) || st.lambda[(size_t)c] != (up ? 0.1 : 10.0) || st.phase[(size_t)c] != CPI_LM_RUNNING ||
                st.cost[(size_t)c] != (up ? cost_new[(size_t)c] : cost[(size_t)c])) {
                printf("chain %lld: accepted %d lambda %.17g phase %d cost %.17g\n", (long long)c, acc[(size_t)c], st.lambda[(size_t)c], st.phase[(size_t)c], st.cost[(size_t)c]);
                bad++;
            }
            for (int64_t s = c * G; s < (c + 1) * G; s++)
                for (int i = 0; i < 16; i++)
                    if (st.states[(size_t)s * 16 + i] != (up ? trial : states)[(size_t)s * 16 + i]) bad++;
            for (int64_t k = c * (G - 1); k < (c + 1) * (G - 1); k++)
                if (st.chi2[(size_t)k] != (up ? chi2_new : chi2)[(size_t)k]) bad++;
        }
        try { chain_cost(ctx, C, G, std::vector<double>(7)); printf("a short chi2 was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        cpi_lm_params wrong = {2.0, 10.0, 0.0, 1e5, 1e-5, 1e-5};
        try { LmState s2 = st; chain_accept(ctx, C, G, chi2_new, pr.pcost, trial, s2, &wrong); printf("lam_down = 2 was accepted\n"); bad++; } catch (const std::exception &) {}
        if (bad) { printf("%d checks failed\n", bad); return 1; }
        for (int64_t c = 0; c < C; c++) {
            for (int i = 0; i < 15; i++) printf("%a ", pr.prior[(size_t)(c * G) * 136 + at(i, 15)]);
            printf("%a %a %a %a\n", pr.pcost[(size_t)(c * G)], cost[(size_t)c], cost_new[(size_t)c], st.cost[(size_t)c]);
        }
        printf("test_lm ok %lld %lld\n", (long long)C, (long long)G);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
