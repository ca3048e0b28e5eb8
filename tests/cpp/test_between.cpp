// test_between.cpp -- GPU: cpi_host::state_between against the C-ABI (cpi_state_between_batch_host), bit for bit, product only.  F
// factors over a chain of F + 1 states whose quaternions are (0.6, 0, 0, 0.8), (0, 0.6, 0, 0.8), (0, 0, 0.6, 0.8) in turn; factor f
// carries f % 3 pose measurements with a triangular R, a weight of 0.5 + m / 4, on a base row and base chi2 of small integers.  The
// facade, the C-ABI out of place and the C-ABI in place must agree bit for bit, a second kind is chained through hess_base, and the
// program prints chi2 and the 91 touched entries of every row of the first call as hexadecimal doubles (one factor per line) for the
// caller to compare with the device form's bits.
//   test_between
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

int main() {
    try {
        Context ctx;
        const int64_t F = 7, S = F + 1;
        std::vector<double> states((size_t)S * 16, 0.0), z, R, w, base((size_t)F * 496), cb((size_t)F);
        std::vector<int64_t> mfirst((size_t)F + 1, 0);
        for (int64_t s = 0; s < S; s++) {
            states[(size_t)s * 16 + (size_t)(s % 3)] = 0.6;
            states[(size_t)s * 16 + 3] = 0.8;
            for (int i = 4; i < 16; i++) states[(size_t)s * 16 + i] = 0.25 * (double)((s * 7 + i * 3) % 11) - 1.0;
        }
        for (size_t i = 0; i < base.size(); i++) base[i] = (double)((i * 13) % 17) - 8.0;
        for (int64_t f = 0; f < F; f++) {
            cb[(size_t)f] = (double)(f + 1);
            mfirst[(size_t)f + 1] = mfirst[(size_t)f] + f % 3;
            for (int64_t k = 0; k < f % 3; k++) {
                const int64_t m = mfirst[(size_t)f] + k;
                const double zq[7] = {0.0, 0.28, 0.0, 0.96, 0.5 * (double)(m + 1), -0.25, 0.125 * (double)m};
                z.insert(z.end(), zq, zq + 7);
                for (int c = 0; c < 6; c++)
                    for (int r = 0; r <= c; r++) R.push_back(r == c ? 2.0 + c : 0.25 * (double)((r + c + m) % 3));
                w.push_back(0.5 + 0.25 * (double)m);
            }
        }
        const int64_t M = mfirst[(size_t)F];
        int bad = 0;
        const BetweenRows got = state_between(ctx, CPI_BETWEEN_POSE, states, z, R, mfirst, {}, {}, w, base, cb);
        std::vector<double> rows((size_t)F * 496, -7.0), chi2((size_t)F, -7.0), chi2_m((size_t)M, -7.0);
        ctx.check(cpi_state_between_batch_host(ctx.get(), F, M, CPI_BETWEEN_POSE, mfirst.data(), states.data(), S, nullptr, nullptr, z.data(), R.data(), w.data(),
                                               base.data(), cb.data(), rows.data(), chi2.data(), chi2_m.data()));
        if (memcmp(rows.data(), got.rows.data(), rows.size() * 8) || memcmp(chi2.data(), got.chi2.data(), chi2.size() * 8) ||
            memcmp(chi2_m.data(), got.chi2_m.data(), chi2_m.size() * 8)) { printf("the facade differs from the C-ABI\n"); bad++; }
        std::vector<double> in(base), cin(cb);                                 // in place
        ctx.check(cpi_state_between_batch_host(ctx.get(), F, M, CPI_BETWEEN_POSE, mfirst.data(), states.data(), S, nullptr, nullptr, z.data(), R.data(), w.data(),
                                               in.data(), cin.data(), in.data(), cin.data(), nullptr));
        if (memcmp(in.data(), rows.data(), rows.size() * 8) || memcmp(cin.data(), chi2.data(), chi2.size() * 8)) { printf("in place differs from out of place\n"); bad++; }
        for (int64_t f = 0; f < F; f++)
            if (f % 3 == 0 && (memcmp(rows.data() + f * 496, base.data() + f * 496, 496 * 8) || chi2[(size_t)f] != cb[(size_t)f])) { printf("factor %lld has no measurement and changed\n", (long long)f); bad++; }
        // a second kind chained through hess_base / chi2_base, explicit indices equal to the chain
        std::vector<int32_t> ii, jj;
        std::vector<double> zp, Rp;
        std::vector<int64_t> pfirst((size_t)F + 1, 0);
        for (int64_t f = 0; f < F; f++) {
            ii.push_back((int32_t)f); jj.push_back((int32_t)f + 1);
            pfirst[(size_t)f + 1] = f + 1;
            const double p[3] = {0.5, -0.5, 0.25 * (double)f}, r[6] = {2.0, 0.0, 2.0, 0.0, 0.0, 2.0};
            zp.insert(zp.end(), p, p + 3);
            Rp.insert(Rp.end(), r, r + 6);
        }
        const BetweenRows both = state_between(ctx, CPI_BETWEEN_POSITION, states, zp, Rp, pfirst, ii, jj, {}, got.rows, got.chi2);
        const BetweenRows chained = state_between(ctx, CPI_BETWEEN_POSITION, states, zp, Rp, pfirst, {}, {}, {}, got.rows, got.chi2);
        if (memcmp(both.rows.data(), chained.rows.data(), rows.size() * 8) || memcmp(both.chi2.data(), chained.chi2.data(), chi2.size() * 8)) { printf("explicit indices differ from the chain\n"); bad++; }
        for (int64_t f = 0; f < F; f++)
            if (!(both.chi2[(size_t)f] > got.chi2[(size_t)f])) { printf("factor %lld: the second kind added no cost\n", (long long)f); bad++; }
        try { state_between(ctx, 5, states, z, R, mfirst); printf("kind 5 was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        try { std::vector<int64_t> wrong(mfirst); wrong[2] = 99; state_between(ctx, CPI_BETWEEN_POSE, states, z, R, wrong); printf("a broken mfirst was accepted\n"); bad++; } catch (const std::exception &) {}
        try { std::vector<int32_t> wrong(ii); wrong[3] = 99; state_between(ctx, CPI_BETWEEN_POSITION, states, zp, Rp, pfirst, wrong, jj); printf("a broken index was accepted\n"); bad++; } catch (const std::exception &) {}
        if (bad) { printf("%d checks failed\n", bad); return 1; }
        static const int col[13] = {0, 1, 2, 12, 13, 14, 15, 16, 17, 27, 28, 29, 30};
        for (int64_t f = 0; f < F; f++) {
            printf("%a", got.chi2[(size_t)f]);
            for (int b = 0; b < 13; b++)
                for (int a = 0; a <= b; a++) printf(" %a", got.rows[(size_t)f * 496 + (size_t)(col[a] + col[b] * (col[b] + 1) / 2)]);
            printf("\n");
        }
        printf("test_between ok %lld %lld\n", (long long)F, (long long)M);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
