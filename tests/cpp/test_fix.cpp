// test_fix.cpp -- GPU: cpi_host::state_fix end to end, product only.  S states with the identity quaternion whose answers are known in
// closed form: state s carries s % 3 position fixes z = p + d with R = diag(1, 2, 3) and d = (m + 1) / 4 in every entry (m the fix's
// number), so Lam += diag(1, 4, 9) on the rows 12 .. 14, eta += diag(1, 4, 9) d and pcost += 0.5 * 14 d^2 per fix, every value
// exact whatever the summation order; then a velocity fix on every state is chained through base / pcost_base.  Checks itself, then
// prints the touched entries of every row and pcost as hexadecimal doubles (one state per line) for the caller to compare with the
// device form's bits.
//   test_fix
#include <cmath>
#include <cstdio>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

int main() {
    try {
        Context ctx;
        const int64_t S = 7;
        auto at = [](int i, int d) { return (size_t)(i + d * (d + 1) / 2); };
        std::vector<double> states((size_t)S * 16, 0.0), z, R, zv, Rv;
        std::vector<int64_t> mfirst((size_t)S + 1, 0), vfirst((size_t)S + 1, 0);
        for (int64_t s = 0; s < S; s++) {
            states[(size_t)s * 16 + 3] = 1.0;                                  // the identity quaternion
            for (int i = 4; i < 16; i++) states[(size_t)s * 16 + i] = (double)(s + i);
            mfirst[(size_t)s + 1] = mfirst[(size_t)s] + s % 3;
            vfirst[(size_t)s + 1] = s + 1;
            for (int64_t k = 0; k < s % 3; k++) {
                const double d = 0.25 * (double)(mfirst[(size_t)s] + k + 1);
                for (int i = 0; i < 3; i++) z.push_back(states[(size_t)s * 16 + 13 + i] + d);
                const double r[6] = {1.0, 0.0, 2.0, 0.0, 0.0, 3.0};
                R.insert(R.end(), r, r + 6);
            }
            for (int i = 0; i < 3; i++) zv.push_back(states[(size_t)s * 16 + 7 + i] - 0.5);
            const double rv[6] = {2.0, 0.0, 2.0, 0.0, 0.0, 2.0};
            Rv.insert(Rv.end(), rv, rv + 6);
        }
        int bad = 0;
        const FixRows pos = state_fix(ctx, CPI_FIX_POSITION, states, z, R, mfirst);
        const FixRows both = state_fix(ctx, CPI_FIX_VELOCITY, states, zv, Rv, vfirst, {}, pos.rows, pos.pcost);
        for (int64_t s = 0; s < S; s++) {
            double lam = 0.0, eta[3] = {0, 0, 0}, pc = 0.0;
            for (int64_t m = mfirst[(size_t)s]; m < mfirst[(size_t)s + 1]; m++) {
                const double d = 0.25 * (double)(m + 1);
                lam += 1.0;
                for (int i = 0; i < 3; i++) eta[i] += (double)((i + 1) * (i + 1)) * d;
                pc += 0.5 * 14.0 * d * d;
                if (pos.chi2[(size_t)m] != 14.0 * d * d) { printf("fix %lld: chi2 %.17g\n", (long long)m, pos.chi2[(size_t)m]); bad++; }
            }
            const double *row = pos.rows.data() + (size_t)s * 136, *row2 = both.rows.data() + (size_t)s * 136;
            for (int i = 0; i < 3; i++) {
                if (row[at(12 + i, 12 + i)] != lam * (double)((i + 1) * (i + 1)) || row[at(12 + i, 15)] != eta[i]) { printf("state %lld row %d: %.17g %.17g\n", (long long)s, i, row[at(12 + i, 12 + i)], row[at(12 + i, 15)]); bad++; }
                if (row2[at(6 + i, 6 + i)] != 4.0 || row2[at(6 + i, 15)] != -2.0 || row2[at(12 + i, 15)] != eta[i]) { printf("state %lld: the chained velocity fix\n", (long long)s); bad++; }
            }
            if (pos.pcost[(size_t)s] != pc || both.pcost[(size_t)s] != pc + 0.5 * 3.0) { printf("state %lld: pcost %.17g %.17g, expected %.17g\n", (long long)s, pos.pcost[(size_t)s], both.pcost[(size_t)s], pc); bad++; }
            double rest = 0.0;
            for (int i = 0; i < 136; i++) rest += std::fabs(row[i]);
            if (s % 3 == 0 && rest != 0.0) { printf("state %lld has no fix and a row that is not zero\n", (long long)s); bad++; }
        }
        try { state_fix(ctx, 7, states, z, R, mfirst); printf("kind 7 was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        try { std::vector<int64_t> wrong(mfirst); wrong[2] = 99; state_fix(ctx, CPI_FIX_POSITION, states, z, R, wrong); printf("a broken mfirst was accepted\n"); bad++; } catch (const std::exception &) {}
        if (bad) { printf("%d checks failed\n", bad); return 1; }
        for (int64_t s = 0; s < S; s++) {
            const double *row = both.rows.data() + (size_t)s * 136;
            for (int i = 0; i < 3; i++) printf("%a %a %a %a ", row[at(6 + i, 6 + i)], row[at(6 + i, 15)], row[at(12 + i, 12 + i)], row[at(12 + i, 15)]);
            printf("%a\n", both.pcost[(size_t)s]);
        }
        printf("test_fix ok %lld %lld\n", (long long)S, (long long)mfirst[(size_t)S]);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
