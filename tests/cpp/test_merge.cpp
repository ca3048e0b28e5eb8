// test_merge.cpp -- GPU: cpi_host::merge (cpi_merge_batch_host) end to end, product only.  An IMU stream is cut at U update times and
// preintegrated by ImuStream::preintegrate with ONE linearisation point for all windows; merge(rows, 5) joins every 5 consecutive
// windows; the result is compared with ImuStream::preintegrate at every 5th update time -- the call merge replaces -- at the
// parity gates (means 1e-9, Jacobians 1e-8, P 1e-6 relative to sqrt(P_ii P_jj)), q after aligning its sign.  Also: the ragged form
// (first / count) against the dense one, count 1 = the row itself, count 0 = the zero state.  Checks itself.
//   test_merge <stream file: K x 7 doubles> <update times file> <imu_avg>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static bool same(const CpiResult &a, const CpiResult &b) {
    return a.DT == b.DT && a.alpha_tau == b.alpha_tau && a.beta_tau == b.beta_tau && a.q_k2tau == b.q_k2tau && a.J_q == b.J_q && a.J_a == b.J_a &&
           a.J_b == b.J_b && a.H_a == b.H_a && a.H_b == b.H_b && a.P_meas == b.P_meas;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<double> knots, ut;
    { std::ifstream g(argv[1]); double v; while (g >> v) knots.push_back(v); }
    { std::ifstream g(argv[2]); double v; while (g >> v) ut.push_back(v); }
    const int G = 5;
    const size_t U = ut.size(), M = U / G;
    if (knots.size() % 7 || U % G || M == 0) return 2;
    try {
        Context ctx;
        CpiV1 proto(0.005, 4e-6, 0.01, 2e-4, atoi(argv[3]) != 0);
        const cpi_params prm = proto.params();
        ImuStream imu;
        imu.assign(knots);
        const double lin1[6] = { 0.01, -0.02, 0.015, 0.1, -0.05, 0.08 };
        std::vector<double> lin, lin5, ut5;
        for (size_t u = 0; u < U; u++) lin.insert(lin.end(), lin1, lin1 + 6);
        for (size_t j = 0; j < M; j++) { lin5.insert(lin5.end(), lin1, lin1 + 6); ut5.push_back(ut[j * G + G - 1]); }
        const std::vector<CpiResult> rows = imu.preintegrate(ctx, prm, ut, lin), want = imu.preintegrate(ctx, prm, ut5, lin5);
        const std::vector<CpiResult> got = merge(ctx, rows, G);
        if (got.size() != M) { printf("merge returned %zu rows, not %zu\n", got.size(), M); return 1; }
        int bad = 0;
        double worst_mean = 0, worst_jac = 0, worst_cov = 0;
        for (size_t j = 0; j < M; j++) {
            const CpiResult &a = got[j], &b = want[j];
            double dotq = 0;
            for (int k = 0; k < 4; k++) dotq += a.q_k2tau[k] * b.q_k2tau[k];
            const double sg = dotq < 0 ? -1.0 : 1.0;
            double em = std::fabs(a.DT - b.DT), ej = 0, ec = 0;
            for (int k = 0; k < 3; k++) em = std::max(em, std::max(std::fabs(a.alpha_tau[k] - b.alpha_tau[k]), std::fabs(a.beta_tau[k] - b.beta_tau[k])));
            for (int k = 0; k < 4; k++) em = std::max(em, std::fabs(sg * a.q_k2tau[k] - b.q_k2tau[k]));
            for (int k = 0; k < 9; k++)
                ej = std::max(ej, std::max(std::max(std::fabs(a.J_q[k] - b.J_q[k]), std::fabs(a.J_a[k] - b.J_a[k])),
                                           std::max(std::fabs(a.J_b[k] - b.J_b[k]), std::max(std::fabs(a.H_a[k] - b.H_a[k]), std::fabs(a.H_b[k] - b.H_b[k])))));
            for (int c = 0; c < 15; c++)
                for (int r = 0; r < 15; r++) {
                    const double den = std::sqrt(b.P_meas[r * 15 + r] * b.P_meas[c * 15 + c]);
                    ec = std::max(ec, std::fabs(a.P_meas[c * 15 + r] - b.P_meas[c * 15 + r]) / den);
                }
            worst_mean = std::max(worst_mean, em); worst_jac = std::max(worst_jac, ej); worst_cov = std::max(worst_cov, ec);
            if (!(em <= 1e-9) || !(ej <= 1e-8) || !(ec <= 1e-6)) { printf("group %zu: mean %.3e jac %.3e cov %.3e\n", j, em, ej, ec); bad++; }
        }
        printf("merge vs preintegrate at every 5th update time: mean %.2e jac %.2e cov %.2e\n", worst_mean, worst_jac, worst_cov);
        // the ragged form: groups listed backwards, then one row, then nothing
        std::vector<int64_t> first;
        std::vector<int32_t> count;
        for (size_t j = 0; j < M; j++) { first.push_back((int64_t)((M - 1 - j) * G)); count.push_back(G); }
        first.push_back(3); count.push_back(1);
        first.push_back(2); count.push_back(0);
        const std::vector<CpiResult> rag = merge(ctx, rows, G, &first, &count);
        for (size_t j = 0; j < M; j++)
            if (!same(rag[j], got[M - 1 - j])) { printf("ragged group %zu differs from the dense one\n", j); bad++; }
        if (!same(rag[M], rows[3])) { printf("count 1 is not the row itself\n"); bad++; }
        if (!same(rag[M + 1], CpiResult())) { printf("count 0 is not the zero state\n"); bad++; }
        if (bad) return 1;
        printf("test_merge ok %zu\n", M);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
