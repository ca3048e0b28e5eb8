// test_running.cpp -- GPU: the members after every feed_IMU through cpi_host::CpiBatch::running (cpi_preintegrate_running_host).
// Reads windows of recorded intervals, prints one line of numbers per interval, window by window (DT alpha beta q [J_q J_a J_b
// H_a H_b] P), for the Python test to compare with Engine.preintegrate_running; then flushes the batch and prints each window's
// own members after a FINAL line marker (they must equal the window's last row).
//   test_running <windows file> <model> <imu_avg>
// windows file: W, then per window "n", the line {b_w_lin[3] b_a_lin[3] q_k_lin[4]} and n + 1 knot lines {t w[3] a[3]}.
#include <cstdio>
#include <fstream>
#include <memory>

#include "../../cpi_amd/csrc/cpi_host.hpp"

static void print(const cpi_host::CpiResult &x, int model) {
    printf("%.17g", x.DT);
    for (double v : x.alpha_tau) printf(" %.17g", v);
    for (double v : x.beta_tau) printf(" %.17g", v);
    for (double v : x.q_k2tau) printf(" %.17g", v);
    if (model == 1) {
        const cpi_host::Mat3 *ms[5] = { &x.J_q, &x.J_a, &x.J_b, &x.H_a, &x.H_b };
        for (const cpi_host::Mat3 *m : ms) for (double v : *m) printf(" %.17g", v);
    }
    for (double v : x.P_meas) printf(" %.17g", v);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    using namespace cpi_host;
    std::ifstream f(argv[1]);
    const int model = atoi(argv[2]);
    const bool avg = atoi(argv[3]) != 0;
    int W = 0;
    f >> W;
    std::vector<std::unique_ptr<CpiBase>> wins;
    for (int w = 0; w < W; w++) {
        int n = 0;
        f >> n;
        double l[10];
        for (double &x : l) f >> x;
        std::unique_ptr<CpiBase> c;
        if (model == 2) c.reset(new CpiV2(0.005, 4e-6, 0.01, 2e-4, avg)); else c.reset(new CpiV1(0.005, 4e-6, 0.01, 2e-4, avg));
        c->setLinearizationPoints(Vec3{{l[0], l[1], l[2]}}, Vec3{{l[3], l[4], l[5]}}, Vec4{{l[6], l[7], l[8], l[9]}}, Vec3{{0, 0, 9.8}});
        double p[7] = {0}, k[7];
        for (int s = 0; s <= n; s++) {
            for (double &x : k) f >> x;
            if (s > 0) c->feed_IMU(p[0], k[0], Vec3{{p[1], p[2], p[3]}}, Vec3{{p[4], p[5], p[6]}}, Vec3{{k[1], k[2], k[3]}}, Vec3{{k[4], k[5], k[6]}});
            for (int i = 0; i < 7; i++) p[i] = k[i];
        }
        wins.push_back(std::move(c));
    }
    try {
        Context ctx;
        CpiBatch batch;
        for (auto &c : wins) batch.add(c.get());
        const std::vector<std::vector<CpiResult>> res = batch.running(ctx);
        for (const std::vector<CpiResult> &win : res) {
            printf("ROWS %zu\n", win.size());
            for (const CpiResult &x : win) print(x, model);
        }
        batch.flush(ctx);
        for (auto &c : wins) { printf("FINAL\n"); print(c->result(), model); }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
