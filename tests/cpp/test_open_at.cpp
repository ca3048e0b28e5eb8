// tests/test_gpu_open_facades.py: cpi_host::CpiBase::at on an incremental preintegrator.  Reads one window of knots, feeds it in reads
// of 3, 5, 4, 3, 5, 4, ... intervals and asks at every read for the state before the chunk, on its first stamp, 0.4 into every one of
// its intervals and on its last stamp; prints one line "AT <time> ..." per result (DT alpha beta q J_q J_a J_b H_a H_b [O_a O_b,
// model 2] P).  The program checks itself where it can: the time before the chunk gives the members as they stood before the read,
// the time on the last stamp the members after it, bit for bit.
// Usage: test_open_at <file> <model>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static void print(double t, const CpiResult &r, int model) {
    std::printf("AT %.17g %.17g", t, r.DT);
    for (double x : r.alpha_tau) std::printf(" %.17g", x);
    for (double x : r.beta_tau) std::printf(" %.17g", x);
    for (double x : r.q_k2tau) std::printf(" %.17g", x);
    for (const Mat3 *m : { &r.J_q, &r.J_a, &r.J_b, &r.H_a, &r.H_b })
        for (double x : *m) std::printf(" %.17g", x);
    if (model == 2)
        for (const Mat3 *m : { &r.O_a, &r.O_b })
            for (double x : *m) std::printf(" %.17g", x);
    for (double x : r.P_meas) std::printf(" %.17g", x);
    std::printf("\n");
}

static bool same(const CpiResult &a, const CpiResult &b, int model) {
    bool ok = std::memcmp(&a.DT, &b.DT, sizeof(double)) == 0 && a.alpha_tau == b.alpha_tau && a.beta_tau == b.beta_tau && a.q_k2tau == b.q_k2tau &&
              a.J_q == b.J_q && a.J_a == b.J_a && a.J_b == b.J_b && a.H_a == b.H_a && a.H_b == b.H_b && a.P_meas == b.P_meas;
    if (model == 2) ok = ok && a.O_a == b.O_a && a.O_b == b.O_b;
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int model = std::atoi(argv[2]);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double hdr[1];
    if (std::fread(hdr, sizeof(double), 1, f) != 1) return 2;
    const int n1 = (int)hdr[0];
    std::vector<double> k(n1 * 7), l(6), q(4);
    if (std::fread(k.data(), sizeof(double), k.size(), f) != k.size() || std::fread(l.data(), sizeof(double), 6, f) != 6 ||
        std::fread(q.data(), sizeof(double), 4, f) != 4)
        return 2;
    std::fclose(f);
    try {
        Context ctx;
        CpiV1 c1(0.005, 4e-6, 0.01, 2e-4);
        CpiV2 c2(0.005, 4e-6, 0.01, 2e-4);
        CpiBase &cpi = (model == 1) ? (CpiBase &)c1 : (CpiBase &)c2;
        cpi.bind(ctx);
        cpi.set_incremental(true);
        cpi.setLinearizationPoints({{l[0], l[1], l[2]}}, {{l[3], l[4], l[5]}}, {{q[0], q[1], q[2], q[3]}}, {{0, 0, 9.8}});
        if (!cpi.at(ctx, {}).empty()) return 3;
        static const int sizes[3] = { 3, 5, 4 };
        int i = 0, turn = 0;
        while (i + 1 < n1) {
            int size = sizes[turn++ % 3];
            if (size > n1 - 1 - i) size = n1 - 1 - i;
            const CpiResult before = cpi.result();        // (a member read: a zero-interval resume from the carried state)
            std::vector<double> times = { k[7 * i] - 0.001, k[7 * i] };
            for (int s = 0; s < size; s++, i++) {
                const double *a = &k[7 * i], *b = &k[7 * (i + 1)];
                cpi.feed_IMU(a[0], b[0], {{a[1], a[2], a[3]}}, {{a[4], a[5], a[6]}}, {{b[1], b[2], b[3]}}, {{b[4], b[5], b[6]}});
                times.push_back(a[0] + 0.4 * (b[0] - a[0]));
            }
            times.push_back(k[7 * i]);
            const std::vector<CpiResult> res = cpi.at(ctx, times);
            if (res.size() != times.size()) return 3;
            for (size_t r = 0; r < res.size(); r++) print(times[r], res[r], model);
            if (!same(res[0], before, model) || !same(res[1], before, model)) { std::fprintf(stderr, "the state before the chunk differs from the members\n"); return 4; }
            const CpiResult after = cpi.result();
            if (!same(res.back(), after, model)) { std::fprintf(stderr, "the state on the last stamp differs from the members\n"); return 4; }
        }
        std::printf("test_open_at ok\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
