// tests/test_gpu_resume.py: the C++ facade in incremental mode (CpiBase::set_incremental).  Reads one window of knots,
// feeds it interval by interval and prints every result member after each feed_IMU (one line per read); a copy taken half
// way is fed the rest on its own and printed last (line "COPY ...").  Usage: test_incremental <file> <model>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static void print(const char *tag, const CpiBase &c, int model) {
    const CpiResult r = c.result();
    std::printf("%s %.17g", tag, r.DT);
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
        CpiV1 c1(0.005, 4e-6, 0.01, 2e-4);
        CpiV2 c2(0.005, 4e-6, 0.01, 2e-4);
        CpiBase &cpi = (model == 1) ? (CpiBase &)c1 : (CpiBase &)c2;
        cpi.set_incremental(true);
        cpi.setLinearizationPoints({{l[0], l[1], l[2]}}, {{l[3], l[4], l[5]}}, {{q[0], q[1], q[2], q[3]}}, {{0, 0, 9.8}});
        CpiBase *copy = nullptr;
        CpiV1 k1(c1);
        CpiV2 k2(c2);
        for (int i = 0; i + 1 < n1; i++) {
            const double *a = &k[7 * i], *b = &k[7 * (i + 1)];
            cpi.feed_IMU(a[0], b[0], {{a[1], a[2], a[3]}}, {{a[4], a[5], a[6]}}, {{b[1], b[2], b[3]}}, {{b[4], b[5], b[6]}});
            print("READ", cpi, model);
            if (i + 1 == (n1 - 1) / 2) {
                if (model == 1) { k1 = c1; copy = &k1; } else { k2 = c2; copy = &k2; }
            }
        }
        for (int i = (n1 - 1) / 2; copy && i + 1 < n1; i++) {
            const double *a = &k[7 * i], *b = &k[7 * (i + 1)];
            copy->feed_IMU(a[0], b[0], {{a[1], a[2], a[3]}}, {{a[4], a[5], a[6]}}, {{b[1], b[2], b[3]}}, {{b[4], b[5], b[6]}});
        }
        if (copy) print("COPY", *copy, model);
        bool threw = false;   // the linearisation point is fixed once intervals were integrated
        try { cpi.setLinearizationPoints({{0, 0, 0}}, {{0, 0, 0}}); } catch (const std::logic_error &) { threw = true; }
        CpiBatch batch;
        bool threw_batch = false;
        try { batch.add(&cpi); } catch (const std::logic_error &) { threw_batch = true; }
        ForsterDiscrete fd(0.005, 4e-6, 0.01, 2e-4);
        bool threw_forster = false;
        try { fd.set_incremental(true); } catch (const std::logic_error &) { threw_forster = true; }
        std::printf("GUARDS %d %d %d\n", threw ? 1 : 0, threw_batch ? 1 : 0, threw_forster ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("THROWS %s\n", e.what());
        return 1;
    }
    return 0;
}
