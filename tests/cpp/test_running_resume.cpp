// tests/test_gpu_running_resume.py: cpi_host::CpiBase::read_rows on an incremental preintegrator.  Reads one window of knots,
// feeds it in reads of 1, 3, 7, 1, 3, 7, ... intervals and prints every entry read_rows returns (one line "ROW ..." per fed
// interval: DT alpha beta q [J_q J_a J_b H_a H_b, model 1] P); after every read the result members must equal the last entry.
// Usage: test_running_resume <file> <model>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static void print(const CpiResult &r, int model) {
    std::printf("ROW %.17g", r.DT);
    for (double x : r.alpha_tau) std::printf(" %.17g", x);
    for (double x : r.beta_tau) std::printf(" %.17g", x);
    for (double x : r.q_k2tau) std::printf(" %.17g", x);
    if (model == 1)
        for (const Mat3 *m : { &r.J_q, &r.J_a, &r.J_b, &r.H_a, &r.H_b })
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
        Context ctx;
        CpiV1 c1(0.005, 4e-6, 0.01, 2e-4);
        CpiV2 c2(0.005, 4e-6, 0.01, 2e-4);
        CpiBase &cpi = (model == 1) ? (CpiBase &)c1 : (CpiBase &)c2;
        cpi.bind(ctx);
        cpi.set_incremental(true);
        cpi.setLinearizationPoints({{l[0], l[1], l[2]}}, {{l[3], l[4], l[5]}}, {{q[0], q[1], q[2], q[3]}}, {{0, 0, 9.8}});
        if (!cpi.read_rows(ctx).empty()) return 3;
        static const int sizes[3] = { 1, 3, 7 };
        int i = 0, turn = 0;
        bool members = true;
        while (i + 1 < n1) {
            int size = sizes[turn++ % 3];
            if (size > n1 - 1 - i) size = n1 - 1 - i;
            for (int s = 0; s < size; s++, i++) {
                const double *a = &k[7 * i], *b = &k[7 * (i + 1)];
                cpi.feed_IMU(a[0], b[0], {{a[1], a[2], a[3]}}, {{a[4], a[5], a[6]}}, {{b[1], b[2], b[3]}}, {{b[4], b[5], b[6]}});
            }
            const std::vector<CpiResult> rows = cpi.read_rows(ctx);
            if ((int)rows.size() != size) return 3;
            for (const CpiResult &r : rows) print(r, model);
            const CpiResult m = cpi.result();
            members = members && m.DT == rows.back().DT && m.alpha_tau == rows.back().alpha_tau && m.beta_tau == rows.back().beta_tau &&
                      m.P_meas == rows.back().P_meas;
        }
        CpiV1 plain(0.005, 4e-6, 0.01, 2e-4);
        bool threw = false;   // rows continue from a carried state: incremental preintegrators only
        try { plain.read_rows(ctx); } catch (const std::logic_error &) { threw = true; }
        std::printf("GUARDS %d %d\n", threw ? 1 : 0, members ? 1 : 0);
    } catch (const std::exception &e) {
        std::printf("THROWS %s\n", e.what());
        return 1;
    }
    return 0;
}
