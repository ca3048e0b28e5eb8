// test_streams.cpp -- GPU: many runs (trajectories) through cpi_host::ImuStreamSet, one call for all of them
// (cpi_preintegrate_streams_host).  Prints one line of numbers per window, run by run in update-time order (DT alpha beta q
// J_q J_a J_b H_a H_b [O_a O_b] P) and a COUNT line, for the Python test to compare with Engine.preintegrate_streams.
//   test_streams <runs file> <model> <N>
// runs file: R, then per run "K U", K lines of {t w[3] a[3]}, U lines of {update time, b_w_lin[3], b_a_lin[3], q_k_lin[4]}.
#include <cstdio>
#include <fstream>

#include "../../cpi_amd/csrc/cpi_host.hpp"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    using namespace cpi_host;
    std::ifstream f(argv[1]);
    const int model = atoi(argv[2]);
    const int32_t N = (int32_t)atoi(argv[3]);
    int R = 0;
    f >> R;
    ImuStreamSet set;
    for (int r = 0; r < R; r++) {
        long K = 0, U = 0;
        f >> K >> U;
        ImuStream run;
        for (long k = 0; k < K; k++) {
            double v[7];
            for (double &x : v) f >> x;
            run.push(v[0], Vec3{{v[1], v[2], v[3]}}, Vec3{{v[4], v[5], v[6]}});
        }
        std::vector<double> ut, lin, qk;
        for (long u = 0; u < U; u++) {
            double v[11];
            for (double &x : v) f >> x;
            ut.push_back(v[0]);
            lin.insert(lin.end(), v + 1, v + 7);
            qk.insert(qk.end(), v + 7, v + 11);
        }
        set.add_run(run, ut, lin, qk);
    }
    try {
        Context ctx;
        CpiV1 proto1(0.005, 4e-6, 0.01, 2e-4);      // cpi_compare/launch/synthetic_test.launch:13-17
        CpiV2 proto2(0.005, 4e-6, 0.01, 2e-4);
        CpiBase &proto = model == 2 ? (CpiBase &)proto2 : (CpiBase &)proto1;
        proto.grav = Vec3{{0, 0, 9.8}};
        cpi_params prm = proto.params();
        prm.lanes_per_window = 1;                   // the lane split of the Python side
        std::vector<std::vector<int32_t>> counts;
        const std::vector<std::vector<CpiResult>> res = set.preintegrate(ctx, prm, &counts, N);
        for (const std::vector<CpiResult> &run : res)
            for (const CpiResult &x : run) {
                printf("%.17g", x.DT);
                for (double v : x.alpha_tau) printf(" %.17g", v);
                for (double v : x.beta_tau) printf(" %.17g", v);
                for (double v : x.q_k2tau) printf(" %.17g", v);
                const Mat3 *ms[7] = { &x.J_q, &x.J_a, &x.J_b, &x.H_a, &x.H_b, &x.O_a, &x.O_b };
                for (int m = 0; m < (model == 2 ? 7 : 5); m++) for (double v : *ms[m]) printf(" %.17g", v);
                for (double v : x.P_meas) printf(" %.17g", v);
                printf("\n");
            }
        printf("COUNT");
        for (const std::vector<int32_t> &c : counts) for (int32_t v : c) printf(" %d", v);
        printf("\n");
    } catch (const std::exception &ex) {
        fprintf(stderr, "test_streams: %s\n", ex.what());
        return 1;
    }
    return 0;
}
