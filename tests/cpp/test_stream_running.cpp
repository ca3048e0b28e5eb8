// test_stream_running.cpp -- GPU: the members after every feed_IMU of every window of IMU stream(s), cut in place, through
// cpi_host::ImuStream::running and ImuStreamSet::running (cpi_preintegrate_stream[s]_running_host).  The reference is the route a
// caller had before: cut every window on the host (cpi_host::assemble_windows), feed it to a CpiV1 / CpiV2 and read
// CpiBatch::running -- same number of windows, same bound, automatic lanes: the results must agree bit for bit, one result per
// interval of a window's count.  Also checked: the counts, the tight default bound, and that a bound smaller than the longest
// window throws.  Prints "OK rows <rows of the multi-run call>".
//   test_stream_running <runs file> <model> <imu_avg>
// runs file: R, then per run "K U", K lines of {t w[3] a[3]} and the U update times.
#include <cstdio>
#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static bool same(const CpiResult &a, const CpiResult &b, int model) {
    bool ok = memcmp(&a.DT, &b.DT, sizeof(double)) == 0 && memcmp(a.alpha_tau.data(), b.alpha_tau.data(), 24) == 0 &&
              memcmp(a.beta_tau.data(), b.beta_tau.data(), 24) == 0 && memcmp(a.q_k2tau.data(), b.q_k2tau.data(), 32) == 0 &&
              memcmp(a.P_meas.data(), b.P_meas.data(), 225 * sizeof(double)) == 0;
    if (model == 1)
        ok = ok && memcmp(a.J_q.data(), b.J_q.data(), 72) == 0 && memcmp(a.J_a.data(), b.J_a.data(), 72) == 0 &&
             memcmp(a.J_b.data(), b.J_b.data(), 72) == 0 && memcmp(a.H_a.data(), b.H_a.data(), 72) == 0 &&
             memcmp(a.H_b.data(), b.H_b.data(), 72) == 0;
    return ok;
}

struct Run {
    ImuStream stream;
    std::vector<double> ut, lin, qk;
};

// the windows of a run as recorded preintegrators (the caller's loop of GraphSolver_IMU.cpp:43-75 on the host)
static void record(const Run &run, int model, bool avg, std::vector<std::unique_ptr<CpiBase>> &wins, std::vector<int32_t> &counts) {
    const WindowSet ws = assemble_windows(run.stream.knots(), run.ut);
    for (size_t u = 0; u < run.ut.size(); u++) {
        std::unique_ptr<CpiBase> c;
        if (model == 2) c.reset(new CpiV2(0.005, 4e-6, 0.01, 2e-4, avg)); else c.reset(new CpiV1(0.005, 4e-6, 0.01, 2e-4, avg));
        const double *l = &run.lin[u * 6], *q = &run.qk[u * 4];
        c->setLinearizationPoints(Vec3{{l[0], l[1], l[2]}}, Vec3{{l[3], l[4], l[5]}}, Vec4{{q[0], q[1], q[2], q[3]}}, Vec3{{0, 0, 9.8}});
        for (int32_t s = 1; s <= ws.count[u]; s++) {
            const double *p = &ws.knots[(ws.first[u] + s - 1) * 7], *k = p + 7;
            c->feed_IMU(p[0], k[0], Vec3{{p[1], p[2], p[3]}}, Vec3{{p[4], p[5], p[6]}}, Vec3{{k[1], k[2], k[3]}}, Vec3{{k[4], k[5], k[6]}});
        }
        counts.push_back(ws.count[u]);
        wins.push_back(std::move(c));
    }
}

static long compare(const std::vector<std::vector<CpiResult>> &got, const std::vector<std::vector<CpiResult>> &ref,
                    const std::vector<int32_t> &counts, int model, const char *what) {
    if (got.size() != ref.size() || got.size() != counts.size()) throw std::runtime_error(std::string(what) + ": number of windows");
    long rows = 0;
    for (size_t w = 0; w < got.size(); w++) {
        if (got[w].size() != (size_t)counts[w] || ref[w].size() != (size_t)counts[w])
            throw std::runtime_error(std::string(what) + ": window " + std::to_string(w) + " does not hold one result per interval");
        for (size_t i = 0; i < got[w].size(); i++, rows++)
            if (!same(got[w][i], ref[w][i], model))
                throw std::runtime_error(std::string(what) + ": window " + std::to_string(w) + " interval " + std::to_string(i) + " differs");
    }
    return rows;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::ifstream f(argv[1]);
    const int model = atoi(argv[2]);
    const bool avg = atoi(argv[3]) != 0;
    int R = 0;
    f >> R;
    std::vector<Run> runs((size_t)R);
    size_t seed = 0;
    for (Run &run : runs) {
        long K = 0, U = 0;
        f >> K >> U;
        for (long k = 0; k < K; k++) {
            double v[7];
            for (double &x : v) f >> x;
            run.stream.push(v[0], Vec3{{v[1], v[2], v[3]}}, Vec3{{v[4], v[5], v[6]}});
        }
        for (long u = 0; u < U; u++, seed++) {
            double t;
            f >> t;
            run.ut.push_back(t);
            for (int i = 0; i < 6; i++) run.lin.push_back((i < 3 ? 0.01 : 0.05) * std::sin(0.7 * (double)seed + i));
            const double a = 0.3 * (double)seed, qx = 0.5 * std::sin(a), qy = 0.2 * std::cos(a), qz = 0.3;
            const double n = std::sqrt(qx * qx + qy * qy + qz * qz + 1.0);
            run.qk.push_back(qx / n); run.qk.push_back(qy / n); run.qk.push_back(qz / n); run.qk.push_back(1.0 / n);
        }
    }
    try {
        Context ctx;
        CpiV1 proto1(0.005, 4e-6, 0.01, 2e-4, avg);
        CpiV2 proto2(0.005, 4e-6, 0.01, 2e-4, avg);
        CpiBase &proto = model == 2 ? (CpiBase &)proto2 : (CpiBase &)proto1;
        proto.grav = Vec3{{0, 0, 9.8}};
        const cpi_params prm = proto.params();
        // ---- every run on its own: ImuStream::running with the default (tight) bound
        for (size_t r = 0; r < runs.size(); r++) {
            const Run &run = runs[r];
            if (run.ut.empty()) continue;
            std::vector<std::unique_ptr<CpiBase>> wins;
            std::vector<int32_t> counts, got_counts;
            record(run, model, avg, wins, counts);
            CpiBatch batch;
            for (auto &c : wins) batch.add(c.get());
            const std::vector<std::vector<CpiResult>> ref = batch.running(ctx);
            const std::vector<std::vector<CpiResult>> got = run.stream.running(ctx, prm, run.ut, run.lin, run.qk, &got_counts);
            if (got_counts != counts) throw std::runtime_error("ImuStream::running: counts of run " + std::to_string(r));
            compare(got, ref, counts, model, "ImuStream::running");
            int32_t longest = 0;
            for (int32_t c : counts) longest = std::max(longest, c);
            if (longest_window(run.stream.knots().data(), run.stream.size(), run.ut.data(), run.ut.size()) != longest)
                throw std::runtime_error("longest_window: not the longest assembled window of run " + std::to_string(r));
            if (longest > 1) {
                bool thrown = false;
                try { run.stream.running(ctx, prm, run.ut, run.lin, run.qk, nullptr, longest - 1); } catch (const std::runtime_error &) { thrown = true; }
                if (!thrown) throw std::runtime_error("ImuStream::running: a bound below the longest window was accepted");
            }
        }
        // ---- all runs in one call: ImuStreamSet::running against ONE batch of every run's windows
        ImuStreamSet set;
        std::vector<std::unique_ptr<CpiBase>> wins;
        std::vector<int32_t> counts;
        for (const Run &run : runs) {
            set.add_run(run.stream, run.ut, run.lin, run.qk);
            record(run, model, avg, wins, counts);
        }
        CpiBatch batch;
        for (auto &c : wins) batch.add(c.get());
        const std::vector<std::vector<CpiResult>> ref = batch.running(ctx);
        std::vector<std::vector<int32_t>> set_counts;
        const std::vector<std::vector<std::vector<CpiResult>>> got = set.running(ctx, prm, &set_counts);
        std::vector<std::vector<CpiResult>> flat;
        std::vector<int32_t> flat_counts;
        if (got.size() != runs.size()) throw std::runtime_error("ImuStreamSet::running: number of runs");
        for (size_t r = 0; r < got.size(); r++) {
            if (got[r].size() != runs[r].ut.size()) throw std::runtime_error("ImuStreamSet::running: windows of run " + std::to_string(r));
            flat.insert(flat.end(), got[r].begin(), got[r].end());
            flat_counts.insert(flat_counts.end(), set_counts[r].begin(), set_counts[r].end());
        }
        if (flat_counts != counts) throw std::runtime_error("ImuStreamSet::running: counts");
        const long rows = compare(flat, ref, counts, model, "ImuStreamSet::running");
        bool thrown = false;
        try { set.running(ctx, prm, nullptr, 2); } catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) throw std::runtime_error("ImuStreamSet::running: a bound below the longest window was accepted");
        printf("OK rows %ld\n", rows);
    } catch (const std::exception &ex) {
        fprintf(stderr, "test_stream_running: %s\n", ex.what());
        return 1;
    }
    return 0;
}
