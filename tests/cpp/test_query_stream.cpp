// test_query_stream.cpp -- GPU: the members at absolute times over IMU stream(s) read in place, through cpi_host::ImuStream::at /
// at_cov / at_stj and ImuStreamSet::at_stj (cpi_query_stream_batch_host).  The reference is the route a caller had before: cut every
// window on the host (cpi_host::assemble_windows), find the window of every time on the host, and ask cpi_query_stj_batch_host -- the
// results must agree bit for bit, and the windows must be the ones a lower bound over the update times gives.  Prints
// "test_query_stream ok <queries>".
//   test_query_stream <runs file> <model> <imu_avg>
// runs file: R, then per run "K U", K lines of {t w[3] a[3]} and the U update times.  The times asked of a run: every update time,
// every stamp, the middle of every interval, one before the run, one past its last update time.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static bool same(const CpiResult &a, const CpiResult &b, int model, bool cov, bool jac2) {
    bool ok = memcmp(&a.DT, &b.DT, 8) == 0 && memcmp(a.alpha_tau.data(), b.alpha_tau.data(), 24) == 0 &&
              memcmp(a.beta_tau.data(), b.beta_tau.data(), 24) == 0 && memcmp(a.q_k2tau.data(), b.q_k2tau.data(), 32) == 0;
    if (cov) ok = ok && memcmp(a.P_meas.data(), b.P_meas.data(), 225 * 8) == 0;
    if (model == 1 || jac2)
        ok = ok && memcmp(a.J_q.data(), b.J_q.data(), 72) == 0 && memcmp(a.J_a.data(), b.J_a.data(), 72) == 0 &&
             memcmp(a.J_b.data(), b.J_b.data(), 72) == 0 && memcmp(a.H_a.data(), b.H_a.data(), 72) == 0 && memcmp(a.H_b.data(), b.H_b.data(), 72) == 0;
    if (jac2) ok = ok && memcmp(a.O_a.data(), b.O_a.data(), 72) == 0 && memcmp(a.O_b.data(), b.O_b.data(), 72) == 0;
    return ok;
}

struct Run {
    ImuStream stream;
    std::vector<double> ut, lin, qk, times;
};

// the old route for the times of one run: assembled windows, host lookup, cpi_query_stj_batch_host
static std::vector<CpiResult> reference(const Context &ctx, const cpi_params &prm, const Run &run, int32_t N, std::vector<int32_t> &qwin) {
    const WindowSet ws = assemble_windows(run.stream.knots(), run.ut);
    const int64_t U = (int64_t)run.ut.size(), Q = (int64_t)run.times.size();
    qwin.resize((size_t)Q);
    for (int64_t k = 0; k < Q; k++)
        qwin[k] = (int32_t)std::min<int64_t>(std::lower_bound(run.ut.begin(), run.ut.end(), run.times[k]) - run.ut.begin(), U - 1);
    std::vector<int32_t> count = ws.count;
    for (int32_t &c : count) c = std::min(c, N);
    const bool v2 = prm.model == CPI_MODEL_V2;
    std::vector<double> DT(Q), al(Q * 3), be(Q * 3), q(Q * 4), J[7], P(Q * 225);
    for (auto &j : J) j.resize(Q * 9);
    cpi_outputs o{};
    o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data(); o.P = P.data();
    o.J_q = J[0].data(); o.J_a = J[1].data(); o.J_b = J[2].data(); o.H_a = J[3].data(); o.H_b = J[4].data();
    if (v2) { o.O_a = J[5].data(); o.O_b = J[6].data(); }
    ctx.check(cpi_query_stj_batch_host(ctx.get(), &prm, U, N, ws.knots.data(), ws.first.data(), count.data(), (int64_t)(ws.knots.size() / 7),
                                       run.lin.data(), run.qk.data(), Q, qwin.data(), run.times.data(), &o));
    std::vector<CpiResult> res((size_t)Q);
    for (size_t r = 0; r < (size_t)Q; r++) {
        CpiResult &x = res[r];
        x.DT = DT[r];
        for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
        for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
        for (int k = 0; k < 9; k++) {
            x.J_q[k] = J[0][r * 9 + k]; x.J_a[k] = J[1][r * 9 + k]; x.J_b[k] = J[2][r * 9 + k]; x.H_a[k] = J[3][r * 9 + k]; x.H_b[k] = J[4][r * 9 + k];
            if (v2) { x.O_a[k] = J[5][r * 9 + k]; x.O_b[k] = J[6][r * 9 + k]; }
        }
        for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
    }
    return res;
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
        std::vector<double> t;
        for (long k = 0; k < K; k++) {
            double v[7];
            for (double &x : v) f >> x;
            run.stream.push(v[0], Vec3{{v[1], v[2], v[3]}}, Vec3{{v[4], v[5], v[6]}});
            t.push_back(v[0]);
        }
        for (long u = 0; u < U; u++, seed++) {
            double T;
            f >> T;
            run.ut.push_back(T);
            for (int i = 0; i < 6; i++) run.lin.push_back((i < 3 ? 0.01 : 0.05) * std::sin(0.7 * (double)seed + i));
            const double a = 0.3 * (double)seed, qx = 0.5 * std::sin(a), qy = 0.2 * std::cos(a), qz = 0.3;
            const double n = std::sqrt(qx * qx + qy * qy + qz * qz + 1.0);
            run.qk.push_back(qx / n); run.qk.push_back(qy / n); run.qk.push_back(qz / n); run.qk.push_back(1.0 / n);
        }
        run.times = run.ut;
        run.times.insert(run.times.end(), t.begin(), t.end());
        for (size_t k = 0; k + 1 < t.size(); k++) run.times.push_back(0.5 * (t[k] + t[k + 1]));
        run.times.push_back(t.front() - 1.0);
        run.times.push_back(run.ut.back() + 1.0);
    }
    try {
        Context ctx;
        CpiV1 proto1(0.005, 4e-6, 0.01, 2e-4, avg);
        CpiV2 proto2(0.005, 4e-6, 0.01, 2e-4, avg);
        CpiBase &proto = model == 2 ? (CpiBase &)proto2 : (CpiBase &)proto1;
        proto.grav = Vec3{{0, 0, 9.8}};
        const cpi_params prm = proto.params();
        long queries = 0;
        ImuStreamSet set;
        std::vector<int32_t> set_runs, set_win;
        std::vector<double> set_times;
        std::vector<CpiResult> set_ref;
        int32_t Nmax = 0;
        int64_t base = 0;
        for (const Run &run : runs)
            Nmax = std::max(Nmax, longest_window(run.stream.knots().data(), run.stream.size(), run.ut.data(), run.ut.size()));
        for (size_t r = 0; r < runs.size(); r++) {
            const Run &run = runs[r];
            const int32_t N = longest_window(run.stream.knots().data(), run.stream.size(), run.ut.data(), run.ut.size());
            std::vector<int32_t> qwin, got_win;
            const std::vector<CpiResult> ref = reference(ctx, prm, run, N, qwin);
            const std::vector<CpiResult> got = run.stream.at_stj(ctx, prm, run.ut, run.lin, run.times, run.qk, &got_win);
            if (got_win != qwin) throw std::runtime_error("ImuStream::at_stj: windows of run " + std::to_string(r));
            const std::vector<CpiResult> got_cov = run.stream.at_cov(ctx, prm, run.ut, run.lin, run.times, run.qk);
            const std::vector<CpiResult> got_mean = run.stream.at(ctx, prm, run.ut, run.lin, run.times, run.qk);
            for (size_t k = 0; k < ref.size(); k++, queries++)
                if (!same(got[k], ref[k], model, true, model == 2) || !same(got_cov[k], ref[k], model, true, false) ||
                    !same(got_mean[k], ref[k], model, false, false))
                    throw std::runtime_error("ImuStream::at*: run " + std::to_string(r) + " time " + std::to_string(k) + " differs");
            // the set is compared at ITS bound: the longest window of any run
            std::vector<int32_t> w2;
            const std::vector<CpiResult> ref2 = reference(ctx, prm, run, Nmax, w2);
            set.add_run(run.stream, run.ut, run.lin, run.qk);
            set_runs.insert(set_runs.end(), run.times.size(), (int32_t)r);
            set_times.insert(set_times.end(), run.times.begin(), run.times.end());
            set_ref.insert(set_ref.end(), ref2.begin(), ref2.end());
            for (int32_t w : w2) set_win.push_back((int32_t)(base + w));
            base += (int64_t)run.ut.size();
        }
        std::vector<int32_t> got_win;
        const std::vector<CpiResult> got = set.at_stj(ctx, prm, set_runs, set_times, &got_win);
        if (got_win != set_win) throw std::runtime_error("ImuStreamSet::at_stj: windows");
        for (size_t k = 0; k < set_ref.size(); k++)
            if (!same(got[k], set_ref[k], model, true, model == 2)) throw std::runtime_error("ImuStreamSet::at_stj: time " + std::to_string(k) + " differs");
        bool thrown = false;
        try { set.at(ctx, prm, std::vector<int32_t>{(int32_t)runs.size()}, std::vector<double>{0.0}); } catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) throw std::runtime_error("ImuStreamSet::at: a run index outside the set was accepted");
        printf("test_query_stream ok %ld\n", queries);
    } catch (const std::exception &ex) {
        fprintf(stderr, "test_query_stream: %s\n", ex.what());
        return 1;
    }
    return 0;
}
