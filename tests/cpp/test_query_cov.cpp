// test_query_cov.cpp -- GPU: the members of a window at arbitrary times WITH P_meas through cpi_host::CpiBatch::at_cov
// (cpi_query_cov_batch_host).  Reads windows of recorded intervals and queries every window before its first stamp, on every knot
// stamp, 0.37 into every interval and past its last stamp, in shuffled order.  Checks itself and prints "test_query_cov ok":
//   - P_meas at a time on knot stamp i >= 1 (and at / past the last stamp) is running()[w][i - 1].P_meas on its upper triangle bit
//     for bit (the host form keeps the covariance rows as the packed upper triangle and mirrors it), at a time <= t_0 all zero;
//   - P_meas at a time inside interval i agrees with a window of its own -- the intervals 0 .. i - 1 and the tail feed_IMU(t_i, t_q,
//     w_i, a_i, w_i, a_i) -- flushed through CpiBatch, within 1e-6 relative to sqrt(P_ii P_jj) (the contractual covariance gate);
//   - the other members are those of at(), bit for bit, and at() leaves P_meas at zero.
//   test_query_cov <windows file> <model> <imu_avg>
// windows file: W, then per window "n", the line {b_w_lin[3] b_a_lin[3] q_k_lin[4]} and n + 1 knot lines {t w[3] a[3]}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

struct Win {
    double l[10];
    std::vector<std::array<double, 7>> k;
};

static std::unique_ptr<CpiBase> make(const Win &w, int model, bool avg) {
    std::unique_ptr<CpiBase> c;
    if (model == 2) c.reset(new CpiV2(0.005, 4e-6, 0.01, 2e-4, avg)); else c.reset(new CpiV1(0.005, 4e-6, 0.01, 2e-4, avg));
    c->setLinearizationPoints(Vec3{{w.l[0], w.l[1], w.l[2]}}, Vec3{{w.l[3], w.l[4], w.l[5]}}, Vec4{{w.l[6], w.l[7], w.l[8], w.l[9]}}, Vec3{{0, 0, 9.8}});
    return c;
}
static void feed(CpiBase &c, const std::array<double, 7> &p, const std::array<double, 7> &k) {
    c.feed_IMU(p[0], k[0], Vec3{{p[1], p[2], p[3]}}, Vec3{{p[4], p[5], p[6]}}, Vec3{{k[1], k[2], k[3]}}, Vec3{{k[4], k[5], k[6]}});
}
template <class A>
static bool same_bits(const A &a, const A &b) { return std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0; }
static bool same_means(const CpiResult &a, const CpiResult &b) {
    return std::memcmp(&a.DT, &b.DT, sizeof(double)) == 0 && same_bits(a.alpha_tau, b.alpha_tau) && same_bits(a.beta_tau, b.beta_tau) &&
           same_bits(a.q_k2tau, b.q_k2tau) && same_bits(a.J_q, b.J_q) && same_bits(a.J_a, b.J_a) && same_bits(a.J_b, b.J_b) &&
           same_bits(a.H_a, b.H_a) && same_bits(a.H_b, b.H_b);
}
// entry (r, c) of a column-major 15 x 15 matrix
static double at(const Mat15 &P, int r, int c) { return P[c * 15 + r]; }

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::ifstream f(argv[1]);
    const int model = atoi(argv[2]);
    const bool avg = atoi(argv[3]) != 0;
    int W = 0;
    f >> W;
    std::vector<Win> wins(W);
    for (Win &w : wins) {
        int n = 0;
        f >> n;
        for (double &x : w.l) f >> x;
        w.k.resize(n + 1);
        for (auto &k : w.k) for (double &x : k) f >> x;
    }
    try {
        Context ctx;
        std::vector<std::unique_ptr<CpiBase>> cs;
        CpiBatch batch;
        // per query: the knot index it sits on (-1: before the window; n: past its end) and whether it lies inside interval i
        struct Qry { int i; bool inside; };
        std::vector<std::vector<double>> times(W);
        std::vector<std::vector<Qry>> what(W);
        for (int w = 0; w < W; w++) {
            const Win &win = wins[w];
            const int n = (int)win.k.size() - 1;
            cs.push_back(make(win, model, avg));
            for (int s = 1; s <= n; s++) feed(*cs.back(), win.k[s - 1], win.k[s]);
            batch.add(cs.back().get());
            std::vector<double> &t = times[w];
            std::vector<Qry> &q = what[w];
            t.push_back(win.k[0][0] - 1.0); q.push_back({-1, false});
            t.push_back(win.k[n][0] + 1.0); q.push_back({n, false});
            for (int s = 0; s <= n; s++) { t.push_back(win.k[s][0]); q.push_back({s, false}); }
            for (int s = 0; s < n; s++) { t.push_back(win.k[s][0] + 0.37 * (win.k[s + 1][0] - win.k[s][0])); q.push_back({s, true}); }
            for (size_t a = 0; a < t.size(); a++) {   // a fixed shuffle: the order of the queries is free
                const size_t b = (a * 7 + 3) % t.size();
                std::swap(t[a], t[b]); std::swap(q[a], q[b]);
            }
        }
        const std::vector<std::vector<CpiResult>> got = batch.at_cov(ctx, times);
        const std::vector<std::vector<CpiResult>> plain = batch.at(ctx, times);
        const std::vector<std::vector<CpiResult>> rows = batch.running(ctx);
        // the windows the inside queries stand for, all in one batch
        std::vector<std::unique_ptr<CpiBase>> refs;
        CpiBatch rb;
        for (int w = 0; w < W; w++)
            for (size_t a = 0; a < times[w].size(); a++) {
                const Qry q = what[w][a];
                if (!q.inside) continue;
                const Win &win = wins[w];
                refs.push_back(make(win, model, avg));
                for (int s = 1; s <= q.i; s++) feed(*refs.back(), win.k[s - 1], win.k[s]);
                std::array<double, 7> tail = win.k[q.i];
                tail[0] = times[w][a];
                feed(*refs.back(), win.k[q.i], tail);
                rb.add(refs.back().get());
            }
        rb.flush(ctx);
        size_t r = 0, copies = 0;
        double ep = 0;
        for (int w = 0; w < W; w++) {
            const int n = (int)wins[w].k.size() - 1;
            if (got[w].size() != times[w].size() || plain[w].size() != times[w].size() || (int)rows[w].size() != n) { fprintf(stderr, "window %d: sizes\n", w); return 1; }
            for (size_t a = 0; a < times[w].size(); a++) {
                const Qry q = what[w][a];
                const CpiResult &x = got[w][a];
                if (!same_means(x, plain[w][a])) { fprintf(stderr, "window %d, query %zu: at_cov's means are not at()'s\n", w, a); return 1; }
                for (double v : plain[w][a].P_meas) if (v != 0) { fprintf(stderr, "at() wrote P_meas\n"); return 1; }
                if (!q.inside) {
                    for (int c = 0; c < 15; c++)
                        for (int i = 0; i < 15; i++) {
                            const double want = q.i <= 0 ? 0.0 : at(rows[w][q.i - 1].P_meas, std::min(i, c), std::max(i, c));
                            const double have = at(x.P_meas, i, c);
                            if (std::memcmp(&want, &have, sizeof(double)) != 0) {
                                fprintf(stderr, "window %d, knot %d: P_meas(%d, %d) is not the running row's\n", w, q.i, i, c);
                                return 1;
                            }
                        }
                    copies++;
                    continue;
                }
                const CpiResult y = refs[r++]->result();
                for (int c = 0; c < 15; c++)
                    for (int i = 0; i < 15; i++) {
                        const double scale = std::sqrt(std::fabs(at(y.P_meas, i, i) * at(y.P_meas, c, c)));
                        if (!(scale > 0)) { fprintf(stderr, "window %d: the reference window has a zero variance\n", w); return 1; }
                        ep = std::fmax(ep, std::fabs(at(x.P_meas, i, c) - at(y.P_meas, i, c)) / scale);
                    }
            }
        }
        printf("copies %zu inside %zu cov rel err %.3e\n", copies, r, ep);
        if (!(ep <= 1e-6)) { fprintf(stderr, "parity\n"); return 1; }
        printf("test_query_cov ok\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
