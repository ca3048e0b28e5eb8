// test_query.cpp -- GPU: the members of a window at arbitrary times through cpi_host::CpiBatch::at (cpi_query_batch_host).
// Reads windows of recorded intervals and queries every window before its first stamp, on every knot stamp, 0.37 into every
// interval and past its last stamp, in shuffled order.  Checks itself and prints "test_query ok":
//   - a time on knot stamp i >= 1 (and at / past the last stamp) is running()[w][i - 1] bit for bit, a time <= t_0 the zero state;
//   - a time inside interval i agrees with a window of its own -- the intervals 0 .. i - 1 and the tail feed_IMU(t_i, t_q, w_i,
//     a_i, w_i, a_i) -- flushed through CpiBatch, means at 1e-9 and the model-1 Jacobians at 1e-8;
//   - a window with a separator knot throws std::logic_error.
//   test_query <windows file> <model> <imu_avg>
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
static bool same_bits(const CpiResult &a, const CpiResult &b, bool jac) {
    bool ok = std::memcmp(&a.DT, &b.DT, sizeof(double)) == 0 && same_bits(a.alpha_tau, b.alpha_tau) && same_bits(a.beta_tau, b.beta_tau) &&
              same_bits(a.q_k2tau, b.q_k2tau);
    if (jac) ok = ok && same_bits(a.J_q, b.J_q) && same_bits(a.J_a, b.J_a) && same_bits(a.J_b, b.J_b) && same_bits(a.H_a, b.H_a) && same_bits(a.H_b, b.H_b);
    return ok;
}
template <class A>
static double dist(const A &a, const A &b) {
    double e = 0;
    for (size_t i = 0; i < a.size(); i++) e = std::fmax(e, std::fabs(a[i] - b[i]));
    return e;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::ifstream f(argv[1]);
    const int model = atoi(argv[2]);
    const bool avg = atoi(argv[3]) != 0, jac = model == 1;
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
        const std::vector<std::vector<CpiResult>> got = batch.at(ctx, times);
        const std::vector<std::vector<CpiResult>> rows = batch.running(ctx);
        const CpiResult zero;
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
        double em = 0, ej = 0;
        for (int w = 0; w < W; w++) {
            const int n = (int)wins[w].k.size() - 1;
            if (got[w].size() != times[w].size() || (int)rows[w].size() != n) { fprintf(stderr, "window %d: sizes\n", w); return 1; }
            for (size_t a = 0; a < times[w].size(); a++) {
                const Qry q = what[w][a];
                const CpiResult &x = got[w][a];
                if (!q.inside) {
                    const CpiResult &want = q.i <= 0 ? zero : rows[w][q.i - 1];
                    if (!same_bits(x, want, jac)) { fprintf(stderr, "window %d, knot %d: not the running row bit for bit\n", w, q.i); return 1; }
                    copies++;
                    continue;
                }
                const CpiResult y = refs[r++]->result();
                em = std::fmax(em, std::fmax(std::fabs(x.DT - y.DT), std::fmax(dist(x.alpha_tau, y.alpha_tau), std::fmax(dist(x.beta_tau, y.beta_tau), dist(x.q_k2tau, y.q_k2tau)))));
                if (jac) ej = std::fmax(ej, std::fmax(dist(x.J_q, y.J_q), std::fmax(dist(x.J_a, y.J_a), std::fmax(dist(x.J_b, y.J_b), std::fmax(dist(x.H_a, y.H_a), dist(x.H_b, y.H_b))))));
            }
        }
        printf("copies %zu inside %zu mean err %.3e jac err %.3e\n", copies, r, em, ej);
        if (!(em <= 1e-9) || !(ej <= 1e-8)) { fprintf(stderr, "parity\n"); return 1; }
        // a window whose intervals do not chain has no time axis
        std::unique_ptr<CpiBase> gap = make(wins[0], model, avg);
        feed(*gap, wins[0].k[0], wins[0].k[1]);
        std::array<double, 7> far0 = wins[0].k[0], far1 = wins[0].k[1];
        far0[0] += 50.0; far1[0] += 50.0;
        feed(*gap, far0, far1);
        CpiBatch gb;
        gb.add(gap.get());
        bool thrown = false;
        try { gb.at(ctx, {{wins[0].k[0][0]}}); } catch (const std::logic_error &) { thrown = true; }
        if (!thrown) { fprintf(stderr, "separator window accepted\n"); return 1; }
        printf("test_query ok\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
