// test_query_stj.cpp -- GPU: model 2's seven bias Jacobians after every interval and at arbitrary times through
// cpi_host::CpiBatch::running_stj / at_stj (cpi_running_stj_batch_host / cpi_query_stj_batch_host).  Reads windows of recorded intervals
// and queries every window before its first stamp, on every knot stamp, 0.37 into every interval and past its last stamp, in shuffled
// order.  Checks itself and prints "test_query_stj ok":
//   - running_stj()[w][i] holds the members of running()[w][i] bit for bit, and J_q ... O_b after interval i: the last row agrees with
//     the window's own flushed members within 1e-8 (the contractual Jacobian gate);
//   - J_q ... O_b at a time on knot stamp i >= 1 (and at / past the last stamp) are running_stj()[w][i - 1]'s bit for bit, at a time
//     <= t_0 all zero;
//   - at a time inside interval i they agree with a window of its own -- the intervals 0 .. i - 1 and the tail feed_IMU(t_i, t_q, w_i,
//     a_i, w_i, a_i) -- flushed through CpiBatch, within 1e-8;
//   - the other members are those of at_cov(), bit for bit, and at_cov() / running() leave model 2's Jacobians at zero.
//   test_query_stj <windows file> <imu_avg>
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

static std::unique_ptr<CpiBase> make(const Win &w, bool avg) {
    std::unique_ptr<CpiBase> c(new CpiV2(0.005, 4e-6, 0.01, 2e-4, avg));
    c->setLinearizationPoints(Vec3{{w.l[0], w.l[1], w.l[2]}}, Vec3{{w.l[3], w.l[4], w.l[5]}}, Vec4{{w.l[6], w.l[7], w.l[8], w.l[9]}}, Vec3{{0, 0, 9.8}});
    return c;
}
static void feed(CpiBase &c, const std::array<double, 7> &p, const std::array<double, 7> &k) {
    c.feed_IMU(p[0], k[0], Vec3{{p[1], p[2], p[3]}}, Vec3{{p[4], p[5], p[6]}}, Vec3{{k[1], k[2], k[3]}}, Vec3{{k[4], k[5], k[6]}});
}
template <class A>
static bool same_bits(const A &a, const A &b) { return std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0; }
static bool same_rest(const CpiResult &a, const CpiResult &b) {
    return std::memcmp(&a.DT, &b.DT, sizeof(double)) == 0 && same_bits(a.alpha_tau, b.alpha_tau) && same_bits(a.beta_tau, b.beta_tau) &&
           same_bits(a.q_k2tau, b.q_k2tau) && same_bits(a.P_meas, b.P_meas);
}
static const Mat3 *jacs(const CpiResult &r, int f) {
    const Mat3 *m[7] = { &r.J_q, &r.J_a, &r.J_b, &r.H_a, &r.H_b, &r.O_a, &r.O_b };
    return m[f];
}
static bool same_jacs(const CpiResult &a, const CpiResult &b) {
    for (int f = 0; f < 7; f++) if (!same_bits(*jacs(a, f), *jacs(b, f))) return false;
    return true;
}
static bool zero_jacs(const CpiResult &a) {
    for (int f = 0; f < 7; f++) for (double v : *jacs(a, f)) if (v != 0) return false;
    return true;
}
static double jac_err(const CpiResult &a, const CpiResult &b) {
    double e = 0;
    for (int f = 0; f < 7; f++) for (int i = 0; i < 9; i++) e = std::fmax(e, std::fabs((*jacs(a, f))[i] - (*jacs(b, f))[i]));
    return e;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream f(argv[1]);
    const bool avg = atoi(argv[2]) != 0;
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
        struct Qry { int i; bool inside; };   // the knot index a query sits on (-1: before the window; n: past its end); inside interval i
        std::vector<std::vector<double>> times(W);
        std::vector<std::vector<Qry>> what(W);
        for (int w = 0; w < W; w++) {
            const Win &win = wins[w];
            const int n = (int)win.k.size() - 1;
            cs.push_back(make(win, avg));
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
        const std::vector<std::vector<CpiResult>> got = batch.at_stj(ctx, times);
        const std::vector<std::vector<CpiResult>> cov = batch.at_cov(ctx, times);
        const std::vector<std::vector<CpiResult>> rows = batch.running_stj(ctx);
        const std::vector<std::vector<CpiResult>> plain = batch.running(ctx);
        // the windows the inside queries stand for, all in one batch
        std::vector<std::unique_ptr<CpiBase>> refs;
        CpiBatch rb;
        for (int w = 0; w < W; w++)
            for (size_t a = 0; a < times[w].size(); a++) {
                const Qry q = what[w][a];
                if (!q.inside) continue;
                const Win &win = wins[w];
                refs.push_back(make(win, avg));
                for (int s = 1; s <= q.i; s++) feed(*refs.back(), win.k[s - 1], win.k[s]);
                std::array<double, 7> tail = win.k[q.i];
                tail[0] = times[w][a];
                feed(*refs.back(), win.k[q.i], tail);
                rb.add(refs.back().get());
            }
        rb.flush(ctx);
        batch.flush(ctx);
        size_t r = 0, copies = 0;
        double ej = 0, el = 0;
        for (int w = 0; w < W; w++) {
            const int n = (int)wins[w].k.size() - 1;
            if (got[w].size() != times[w].size() || cov[w].size() != times[w].size() || (int)rows[w].size() != n || (int)plain[w].size() != n) {
                fprintf(stderr, "window %d: sizes\n", w);
                return 1;
            }
            for (int i = 0; i < n; i++) {
                if (!same_rest(rows[w][i], plain[w][i])) { fprintf(stderr, "window %d, row %d: running_stj's members are not running()'s\n", w, i); return 1; }
                if (!zero_jacs(plain[w][i])) { fprintf(stderr, "running() wrote model 2's Jacobians\n"); return 1; }
            }
            if (n > 0) el = std::fmax(el, jac_err(rows[w][n - 1], cs[w]->result()));
            for (size_t a = 0; a < times[w].size(); a++) {
                const Qry q = what[w][a];
                const CpiResult &x = got[w][a];
                if (!same_rest(x, cov[w][a])) { fprintf(stderr, "window %d, query %zu: at_stj's members are not at_cov()'s\n", w, a); return 1; }
                if (!zero_jacs(cov[w][a])) { fprintf(stderr, "at_cov() wrote model 2's Jacobians\n"); return 1; }
                if (!q.inside) {
                    const bool ok = q.i <= 0 ? zero_jacs(x) : same_jacs(x, rows[w][q.i - 1]);
                    if (!ok) { fprintf(stderr, "window %d, knot %d: the Jacobians are not the running row's\n", w, q.i); return 1; }
                    copies++;
                    continue;
                }
                ej = std::fmax(ej, jac_err(x, refs[r++]->result()));
            }
        }
        printf("copies %zu inside %zu jacobian err %.3e last row err %.3e\n", copies, r, ej, el);
        if (!(ej <= 1e-8) || !(el <= 1e-8)) { fprintf(stderr, "parity\n"); return 1; }
        printf("test_query_stj ok\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
