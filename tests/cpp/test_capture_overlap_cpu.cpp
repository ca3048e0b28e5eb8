// CPU only: cpi_amd/csrc/cpi_capture_overlap.hpp -- the footprint conflict test and the window bookkeeping, driven with fake
// node ids.  Built with -fsanitize=address,undefined by tests/test_capture_overlap_cpu.py; the program checks itself and
// prints "test_capture_overlap_cpu ok" as its last line.
//
// The invariant, checked by brute-force reachability over random call sequences:
//   (1) two library nodes of one capture without a path between them have disjoint footprints, belong to the same window
//       (nothing else was captured between them) and are fewer than D calls apart;
//   (2) every node the caller captures has a path from every node captured on the stream before it, and every library node has
//       a path from every caller node captured before it.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>

#include "../../cpi_amd/csrc/cpi_capture_overlap.hpp"

using namespace cpi::overlap;

static int g_fail = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
    } while (0)

static const int OUT_N[13] = { 1, 3, 3, 4, 9, 9, 9, 9, 9, 9, 9, 225, 120 };

static Footprint fp_of(int64_t W, int32_t N, const double *knots, const int64_t *first, const int32_t *count, const double *lin, const double *qk,
                       double *DT, double *alpha, double *J_q = nullptr) {
    const void *outs[13] = { DT, alpha, nullptr, nullptr, J_q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    return make_footprint(W, N, knots, first, count, lin, qk, outs, OUT_N, 13);
}

static void test_ranges() {
    char *b = (char *)0x10000;
    // touching: [0,16) and [16,32) share no byte
    CHECK(!ranges_overlap(make_range(b, 16), make_range(b + 16, 16)));
    CHECK(!ranges_overlap(make_range(b + 16, 16), make_range(b, 16)));
    // one byte shared
    CHECK(ranges_overlap(make_range(b, 17), make_range(b + 16, 16)));
    CHECK(ranges_overlap(make_range(b + 16, 16), make_range(b, 17)));
    // nested, identical
    CHECK(ranges_overlap(make_range(b, 64), make_range(b + 8, 8)));
    CHECK(ranges_overlap(make_range(b + 8, 8), make_range(b, 64)));
    CHECK(ranges_overlap(make_range(b, 64), make_range(b, 64)));
    // empty ranges and NULL overlap nothing, not even when they lie inside the other range
    CHECK(!ranges_overlap(make_range(b + 8, 0), make_range(b, 64)));
    CHECK(!ranges_overlap(make_range(b, 64), make_range(b + 8, 0)));
    CHECK(!ranges_overlap(make_range(nullptr, 64), make_range(nullptr, 64)));
    CHECK(!ranges_overlap(make_range(b, 0), make_range(b, 0)));
    // a range that would wrap the address space reaches its top instead
    const Range top = make_range((void *)(UINTPTR_MAX - 7), 64);
    CHECK(top.hi == UINTPTR_MAX && top.lo < top.hi);
    CHECK(ranges_overlap(top, make_range((void *)(UINTPTR_MAX - 3), 2)));
}

static void test_footprints() {
    const int64_t W = 10;
    const int32_t N = 4;
    std::vector<double> mem(100000);
    double *knA = &mem[0], *knB = &mem[1000], *linA = &mem[2000], *linB = &mem[2100], *qk = &mem[2200];
    double *dtA = &mem[3000], *dtB = &mem[3010], *alA = &mem[3100], *alB = &mem[3130], *jq = &mem[3400];
    int32_t *cnt = (int32_t *)&mem[4000];
    int64_t *first = (int64_t *)&mem[5000];

    const Footprint a = fp_of(W, N, knA, nullptr, nullptr, linA, nullptr, dtA, alA);
    CHECK(!a.unknown && a.nr == 2 && a.nw == 2);
    CHECK(a.r[0].hi - a.r[0].lo == (uintptr_t)W * (N + 1) * 56);
    CHECK(a.r[1].hi - a.r[1].lo == (uintptr_t)W * 48);
    CHECK(a.w[0].hi - a.w[0].lo == (uintptr_t)W * 8 && a.w[1].hi - a.w[1].lo == (uintptr_t)W * 24);
    // disjoint everything; outputs that TOUCH (dtB starts where dtA's W doubles end)
    const Footprint b = fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtB, alB);
    CHECK(!conflict(a, b) && !conflict(b, a));
    // shared inputs are no conflict
    CHECK(!conflict(a, fp_of(W, N, knA, nullptr, nullptr, linA, nullptr, dtB, alB)));
    // write / write: the same output set; outputs overlapping by one row; by one double
    CHECK(conflict(a, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtA, alB)));
    CHECK(conflict(a, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtB, alA + 3 * (W - 1))));
    CHECK(conflict(a, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtA + (W - 1), alB)));
    CHECK(!conflict(a, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtA + W, alA + 3 * W)));
    // write / read and read / write: one call's output is the other's lin, knots, q_k_lin, count
    const Footprint wl = fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, linA + 6 * (W - 1), alB);
    CHECK(conflict(a, wl) && conflict(wl, a));
    const Footprint wk = fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtB, knA + (W * (N + 1) * 7 - 1));
    CHECK(conflict(a, wk) && conflict(wk, a));
    CHECK(!conflict(a, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtB, knA + W * (N + 1) * 7)));
    const Footprint rq = fp_of(W, N, knA, nullptr, nullptr, linA, qk, dtA, alA);
    CHECK(rq.nr == 3);
    CHECK(conflict(rq, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, qk + 4 * W - 1, alB)));
    CHECK(!conflict(rq, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, qk + 4 * W, alB)));
    const Footprint rc = fp_of(W, N, knA, nullptr, cnt, linA, nullptr, dtA, alA);
    CHECK(rc.nr == 3);
    CHECK(conflict(rc, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, (double *)cnt + (W * 4 - 1) / 8, alB)));
    CHECK(!conflict(rc, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, (double *)cnt + (W * 4 + 7) / 8, alB)));
    // NULL outputs write nothing: a Jacobian field only one side asks for
    const Footprint aj = fp_of(W, N, knA, nullptr, nullptr, linA, nullptr, dtA, alA, jq);
    CHECK(aj.nw == 3 && !conflict(aj, b));
    CHECK(conflict(aj, fp_of(W, N, knB, nullptr, nullptr, linB, nullptr, dtB, jq + 9 * W - 1)));
    const Footprint none = fp_of(W, N, knA, nullptr, nullptr, linA, nullptr, nullptr, nullptr);
    CHECK(none.nw == 0 && !conflict(none, a) && !conflict(a, none) && !conflict(none, none));
    // CSR: the knot span is unknown -> conflicts with everything, itself included
    const Footprint csr = fp_of(W, N, knB, first, cnt, linB, nullptr, dtB, alB);
    CHECK(csr.unknown && conflict(csr, a) && conflict(a, csr) && conflict(csr, none) && conflict(csr, csr));
    // nothing to do / nonsense sizes: unknown as well
    CHECK(fp_of(0, N, knA, nullptr, nullptr, linA, nullptr, dtA, alA).unknown);
    CHECK(fp_of(W, -1, knA, nullptr, nullptr, linA, nullptr, dtA, alA).unknown);
    // the context's starting policy: default 2, clamped, and depth 1 for good when the process asks for fewer than 4 queues
    CHECK(policy_from(nullptr, nullptr).allowed && policy_from(nullptr, nullptr).depth == 2);
    CHECK(policy_from("", "").depth == 2 && policy_from("4", "2").depth == 2 && policy_from("32", "9").depth == 4 && policy_from(nullptr, "0").depth == 1);
    CHECK(!policy_from("2", "4").allowed && policy_from("2", "4").depth == 1 && policy_from("3", nullptr).depth == 1 && policy_from("4", nullptr).allowed);
    // several contexts in one capture: serial for the rest of that capture, for every context; a new capture starts afresh
    CaptureRegistry reg;
    int ctxA = 0, ctxB = 0;
    CHECK(reg.sole(0, &ctxA) && reg.sole(0, &ctxA) && !reg.sole(0, &ctxB) && !reg.sole(0, &ctxA) && !reg.sole(0, &ctxB));
    CHECK(reg.sole(7, &ctxB) && reg.sole(7, &ctxB) && !reg.sole(7, &ctxA) && reg.sole(8, &ctxA));
    // only launches of at most one wavefront per SIMD have an idle head and tail for a neighbour to fill
    CHECK(launch_is_latency_bound(1) && launch_is_latency_bound(1000) && launch_is_latency_bound(1024) && !launch_is_latency_bound(1025) && !launch_is_latency_bound(15625));
    CHECK(clamp_depth(-5) == 1 &&clamp_depth(0) == 1 && clamp_depth(1) == 1 && clamp_depth(3) == 3 && clamp_depth(4) == 4 && clamp_depth(99) == 4);
}

// ---- the window against a simulated capture -----------------------------------------------------------------------------------
struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};
struct SimNode {
    bool lib;
    int capture, window, call;   // library nodes: which window (a counter) and which call of it
    Footprint fp;
    std::vector<int> preds;
};
static bool reaches(const std::vector<SimNode> &g, int from, int to) {   // from < to: nodes are numbered in capture order
    std::vector<char> seen(g.size(), 0);
    std::vector<int> todo(1, to);
    while (!todo.empty()) {
        const int n = todo.back();
        todo.pop_back();
        if (n == from) return true;
        if (n < from || seen[n]) continue;
        seen[n] = 1;
        for (int p : g[n].preds) todo.push_back(p);
    }
    return false;
}

static void run_sequence(uint64_t seed, int D, bool always_disjoint) {
    Rng rng{seed * 2654435761ull + 12345};
    std::vector<double> mem(1 << 16);
    const int64_t W = 8;
    const int32_t N = 3;
    // a pool of buffers: input sets 0..3, output sets 0..5 of which 4 and 5 overlap 0 and 1 by one row
    auto kn = [&](int i) { return &mem[0] + 1000 * i; };
    auto lin = [&](int i) { return &mem[8000] + 100 * i; };
    auto dt = [&](int i) { return i < 4 ? &mem[10000] + 100 * i : &mem[10000] + 100 * (i - 4) + (W - 1); };
    auto al = [&](int i) { return &mem[12000] + 100 * i; };

    std::vector<SimNode> g;
    Window<int> win;
    std::vector<int> cur, preds;   // cur: the stream's capture dependencies
    unsigned long long cap = 1;
    int window_no = 0;
    const int steps = 40;
    for (int s = 0; s < steps; s++) {
        const int what = rng.below(20);
        if (what == 0) {   // the capture ends, another begins: new id, no dependencies; node ids go on counting
            cap++;
            cur.clear();
            continue;
        }
        SimNode n;
        n.capture = (int)cap;
        const int id = (int)g.size();
        if (what <= 2) {   // the caller captures something of their own: ordered behind the stream's dependencies
            n.lib = false; n.window = -1; n.call = -1;
            n.preds = cur;
            g.push_back(n);
            cur.assign(1, id);
            continue;
        }
        n.lib = true;
        if (always_disjoint) {
            const int k = s % 6;   // six disjoint input / output sets in turn
            n.fp = fp_of(W, N, kn(k), nullptr, nullptr, lin(k), nullptr, &mem[20000] + 100 * k, &mem[30000] + 100 * k);
        } else if (rng.below(10) == 0) {
            n.fp = fp_of(W, N, kn(0), (const int64_t *)&mem[40000], nullptr, lin(0), nullptr, dt(rng.below(6)), al(rng.below(6)));   // CSR
        } else if (rng.below(8) == 0) {
            n.fp = fp_of(W, N, kn(rng.below(4)), nullptr, nullptr, lin(rng.below(4)), nullptr, lin(rng.below(4)), al(rng.below(6)));   // writes a lin
        } else {
            n.fp = fp_of(W, N, kn(rng.below(4)), nullptr, nullptr, lin(rng.below(4)), nullptr, dt(rng.below(6)), al(rng.below(6)));
        }
        if (!win.continues(cap, cur.data(), cur.size())) { win.open_at(cap, D, cur.data(), cur.size()); window_no++; }
        n.window = window_no;
        n.call = (int)win.calls();
        win.plan(n.fp, preds);
        n.preds = preds;
        for (size_t i = 0; i < preds.size(); i++)
            for (size_t j = i + 1; j < preds.size(); j++) CHECK(preds[i] != preds[j]);
        CHECK((int)preds.size() <= 2 * D - 1 || preds.size() == win.base().size());
        g.push_back(n);
        win.commit(id, n.fp);
        cur = win.frontier();
        for (size_t i = 0; i < cur.size(); i++)
            for (size_t j = i + 1; j < cur.size(); j++) CHECK(cur[i] != cur[j]);
    }
    int unordered = 0;
    for (int b = 0; b < (int)g.size(); b++)
        for (int a = 0; a < b; a++) {
            if (g[a].capture != g[b].capture) continue;
            if (reaches(g, a, b)) continue;
            unordered++;
            // no path: only two library calls of one window, fewer than D apart, on disjoint memory
            CHECK(g[a].lib && g[b].lib);
            CHECK(g[a].window == g[b].window);
            CHECK(g[b].call - g[a].call < D);
            CHECK(!conflict(g[a].fp, g[b].fp));
        }
    if (D == 1) CHECK(unordered == 0);
    if (always_disjoint && D > 1) {
        // and the relaxation is really taken: inside a window, disjoint neighbours closer than D have NO path
        for (int b = 0; b < (int)g.size(); b++)
            for (int a = 0; a < b; a++)
                if (g[a].lib && g[b].lib && g[a].capture == g[b].capture && g[a].window == g[b].window && g[b].call - g[a].call < D)
                    CHECK(!reaches(g, a, b));
    }
}

int main() {
    test_ranges();
    test_footprints();
    for (int seq = 0; seq < 200; seq++) run_sequence(20240611u + (uint64_t)seq, 1 + seq % 4, false);
    for (int seq = 0; seq < 16; seq++) run_sequence(777u + (uint64_t)seq, 1 + seq % 4, true);
    if (g_fail) { printf("test_capture_overlap_cpu: %d checks FAILED\n", g_fail); return 1; }
    printf("test_capture_overlap_cpu ok\n");
    return 0;
}
