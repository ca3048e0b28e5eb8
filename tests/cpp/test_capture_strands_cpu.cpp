// CPU only: cpi_amd/csrc/cpi_capture_overlap.hpp -- RangeSet, the strand bookkeeping (Strands) and the choice of a new context's
// capture shape (capture_policy_from), driven with fake node ids and fake addresses.  Built with -fsanitize=address,undefined by
// tests/test_capture_strands_cpu.py; the program checks itself and prints "test_capture_strands_cpu ok" as its last line.
//
// The invariant, checked by brute-force reachability over random call sequences:
//   (a) two library nodes of one capture without a path between them have disjoint footprints and belong to the same window
//       (nothing else was captured between them, and no join);
//   (b) every node captured later has a path from every library node before it, and every library node has a path from
//       everything captured on the stream before it  (so: whenever a pair has no path, both are library nodes).
// Beside it: a call that is no join has exactly one in-edge (or the base), no node has more than S, the frontier has at most S
// nodes and none twice, and the placement is the one a model that keeps every footprint of every strand arrives at.
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

static Range rg(uintptr_t lo, uintptr_t hi) { return Range{lo, hi}; }

template <int Cap>
static bool is_sorted_and_coalesced(const RangeSet<Cap> &s) {
    for (int i = 0; i < s.size(); i++) {
        if (!(s[i].lo < s[i].hi)) return false;
        if (i && !(s[i - 1].hi < s[i].lo)) return false;   // neither overlapping nor touching
    }
    return s.size() <= Cap;
}

static void test_rangeset() {
    RangeSet<4> s;
    CHECK(s.size() == 0 && !s.overlaps(rg(0, 100)));
    // an empty range adds nothing and overlaps nothing
    CHECK(s.add(rg(50, 50)) && s.add(rg(60, 40)) && s.size() == 0);
    CHECK(s.add(rg(100, 200)) && s.size() == 1);
    CHECK(!s.overlaps(rg(150, 150)) && s.overlaps(rg(150, 151)) && !s.overlaps(rg(200, 300)) && !s.overlaps(rg(0, 100)) && s.overlaps(rg(199, 300)) && s.overlaps(rg(0, 101)));
    // identical, nested
    CHECK(s.add(rg(100, 200)) && s.add(rg(120, 130)) && s.size() == 1 && s[0].lo == 100 && s[0].hi == 200);
    // touching at either end merges
    CHECK(s.add(rg(200, 250)) && s.size() == 1 && s[0].hi == 250);
    CHECK(s.add(rg(90, 100)) && s.size() == 1 && s[0].lo == 90);
    // overlapping by one byte
    CHECK(s.add(rg(249, 260)) && s.size() == 1 && s[0].hi == 260);
    // separate entries stay sorted whatever the order they arrive in
    CHECK(s.add(rg(500, 600)) && s.add(rg(300, 400)) && s.add(rg(10, 20)) && s.size() == 4 && is_sorted_and_coalesced(s));
    CHECK(s[0].lo == 10 && s[1].lo == 90 && s[2].lo == 300 && s[3].lo == 500);
    CHECK(s.overlaps(rg(0, 11)) && !s.overlaps(rg(20, 90)) && s.overlaps(rg(20, 91)) && !s.overlaps(rg(260, 300)) && !s.overlaps(rg(400, 500)) && !s.overlaps(rg(600, 700)) && s.overlaps(rg(599, 700)));
    // full: a range that starts a new entry is refused and changes nothing; one that merges is still taken
    CHECK(!s.add(rg(700, 800)) && !s.add(rg(0, 5)) && !s.add(rg(30, 40)) && s.size() == 4 && is_sorted_and_coalesced(s));
    CHECK(s[0].lo == 10 && s[0].hi == 20 && s[3].lo == 500 && s[3].hi == 600 && !s.overlaps(rg(700, 800)));
    CHECK(s.add(rg(600, 700)) && s.size() == 4 && s[3].hi == 700);
    // one range that bridges several entries collapses them
    CHECK(s.add(rg(20, 300)) && s.size() == 2 && s[0].lo == 10 && s[0].hi == 400 && s[1].lo == 500 && is_sorted_and_coalesced(s));
    CHECK(s.add(rg(0, 1000)) && s.size() == 1 && s[0].lo == 0 && s[0].hi == 1000);
    // the saturating top-of-address-space range
    const Range top = make_range((void *)(UINTPTR_MAX - 7), 64);
    CHECK(top.hi == UINTPTR_MAX);
    CHECK(s.add(top) && s.size() == 2 && s[1].hi == UINTPTR_MAX && s.overlaps(make_range((void *)(UINTPTR_MAX - 3), 2)) && !s.overlaps(make_range((void *)(UINTPTR_MAX - 64), 50)));
    CHECK(s.add(make_range((void *)(UINTPTR_MAX - 100), 1000)) && s.size() == 2 && s[1].lo == UINTPTR_MAX - 100 && s[1].hi == UINTPTR_MAX);
    s.clear();
    CHECK(s.size() == 0 && !s.overlaps(rg(0, UINTPTR_MAX)));
    // against a byte map, random ranges in a small space: the set is the union, sorted and coalesced, and never past its end
    uint64_t x = 88172645463325252ull;
    for (int round = 0; round < 200; round++) {
        RangeSet<6> t;
        char map[64] = {0};
        for (int k = 0; k < 12; k++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const uintptr_t lo = (uintptr_t)(x % 60), len = (uintptr_t)((x >> 8) % 6);
            RangeSet<6> before = t;
            if (t.add(rg(1000 + lo, 1000 + lo + len))) {
                for (uintptr_t b = lo; b < lo + len; b++) map[b] = 1;
            } else {
                CHECK(before.size() == 6 && t.size() == 6);
                for (int i = 0; i < 6; i++) CHECK(before[i].lo == t[i].lo && before[i].hi == t[i].hi);
            }
            CHECK(is_sorted_and_coalesced(t));
            for (uintptr_t b = 0; b < 64; b++) CHECK(t.overlaps(rg(1000 + b, 1001 + b)) == (map[b] != 0));
        }
    }
}

static void test_policy() {
    // neither variable: the shipped default
    const CapturePolicy d = capture_policy_from(nullptr, nullptr, nullptr);
    CHECK(d.allowed && d.shape == kDefaultShape && d.n == (kDefaultShape == kShapeStrands ? kDefaultStrands : kDefaultDepth));
    CHECK(kDefaultStrands >= 1 && kDefaultStrands <= kMaxStrands && kMaxStrands == 4);
    const char *hw[] = { nullptr, "", "4", "32", "3", "1", "0" };
    const char *st[] = { nullptr, "", "1", "2", "3", "4", "9", "0", "-2" };
    const char *dp[] = { nullptr, "", "1", "2", "4", "7", "0" };
    for (const char *h : hw)
        for (const char *s : st)
            for (const char *p : dp) {
                const CapturePolicy c = capture_policy_from(h, s, p);
                const bool few = h && *h && atoi(h) < 4;
                if (few) { CHECK(!c.allowed && c.n == 1); continue; }   // below 4 queues: serial whatever else is asked
                CHECK(c.allowed);
                if (s && *s) {   // strands win over the depth
                    const int want = atoi(s) < 1 ? 1 : (atoi(s) > 4 ? 4 : atoi(s));
                    CHECK(c.shape == kShapeStrands && c.n == want);
                } else if (p && *p) {
                    const int want = atoi(p) < 1 ? 1 : (atoi(p) > 4 ? 4 : atoi(p));
                    CHECK(c.shape == kShapeLookback && c.n == want);
                    CHECK(policy_from(h, p).depth == c.n);   // the look-back shape reads its variable as it always did
                } else {
                    CHECK(c.shape == d.shape && c.n == d.n);
                }
            }
    CHECK(capture_policy_from("4", "3", "2").shape == kShapeStrands && capture_policy_from("4", "3", "2").n == 3);
    CHECK(capture_policy_from(nullptr, nullptr, "2").shape == kShapeLookback && capture_policy_from(nullptr, nullptr, "2").n == 2);
    CHECK(clamp_strands(-3) == 1 && clamp_strands(0) == 1 && clamp_strands(1) == 1 && clamp_strands(4) == 4 && clamp_strands(5) == 4);
}

// ---- the strands against a simulated capture ----------------------------------------------------------------------------------
struct SimNode {
    bool lib, join;
    int capture, epoch, strand;   // library nodes: which window or restart of one (a counter), and which strand
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

static bool same_fp(const Footprint &a, const Footprint &b) {
    if (a.unknown != b.unknown || a.nr != b.nr || a.nw != b.nw) return false;
    for (int k = 0; k < a.nr; k++) if (a.r[k].lo != b.r[k].lo || a.r[k].hi != b.r[k].hi) return false;
    for (int k = 0; k < a.nw; k++) if (a.w[k].lo != b.w[k].lo || a.w[k].hi != b.w[k].hi) return false;
    return true;
}

// One stream under capture.  `exact`: the summaries never overflow, so the placement must be what the model arrives at that keeps
// every footprint of every strand (conflict() pair by pair); otherwise joins beyond the model's are allowed (overflow).
template <class StrandsT>
struct Sim {
    int S;
    bool exact;
    StrandsT st;
    std::vector<SimNode> g;
    std::vector<int> cur, preds;   // cur: the stream's capture dependencies
    unsigned long long cap = 1;
    int epoch = 0, joins = 0, overflow_joins = 0;
    std::vector<std::vector<Footprint>> model;   // per strand, the footprints since the last restart
    long long ext[kMaxStrands] = {0, 0, 0, 0}, tick = 0;   // per strand, when it was extended last

    Sim(int S_, bool exact_) : S(S_), exact(exact_), model(kMaxStrands) {}
    void new_capture() { cap++; cur.clear(); }
    int caller_node() {
        SimNode n;
        n.lib = false; n.join = false; n.capture = (int)cap; n.epoch = -1; n.strand = -1;
        n.preds = cur;
        g.push_back(n);
        cur.assign(1, (int)g.size() - 1);
        return cur[0];
    }
    int lib_call(const Footprint &fp) {
        const int id = (int)g.size();
        if (!st.continues(cap, cur.data(), cur.size())) {
            st.open_at(cap, S, cur.data(), cur.size());
            epoch++;
            for (auto &m : model) m.clear();
        }
        // the model: strands with a conflicting call, non-empty strands
        int nhit = 0, hit = -1, nonempty = 0;
        for (int s = 0; s < kMaxStrands; s++) {
            bool c = false;
            for (const Footprint &o : model[s]) c = c || conflict(o, fp);
            if (c) { nhit++; hit = s; }
            if (!model[s].empty()) nonempty++;
        }
        const bool model_join = nhit >= 2 || (fp.unknown && nonempty >= 2);
        const std::vector<int> base = st.base();
        st.plan(fp, preds);
        for (size_t i = 0; i < preds.size(); i++)
            for (size_t j = i + 1; j < preds.size(); j++) CHECK(preds[i] != preds[j]);
        SimNode n;
        n.lib = true; n.capture = (int)cap; n.fp = fp; n.preds = preds;
        st.commit(id, fp);
        n.join = st.last_strand() < 0;
        n.strand = st.last_strand();
        n.epoch = epoch;
        if (model_join) CHECK(n.join);
        if (exact) CHECK(n.join == model_join);
        if (n.join) {
            joins++;
            if (!model_join) overflow_joins++;
            if (nonempty) CHECK((int)preds.size() == nonempty && (int)preds.size() <= S);
            else CHECK(preds == base);
            epoch++;   // everything later descends from it: a window of its own
            for (auto &m : model) m.clear();
            CHECK(st.frontier().size() == 1 && st.frontier()[0] == id);
        } else {
            CHECK(n.strand >= 0 && n.strand < S);
            if (nhit == 1) CHECK(n.strand == hit);
            else {
                CHECK(model[n.strand].empty() || nonempty == S);   // empty strands first ...
                for (int s = 0; s < S; s++) CHECK(model[n.strand].empty() ? (s >= n.strand || !model[s].empty()) : ext[n.strand] <= ext[s]);   // ... then the least recently extended
            }
            ext[n.strand] = ++tick;
            if (model[n.strand].empty()) CHECK(preds == base);
            else CHECK(preds.size() == 1 && g[preds[0]].lib && g[preds[0]].strand == n.strand && g[preds[0]].epoch == n.epoch);
            bool held = false;   // (a set: a walk over a fixed pool adds nothing new after its first period)
            for (const Footprint &o : model[n.strand]) held = held || same_fp(o, fp);
            if (!held) model[n.strand].push_back(fp);
        }
        g.push_back(n);
        cur = st.frontier();
        CHECK((int)cur.size() <= S && !cur.empty());
        for (size_t i = 0; i < cur.size(); i++)
            for (size_t j = i + 1; j < cur.size(); j++) CHECK(cur[i] != cur[j]);
        return id;
    }
    // (a) and (b) by brute force; returns the number of unordered pairs
    int check_invariant() const {
        int unordered = 0;
        for (int b = 0; b < (int)g.size(); b++)
            for (int a = 0; a < b; a++) {
                if (g[a].capture != g[b].capture) continue;
                if (reaches(g, a, b)) continue;
                unordered++;
                CHECK(g[a].lib && g[b].lib);
                CHECK(!g[a].join && !g[b].join);
                CHECK(g[a].epoch == g[b].epoch);
                CHECK(g[a].strand != g[b].strand);
                CHECK(!conflict(g[a].fp, g[b].fp));
            }
        return unordered;
    }
};

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

static Footprint fp_of(int64_t W, int32_t N, const void *knots, const void *first, const void *lin, const void *qk, double *DT, double *alpha,
                       double *beta = nullptr, double *q = nullptr) {
    const void *outs[13] = { DT, alpha, beta, q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    return make_footprint(W, N, knots, first, nullptr, lin, qk, outs, OUT_N, 13);
}

// Random sequences: disjoint calls, conflicting calls (shared or one-row-overlapping outputs, an output that is another call's
// lin), unknown calls, caller nodes in between and new captures.  Returns {unordered pairs, joins, overflow joins}.
struct Tally { long long unordered = 0, joins = 0, overflow = 0, calls = 0; };
template <class StrandsT>
static void run_sequence(uint64_t seed, int S, bool exact, int nsets, Tally &t) {
    Rng rng{seed * 2654435761ull + 12345};
    const int64_t W = 8;
    const int32_t N = 3;
    char *mem = (char *)0x40000000;   // fake addresses: nothing is dereferenced
    auto kn = [&](int i) { return (double *)(mem + 0x10000 * i); };
    auto lin = [&](int i) { return (double *)(mem + 0x800000 + 0x1000 * i); };
    // output set i: DT and alpha well apart; sets nsets .. nsets + 1 overlap sets 0 and 1 by one row of DT
    auto dt = [&](int i) { return i < nsets ? (double *)(mem + 0x1000000 + 0x1000 * i) : (double *)(mem + 0x1000000 + 0x1000 * (i - nsets)) + (W - 1); };
    auto al = [&](int i) { return (double *)(mem + 0x2000000 + 0x1000 * i); };

    Sim<StrandsT> sim(S, exact);
    for (int s = 0; s < 48; s++) {
        const int what = rng.below(24);
        if (what == 0) { sim.new_capture(); continue; }
        if (what <= 2) { sim.caller_node(); continue; }
        Footprint fp;
        const int kind = rng.below(16);
        if (kind == 0) fp = fp_of(W, N, kn(0), mem + 0x3000000, lin(0), nullptr, dt(rng.below(nsets)), al(rng.below(nsets)));   // CSR: unknown
        else if (kind == 1) fp = fp_of(W, N, kn(rng.below(4)), nullptr, lin(rng.below(4)), nullptr, lin(rng.below(4)), al(rng.below(nsets)));   // writes a lin
        else if (kind <= 3) fp = fp_of(W, N, kn(rng.below(4)), nullptr, lin(rng.below(4)), nullptr, dt(rng.below(nsets + 2)), al(rng.below(nsets)));   // any DT with any alpha
        else { const int k = rng.below(nsets); fp = fp_of(W, N, kn(rng.below(4)), nullptr, lin(rng.below(4)), nullptr, dt(k), al(k)); }   // one whole set
        sim.lib_call(fp);
        t.calls++;
    }
    const int un = sim.check_invariant();
    if (S == 1) CHECK(un == 0 && sim.joins == sim.overflow_joins);   // one strand: a chain, and nothing but an overflow joins
    t.unordered += un; t.joins += sim.joins; t.overflow += sim.overflow_joins;
}

// ---- fixed patterns -----------------------------------------------------------------------------------------------------------
// The headline's walk: 12 input batches of knots + lin + q_k_lin, a ring of 4 packed output slabs (DT | alpha | beta | q), 10 000
// windows of 50 samples.  At the shipped capacities: no join, one in-edge per node, periodic placement.
static Footprint headline_fp(int i) {
    const int64_t W = 10000;
    const int32_t N = 50;
    const int b = i % 12, s = i % 4;
    char *kn = (char *)0x7f0000000000 + (uintptr_t)0x2000000 * b;   // 28.56 MB of knots per batch, 32 MB apart
    char *lin = (char *)0x7f1000000000 + (uintptr_t)0x100000 * b;
    char *qk = (char *)0x7f2000000000 + (uintptr_t)0x100000 * b;
    double *slab = (double *)((char *)0x7f3000000000 + (uintptr_t)0x200000 * s);
    return fp_of(W, N, kn, nullptr, lin, qk, slab, slab + W, slab + 4 * W, slab + 7 * W);
}
static void test_headline_walk(int S) {
    Sim<Strands<int>> sim(S, true);
    sim.caller_node();   // whatever the capture began with
    const int first = (int)sim.g.size();
    const int calls = 5000;
    for (int i = 0; i < calls; i++) sim.lib_call(headline_fp(i));
    CHECK(sim.joins == 0 && sim.st.joins() == 0);
    int load[kMaxStrands] = {0, 0, 0, 0};
    for (int i = 0; i < calls; i++) {
        const SimNode &n = sim.g[first + i];
        CHECK(n.preds.size() == 1 && !n.join);
        if (i >= 12) CHECK(n.strand == sim.g[first + i - 12].strand);   // periodic in the walk's period
        if (i >= 4) CHECK(n.strand == sim.g[first + i - 4].strand);     // a slab stays on its strand
        load[n.strand]++;
        int want = -1;   // the predecessor, as a call number (-1: the base)
        if (S == 2) want = i - 2;                                       // even and odd calls: two pure chains
        if (S == 4) want = i - 4;                                       // one chain per slab
        if (S == 3) want = (i % 4 == 0) ? i - 1 : (i % 4 == 3 ? i - 3 : i - 4);   // slabs 0 and 3 share a strand: 2 : 1 : 1
        if (want < 0) CHECK(n.preds[0] == first - 1);
        else CHECK(n.preds[0] == first + want);
    }
    if (S == 2) CHECK(load[0] == 2500 && load[1] == 2500);
    if (S == 3) CHECK(load[0] == 2500 && load[1] == 1250 && load[2] == 1250);
    if (S == 4) CHECK(load[0] == 1250 && load[1] == 1250 && load[2] == 1250 && load[3] == 1250);
    CHECK((int)sim.st.frontier().size() == S);
    // a caller node behind it follows every tail
    const int end = sim.caller_node();
    CHECK((int)sim.g[end].preds.size() == S);
}

static Footprint set_fp(int k, int k_alpha = -1) {   // output set k (alpha of set k_alpha), inputs of their own
    const int64_t W = 64;
    char *mem = (char *)0x50000000;
    double *out = (double *)(mem + 0x4000000 + 0x10000 * k), *al = (double *)(mem + 0x6000000 + 0x10000 * (k_alpha < 0 ? k : k_alpha));
    return fp_of(W, 5, mem + 0x20000 * (k % 7), nullptr, mem + 0x2000000 + 0x1000 * (k % 7), nullptr, out, al);
}
static void test_fixed_patterns(int S) {
    {   // all calls into one output set: one strand is used, a chain
        Sim<Strands<int>> sim(S, true);
        const int base = sim.caller_node();
        for (int i = 0; i < 40; i++) {
            const int id = sim.lib_call(set_fp(0));
            CHECK(sim.g[id].strand == 0 && sim.g[id].preds.size() == 1 && sim.g[id].preds[0] == (i ? id - 1 : base));
            CHECK(sim.st.frontier().size() == 1);
        }
        CHECK(sim.joins == 0 && sim.check_invariant() == 0);
    }
    {   // all calls disjoint, n output sets for n calls: a strict round-robin, call i behind call i - S
        Sim<Strands<int>> sim(S, true);
        const int base = sim.caller_node();
        const int n = 12;   // (12 sets x 2 output ranges stay below the write capacity of 32 even on one strand)
        for (int i = 0; i < n; i++) {
            const int id = sim.lib_call(set_fp(i));
            CHECK(sim.g[id].strand == i % S && sim.g[id].preds.size() == 1 && sim.g[id].preds[0] == (i < S ? base : id - S));
        }
        CHECK(sim.joins == 0);
        const int un = sim.check_invariant();
        int want = 0;   // pairs on different strands
        for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) want += (i % S != j % S);
        CHECK(un == want);
    }
    if (S >= 2) {   // one call conflicting with two strands: one join with as many in-edges as there are non-empty strands
        for (int filled = 2; filled <= S; filled++) {
            Sim<Strands<int>> sim(S, true);
            sim.caller_node();
            std::vector<int> ids;
            for (int i = 0; i < filled; i++) ids.push_back(sim.lib_call(set_fp(i)));
            const int j = sim.lib_call(set_fp(0, 1));   // DT of set 0, alpha of set 1
            CHECK(sim.g[j].join && (int)sim.g[j].preds.size() == filled && sim.joins == 1);
            for (int i = 0; i < filled; i++) {
                bool found = false;
                for (int p : sim.g[j].preds) found = found || p == ids[i];
                CHECK(found);
            }
            for (int i = 0; i < S; i++) {   // the next S calls all hang off it
                const int id = sim.lib_call(set_fp(10 + i));
                CHECK(sim.g[id].preds.size() == 1 && sim.g[id].preds[0] == j && sim.g[id].strand == i);
            }
            const int id = sim.lib_call(set_fp(20));
            CHECK(sim.g[id].preds.size() == 1 && sim.g[id].preds[0] == j + 1);
            CHECK(sim.joins == 1);
            sim.check_invariant();
        }
    }
    if (S >= 2) {   // an unknown call while two strands are in use joins them; with one strand in use it just follows that strand
        Sim<Strands<int>> sim(S, true);
        sim.caller_node();
        const Footprint csr = fp_of(64, 5, (void *)0x1000, (void *)0x2000, (void *)0x3000, nullptr, (double *)0x4000, (double *)0x5000);
        CHECK(csr.unknown);
        const int a = sim.lib_call(set_fp(0));
        const int u = sim.lib_call(csr);
        CHECK(!sim.g[u].join && sim.g[u].preds.size() == 1 && sim.g[u].preds[0] == a);
        const int b = sim.lib_call(set_fp(1));   // whatever it touches, it conflicts with the strand that holds the unknown call
        CHECK(!sim.g[b].join && sim.g[b].preds[0] == u && sim.st.frontier().size() == 1);
        sim.new_capture();
        sim.lib_call(set_fp(0));
        sim.lib_call(set_fp(1));
        const int u2 = sim.lib_call(csr);
        CHECK(sim.g[u2].join && sim.g[u2].preds.size() == 2);
        sim.check_invariant();
    }
}

int main() {
    test_rangeset();
    test_policy();
    Tally shipped, small;
    for (int S = 1; S <= 4; S++)
        for (int seq = 0; seq < 200; seq++) {
            run_sequence<Strands<int>>(20250917u + 1000u * (uint64_t)S + (uint64_t)seq, S, true, 6, shipped);
            // 4 ranges per summary: overflow joins occur (12 output sets: 2 write ranges per call)
            run_sequence<Strands<int, 4, 4>>(31337u + 1000u * (uint64_t)S + (uint64_t)seq, S, false, 12, small);
        }
    CHECK(shipped.overflow == 0 && shipped.joins > 0 && shipped.unordered > 0);
    CHECK(small.overflow > 0 && small.unordered > 0);
    for (int S = 1; S <= 4; S++) test_fixed_patterns(S);
    for (int S = 2; S <= 4; S++) test_headline_walk(S);
    if (g_fail) { printf("test_capture_strands_cpu: %d checks FAILED\n", g_fail); return 1; }
    printf("test_capture_strands_cpu ok (%lld calls, %lld unordered pairs, %lld joins; small summaries: %lld joins, %lld by overflow)\n",
           shipped.calls, shipped.unordered, shipped.joins, small.joins, small.overflow);
    return 0;
}
