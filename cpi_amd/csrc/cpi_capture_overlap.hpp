// cpi_capture_overlap.hpp -- which captured cpi_preintegrate_batch calls may run unordered in a HIP graph, decided on the host.
// Plain C++ (no HIP): cpi_abi.hip drives it with hipGraphNode_t, tests/cpp/test_capture_overlap_cpu.cpp and
// tests/cpp/test_capture_strands_cpu.cpp with fake node ids.
//
// Three parts:
//   Footprint  the byte ranges a call reads and writes, and the conflict test between two calls;
//   Window     the bookkeeping of consecutive eligible calls captured on one stream: the predecessors of the next call and
//              the dependency set ("frontier") the stream is left with after it -- the look-back shape, an opt-in;
//   Strands    the same bookkeeping for the shape a context starts with: one chain per strand (at the end of this file).
// The rule: call i of a window may be unordered only with calls i-1 ... i-D+1, and only
// with those whose footprint is disjoint from its own; it has a path from every earlier call of the window and from the
// base (the stream's dependency set when the window opened).  Realised with at most 2D-1 edges per call:
//   required(i) = { i-2D+1 ... i-D }  u  { j in i-D+1 ... i-1 : conflict(j, i) }
//   preds(i)    = required(i) less the calls another chosen predecessor already has a path from; the base when none is left
//   frontier(i) = { i-D+1 ... i } less the calls a later one of them has a path from
// Call i-D has (by induction) a path from everything up to i-2D, so required(i) covers every call up to i-D; every call has a
// path from the base; whatever is captured behind the frontier has a path from every call of the window and from the base.
// All calls disjoint: D edges per call and D nodes in the frontier.  All calls conflicting: a chain, one node in the frontier.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

namespace cpi {
namespace overlap {

constexpr int kMaxDepth = 4;
constexpr int kDefaultDepth = 2;   // of the look-back shape; measured: profiles/capture_overlap.md (3 and 4 are slower than the serial shape)
inline int clamp_depth(long long d) { return d < 1 ? 1 : (d > kMaxDepth ? kMaxDepth : (int)d); }

// What a new context starts with; read ONCE per context, at its creation -- no launch path reads the environment.
//   GPU_MAX_HW_QUEUES        (the runtime's own variable; never set here)  below 4: parallel branches of a graph are not safe
//                            to replay, the context keeps depth 1 whatever else is asked (allowed = false)
//   CPI_AMD_CAPTURE_OVERLAP  the depth, clamped to [1, kMaxDepth]; unset or empty: kDefaultDepth
struct Policy {
    bool allowed;
    int depth;
};
inline Policy policy_from(const char *hw_queues, const char *depth) {
    Policy p;
    p.allowed = !(hw_queues && *hw_queues && atoll(hw_queues) < 4);
    p.depth = p.allowed ? clamp_depth(depth && *depth ? atoll(depth) : kDefaultDepth) : 1;
    return p;
}
inline Policy policy_from_environment() { return policy_from(getenv("GPU_MAX_HW_QUEUES"), getenv("CPI_AMD_CAPTURE_OVERLAP")); }

// Which launches have something to hide.  Up to one wavefront per SIMD (1 024 on the MI355X -- the boundary pick_lanes in
// cpi_abi.hip splits windows over lanes by) a launch lasts as long as ONE wavefront's chain of memory round trips, and the memory
// system idles during every wavefront's head and tail: the regime the overlap was measured to pay in (10 000 x 50, 1 000
// wavefronts: 11.2 -> 9.3 us per step).  A launch of many rounds of wavefronts fills those gaps by itself; at 1 M windows the
// overlap was measured 0-3 % slower than the chain in three rounds of three.  Such launches keep the serial shape.
constexpr long long kLatencyBoundWavefronts = 1024;
inline bool launch_is_latency_bound(long long wavefronts) { return wavefronts <= kLatencyBoundWavefronts; }

// A caller that spreads its calls over several contexts inside ONE capture (one stream each, forked and joined by events) has
// built the overlap by hand; relaxing each of those streams as well multiplies the branches and is slower than either alone
// (profiles/capture_overlap.md).  One process-wide slot remembers which context asked first in the capture seen last: as soon
// as a second context asks in the same capture, every context keeps the serial shape for the rest of it.  A matter of speed
// only -- the slot decides whether a window is used at all, never what is ordered inside one.
class CaptureRegistry {
public:
    // true: `ctx` is (still) the only context seen in capture `id`
    bool sole(unsigned long long id, const void *ctx) {
        std::lock_guard<std::mutex> lock(m_);
        if (!valid_ || id != id_) { valid_ = true; id_ = id; owner_ = ctx; shared_ = false; }
        else if (owner_ != ctx) shared_ = true;
        return !shared_;
    }

private:
    std::mutex m_;
    bool valid_ = false, shared_ = false;
    unsigned long long id_ = 0;
    const void *owner_ = nullptr;
};
inline CaptureRegistry &capture_registry() { static CaptureRegistry r; return r; }

// [lo, hi) in bytes; empty when hi <= lo.  An empty range overlaps nothing.
struct Range {
    uintptr_t lo, hi;
};
inline Range make_range(const void *p, uint64_t bytes) {
    const uintptr_t lo = (uintptr_t)p;
    if (!p || bytes == 0) return {lo, lo};
    const uintptr_t room = UINTPTR_MAX - lo;
    return {lo, bytes > room ? UINTPTR_MAX : lo + (uintptr_t)bytes};   // saturates: a range that would wrap reaches the top
}
inline bool ranges_overlap(const Range &a, const Range &b) {
    return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi;
}

constexpr int kMaxReads = 5, kMaxWrites = 13;
struct Footprint {
    bool unknown = true;   // the host cannot bound what the call touches: conflicts with every call
    int nr = 0, nw = 0;
    Range r[kMaxReads], w[kMaxWrites];
};
// The arrays of one cpi_preintegrate_batch call (include/cpi_amd.h).  out[k] / out_doubles[k]: the nout output arrays and
// their doubles per window; NULL = not written.  A CSR `first` array places the windows anywhere in `knots`: unknown span.
inline Footprint make_footprint(int64_t W, int32_t N, const void *knots, const void *first, const void *count, const void *lin,
                                const void *q_k_lin, const void *const *out, const int *out_doubles, int nout) {
    Footprint f;
    if (first || W <= 0 || N < 0 || nout > kMaxWrites) return f;
    f.unknown = false;
    const uint64_t w = (uint64_t)W;
    f.r[f.nr++] = make_range(knots, w * ((uint64_t)N + 1) * 7 * 8);
    f.r[f.nr++] = make_range(lin, w * 6 * 8);
    if (q_k_lin) f.r[f.nr++] = make_range(q_k_lin, w * 4 * 8);
    if (count) f.r[f.nr++] = make_range(count, w * 4);
    for (int k = 0; k < nout; k++)
        if (out[k]) f.w[f.nw++] = make_range(out[k], w * (uint64_t)out_doubles[k] * 8);
    return f;
}
// write/write, read/write or write/read overlap of any two ranges
inline bool conflict(const Footprint &a, const Footprint &b) {
    if (a.unknown || b.unknown) return true;
    for (int i = 0; i < a.nw; i++) {
        for (int j = 0; j < b.nw; j++) if (ranges_overlap(a.w[i], b.w[j])) return true;
        for (int j = 0; j < b.nr; j++) if (ranges_overlap(a.w[i], b.r[j])) return true;
    }
    for (int i = 0; i < a.nr; i++)
        for (int j = 0; j < b.nw; j++) if (ranges_overlap(a.r[i], b.w[j])) return true;
    return false;
}

template <class Node>
inline bool same_set(const std::vector<Node> &a, const Node *b, size_t nb) {
    if (a.size() != nb) return false;
    for (size_t i = 0; i < nb; i++) {
        bool found = false;
        for (size_t j = 0; j < a.size() && !found; j++) found = a[j] == b[i];
        if (!found) return false;
    }
    return true;   // (neither side holds a node twice: equal sizes + inclusion = equality)
}

template <class Node>
class Window {
public:
    bool is_open() const { return open_; }
    void close() { open_ = false; }
    long long calls() const { return n_; }
    const std::vector<Node> &base() const { return base_; }
    const std::vector<Node> &frontier() const { return frontier_; }

    // Does a call captured now continue this window?  Only when it belongs to the same capture and the stream's dependency
    // set is exactly the frontier the previous call left: anything else was captured in between.
    bool continues(unsigned long long capture_id, const Node *deps, size_t ndeps) const {
        return open_ && capture_id == id_ && same_set(frontier_, deps, ndeps);
    }
    void open_at(unsigned long long capture_id, int depth, const Node *deps, size_t ndeps) {
        open_ = true; id_ = capture_id; depth_ = clamp_depth(depth); n_ = 0;
        base_.assign(deps, deps + ndeps);
        frontier_ = base_;
    }
    // The predecessors of the next call, whose footprint is fp: call i-d is REQUIRED when d >= D or the footprints conflict.
    // Candidates are taken from the newest (d = 1) to d = 2D-1 and skipped when a predecessor chosen before already has a path
    // from them -- anc bit d of a call says "call i-d is an ancestor"; a chosen i-d brings its own ancestors and, by the
    // induction above, every call up to i-d-D.  Calls beyond 2D-1 are ancestors of i-D.  The base is needed only when no call
    // of the window was chosen: each of them has a path from it.
    void plan(const Footprint &fp, std::vector<Node> &preds) {
        preds.clear();
        const long long i = n_, D = depth_;
        uint32_t anc = 0;
        for (long long d = 1; d <= 2 * D - 1 && d <= i; d++) {
            const long long j = i - d;
            if ((anc >> d) & 1u) continue;
            if (d < D && !conflict(fp_[j % kRing], fp)) continue;
            preds.push_back(node_[j % kRing]);
            anc |= (1u << d) | (anc_[j % kRing] << d) | (~0u << (d + D));
        }
        if (preds.empty()) preds = base_;
        pending_anc_ = anc;
    }
    // The call plan() was asked about was captured as `node`; frontier() is what the stream is to be left with: the last D
    // calls, less those a later one of them has a path from.
    void commit(Node node, const Footprint &fp) {
        node_[n_ % kRing] = node; fp_[n_ % kRing] = fp; anc_[n_ % kRing] = pending_anc_;
        n_++;
        frontier_.clear();
        for (long long j = n_ - 1; j >= 0 && j >= n_ - depth_; j--) {
            bool covered = false;
            for (long long l = j + 1; l < n_ && !covered; l++) covered = (anc_[l % kRing] >> (l - j)) & 1u;
            if (!covered) frontier_.push_back(node_[j % kRing]);
        }
    }

private:
    static constexpr int kRing = 2 * kMaxDepth;   // plan() looks back 2D-1 calls
    bool open_ = false;
    unsigned long long id_ = 0;
    int depth_ = 1;
    long long n_ = 0;   // calls in the window
    std::vector<Node> base_, frontier_;
    Node node_[kRing] = {};
    Footprint fp_[kRing];
    uint32_t anc_[kRing] = {}, pending_anc_ = 0;   // bit d: the call d before this one is an ancestor (d < 32)
};

// ---- strands: one chain of calls per strand, no cross edges except at joins --------------------------------------
// The look-back rule above makes every node of an all-disjoint walk join D branches; measured, those cross-branch edges cost
// more than a third launch in flight returns.  Strands keep the same two guarantees with ONE in-edge per call:
//   summary    per strand, the union of what its calls have read / written since the window opened or was last joined, as two
//              RangeSets of fixed capacity: look-back unbounded in calls, bounded in memory, nothing allocated per call;
//   placement  a call that conflicts with no strand's summary goes to the least recently extended strand (empty ones first);
//              one that conflicts with exactly one strand goes behind that strand's tail; one that conflicts with several
//              strands, or is unknown while several are non-empty, or whose ranges no longer fit the summary, is a JOIN: its
//              predecessors are the tails of all non-empty strands, and the window restarts behind it (base = {the join});
//   preds      of any other call: its strand's tail, or the base while the strand is empty;
//   frontier   the tails of the non-empty strands; the base while there is none.
// Two calls without a path between them lie on different strands of one window between two joins, so neither conflicted with
// the other's strand summary when it was placed: their footprints are disjoint.  Everything behind a join descends from it.
constexpr int kMaxStrands = 4;
constexpr int kReadRanges = 64, kWriteRanges = 32;
inline int clamp_strands(long long n) { return n < 1 ? 1 : (n > kMaxStrands ? kMaxStrands : (int)n); }

// A sorted array of coalesced byte ranges: overlapping, touching and identical ranges merge, so no two entries share or touch.
template <int Cap>
class RangeSet {
public:
    int size() const { return n_; }
    const Range &operator[](int i) const { return r_[i]; }
    void clear() { n_ = 0; }
    bool overlaps(const Range &x) const {
        if (x.hi <= x.lo) return false;
        int i = 0;
        while (i < n_ && r_[i].hi <= x.lo) i++;   // (entries are disjoint and sorted: the first one that ends behind x.lo decides)
        return i < n_ && r_[i].lo < x.hi;
    }
    // false: the set is full and x starts a new entry -- nothing was changed
    bool add(const Range &x) {
        if (x.hi <= x.lo) return true;
        int i = 0;
        while (i < n_ && r_[i].hi < x.lo) i++;    // [i, j): the entries x overlaps or touches
        int j = i;
        while (j < n_ && r_[j].lo <= x.hi) j++;
        if (i == j) {
            if (n_ == Cap) return false;
            for (int k = n_; k > i; k--) r_[k] = r_[k - 1];
            r_[i] = x;
            n_++;
            return true;
        }
        Range m = {x.lo < r_[i].lo ? x.lo : r_[i].lo, x.hi > r_[j - 1].hi ? x.hi : r_[j - 1].hi};
        r_[i] = m;
        for (int k = j; k < n_; k++) r_[i + 1 + (k - j)] = r_[k];
        n_ -= j - i - 1;
        return true;
    }

private:
    int n_ = 0;
    Range r_[Cap];
};

// RCap / WCap: the summaries' capacities (the test instantiates a small one so that overflow joins occur)
template <class Node, int RCap = kReadRanges, int WCap = kWriteRanges>
class Strands {
public:
    bool is_open() const { return open_; }
    void close() { open_ = false; }
    long long calls() const { return n_; }
    long long joins() const { return joins_; }
    int last_strand() const { return last_; }   // where the call committed last went; -1: it was a join
    const std::vector<Node> &base() const { return base_; }
    const std::vector<Node> &frontier() const { return frontier_; }

    bool continues(unsigned long long capture_id, const Node *deps, size_t ndeps) const {
        return open_ && capture_id == id_ && same_set(frontier_, deps, ndeps);
    }
    void open_at(unsigned long long capture_id, int strands, const Node *deps, size_t ndeps) {
        open_ = true; id_ = capture_id; S_ = clamp_strands(strands); n_ = 0; joins_ = 0; last_ = -1;
        base_.assign(deps, deps + ndeps);
        restart();
    }
    void plan(const Footprint &fp, std::vector<Node> &preds) {
        preds.clear();
        int hit = -1, nhit = 0, nonempty = 0, lru = 0;
        for (int s = 0; s < S_; s++) {
            if (!st_[s].empty) nonempty++;
            if (conflicts(st_[s], fp)) { nhit++; hit = s; }
            if (st_[s].stamp < st_[lru].stamp) lru = s;   // (empty strands carry stamp 0: they come first, lowest index first)
        }
        target_ = nhit == 0 ? lru : hit;
        if (nhit >= 2 || (fp.unknown && nonempty >= 2)) target_ = -1;
        if (target_ >= 0) {   // the summary as it would be: kept aside, the strand's own stays untouched until commit
            pending_ = st_[target_];
            pending_.everything = pending_.everything || fp.unknown;
            bool fits = true;
            if (!fp.unknown) {
                for (int k = 0; k < fp.nr && fits; k++) fits = pending_.reads.add(fp.r[k]);
                for (int k = 0; k < fp.nw && fits; k++) fits = pending_.writes.add(fp.w[k]);
            }
            if (!fits) target_ = -1;
        }
        if (target_ >= 0) {
            if (!st_[target_].empty) preds.push_back(st_[target_].tail);
        } else {
            for (int s = 0; s < S_; s++) if (!st_[s].empty) preds.push_back(st_[s].tail);
        }
        if (preds.empty()) preds = base_;
    }
    void commit(Node node, const Footprint &) {
        n_++;
        last_ = target_;
        if (target_ < 0) {
            joins_++;
            base_.assign(1, node);
            restart();
            return;
        }
        st_[target_] = pending_;
        st_[target_].empty = false; st_[target_].tail = node; st_[target_].stamp = ++clock_;
        frontier_.clear();
        for (int s = 0; s < S_; s++) if (!st_[s].empty) frontier_.push_back(st_[s].tail);
    }

private:
    struct Strand {
        bool empty = true, everything = false;   // everything: holds a call of unknown footprint -- conflicts with every call
        Node tail = Node();
        unsigned long long stamp = 0;            // when it was extended last (0: not since the window restarted)
        RangeSet<RCap> reads;
        RangeSet<WCap> writes;
    };
    static bool conflicts(const Strand &s, const Footprint &fp) {
        if (s.empty) return false;
        if (s.everything || fp.unknown) return true;
        for (int k = 0; k < fp.nw; k++) if (s.reads.overlaps(fp.w[k]) || s.writes.overlaps(fp.w[k])) return true;
        for (int k = 0; k < fp.nr; k++) if (s.writes.overlaps(fp.r[k])) return true;
        return false;
    }
    void restart() {
        for (int s = 0; s < kMaxStrands; s++) { st_[s].empty = true; st_[s].everything = false; st_[s].stamp = 0; st_[s].reads.clear(); st_[s].writes.clear(); }
        clock_ = 0;
        frontier_ = base_;
    }

    bool open_ = false;
    unsigned long long id_ = 0, clock_ = 0;
    int S_ = 1, target_ = -1, last_ = -1;
    long long n_ = 0, joins_ = 0;
    std::vector<Node> base_, frontier_;
    Strand st_[kMaxStrands], pending_;
};

// Which shape a new context captures with; read ONCE per context, at its creation (policy_from above stays the look-back
// shape's own reading of its variable).
//   GPU_MAX_HW_QUEUES below 4     serial for good (allowed = false, n = 1)
//   CPI_AMD_CAPTURE_STRANDS set   strands, clamped to [1, kMaxStrands]
//   CPI_AMD_CAPTURE_OVERLAP set   otherwise: the look-back shape at that depth, clamped to [1, kMaxDepth]
//   neither                       kDefaultShape at kDefaultStrands / kDefaultDepth
enum Shape { kShapeLookback = 0, kShapeStrands = 1 };
constexpr int kDefaultStrands = 4;   // measured: profiles/capture_strands.md (the fastest on the headline, not slower than 2 on twelve disjoint sets)
constexpr Shape kDefaultShape = kShapeStrands;
struct CapturePolicy {
    bool allowed;
    Shape shape;
    int n;   // strands, or the look-back depth; 1 = the serial chain in either shape
};
inline CapturePolicy capture_policy_from(const char *hw_queues, const char *strands, const char *depth) {
    if (hw_queues && *hw_queues && atoll(hw_queues) < 4) return {false, kDefaultShape, 1};
    if (strands && *strands) return {true, kShapeStrands, clamp_strands(atoll(strands))};
    if (depth && *depth) return {true, kShapeLookback, clamp_depth(atoll(depth))};
    return {true, kDefaultShape, kDefaultShape == kShapeStrands ? kDefaultStrands : kDefaultDepth};
}
inline CapturePolicy capture_policy_from_environment() {
    return capture_policy_from(getenv("GPU_MAX_HW_QUEUES"), getenv("CPI_AMD_CAPTURE_STRANDS"), getenv("CPI_AMD_CAPTURE_OVERLAP"));
}

}  // namespace overlap
}  // namespace cpi
