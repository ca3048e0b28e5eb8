// cpi_capture_overlap.hpp -- which captured cpi_preintegrate_batch calls may run unordered in a HIP graph, decided on the host.
// Plain C++ (no HIP): cpi_abi.hip drives it with hipGraphNode_t, tests/cpp/test_capture_overlap_cpu.cpp with fake node ids.
//
// Two parts:
//   Footprint  the byte ranges a call reads and writes, and the conflict test between two calls;
//   Window     the bookkeeping of consecutive eligible calls captured on one stream: the predecessors of the next call and
//              the dependency set ("frontier") the stream is left with after it.
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
constexpr int kDefaultDepth = 2;   // measured: profiles/capture_overlap.md (3 and 4 are slower than the serial shape)
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

}  // namespace overlap
}  // namespace cpi
