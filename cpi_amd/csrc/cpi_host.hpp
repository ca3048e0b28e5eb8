// cpi_host.hpp -- C++ host facade above the C-ABI (include/cpi_amd.h), shaped like the reference's
// classes so caller code written like GraphSolver_IMU.cpp:43-75 / 97-130 keeps its structure:
//
//   cpi_host::CpiV1 cpi(sigma_g, sigma_wg, sigma_a, sigma_wa);          // CpiV1.h:55
//   cpi.setLinearizationPoints(bg_K, ba_K, q_K, gravity);               // CpiBase.h:73
//   while (...) cpi.feed_IMU(t0, t1, w0, a0, w1, a1);                   // CpiBase.h:86
//   use cpi.DT, cpi.alpha_tau, cpi.beta_tau, cpi.q_k2tau, cpi.J_q ... cpi.P_meas   // CpiBase.h:99-124
//
// Differences forced by the device boundary: feed_IMU() only records the interval; the recursion runs on the GPU when a
// result member is READ (round 5: the members are lazy -- code shaped like GraphSolver_IMU.cpp:43-75 compiles unchanged, no
// finalize() between the feed_IMU loop and `ImuFactorCPIv1(..., cpi.P_meas, cpi.DT, cpi.grav, cpi.alpha_tau, ...)`), when
// finalize(ctx) is called, or through CpiBatch, which flushes many windows in one launch -- the intended use for more than a
// handful of windows.  Matrices are plain column-major arrays (Eigen::Map them if needed).
// Header-only; link with -lcpi_amd.  No CPU fallback: errors throw std::runtime_error.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cpi_amd.h"

namespace cpi_host {

typedef std::array<double, 3> Vec3;
typedef std::array<double, 4> Vec4;
typedef std::array<double, 9> Mat3;      // column-major
typedef std::array<double, 225> Mat15;   // column-major

class Context {
public:
    explicit Context(int device = -1, void *stream = nullptr) {
        if (cpi_ctx_create(device, stream, &ctx_) != CPI_OK) throw std::runtime_error(cpi_last_error(nullptr));
    }
    ~Context() { cpi_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    cpi_ctx *get() const { return ctx_; }
    void check(int rc) const { if (rc != CPI_OK) throw std::runtime_error(cpi_last_error(ctx_)); }
private:
    cpi_ctx *ctx_ = nullptr;
};

// A set of devices of this process (include/cpi_amd.h "Device sets"): one context + stream + RCCL rank per GPU.
// Windows shard as contiguous blocks (bounds(W, r)); every rank runs the ordinary entries on ctx(r) with pointers into
// its own device's memory; gather() is the one exchange step (each peer sends its output slab straight to the root).
class DeviceGroup {
public:
    explicit DeviceGroup(int n, const int *devices = nullptr) {
        if (cpi_group_create(n, devices, &g_) != CPI_OK) throw std::runtime_error(cpi_group_last_error(nullptr));
    }
    explicit DeviceGroup(cpi_group *adopt) : g_(adopt) { if (!g_) throw std::runtime_error("DeviceGroup: null group"); }   // takes ownership
    ~DeviceGroup() { cpi_group_destroy(g_); }
    DeviceGroup(const DeviceGroup &) = delete;
    DeviceGroup &operator=(const DeviceGroup &) = delete;
    DeviceGroup(DeviceGroup &&o) noexcept : g_(o.g_) { o.g_ = nullptr; }
    int size() const { return cpi_group_size(g_); }
    cpi_ctx *ctx(int rank) const { return cpi_group_ctx(g_, rank); }
    void bounds(int64_t W, int rank, int64_t &lo, int64_t &hi) const { cpi_shard_bounds(W, rank, size(), &lo, &hi); }
    void check(int rc) const { if (rc != CPI_OK) throw std::runtime_error(cpi_group_last_error(g_)); }
    void gather(int root, int64_t W, const cpi_outputs *local, const cpi_outputs &root_out) { check(cpi_group_gather(g_, root, W, local, &root_out)); }
    // The exchange inside ONE batch (include/cpi_amd.h: cpi_group_gather_chunk): every block in `chunks` sub-blocks
    // (chunk_bounds), sub-block c on the wire -- on the group's exchange streams -- while the kernels of sub-block c + 1 run.
    //   for (c = 0; c < chunks; c++) { for every rank r: enqueue the entries for chunk_bounds(W, r, c, chunks) on ctx(r);
    //                                  gather_chunk(root, W, c, chunks, local_c, root_out); }      // the last call joins
    void chunk_bounds(int64_t W, int rank, int chunk, int chunks, int64_t &lo, int64_t &hi) const { cpi_shard_chunk_bounds(W, rank, size(), chunk, chunks, &lo, &hi); }
    void gather_chunk(int root, int64_t W, int chunk, int chunks, const cpi_outputs *local_chunk, const cpi_outputs &root_out) {
        check(cpi_group_gather_chunk(g_, root, W, chunk, chunks, local_chunk, &root_out));
    }
    void synchronize() { check(cpi_group_synchronize(g_)); }
    int last_gather_messages() const { return cpi_group_last_gather_messages(g_); }   // per peer; 1 = slab path
private:
    cpi_group *g_ = nullptr;
};

// Results of one window: the public members of CpiBase / CpiV2, as plain values.
struct CpiResult {
    double DT = 0;
    Vec3 alpha_tau{}, beta_tau{};
    Vec4 q_k2tau{{0, 0, 0, 1}};
    Mat3 J_q{}, J_a{}, J_b{}, H_a{}, H_b{}, O_a{}, O_b{};
    Mat15 P_meas{};
};

// The context a lazy read runs on when the preintegrator was not bound to one (CpiBase::bind): one per THREAD, on the device
// that is current when the thread first reads a result.  Calls on one context are not re-entrant, and the reference's result
// members are plain per-object data that different threads may read side by side -- so reads of DIFFERENT preintegrators from
// different threads each use their own thread's context (stream, staging) and do not race.  ONE preintegrator read from two
// threads at once is still a data race on its members the first time (the read runs the recursion and stores the results):
// read it once before sharing it, or guard it -- INTEGRATION.md section 3.
inline const Context &default_context() {
    static thread_local Context ctx;
    return ctx;
}

class CpiBase;
// A result member of CpiBase (CpiBase.h:99-124: DT, alpha_tau, ... P_meas).  The reference's members are live after every
// feed_IMU; here the recorded intervals run on the GPU the first time ANY member is read after a feed_IMU (one launch for the
// whole window so far), so caller code keeps the reference's shape.  Reading = conversion to const T &, get(), and for the
// array members operator[], begin() / end(), data().  Assignment stores a value and runs nothing.
template <class T>
class Lazy {
public:
    explicit Lazy(const CpiBase *owner, const T &init = T{}, bool mean = false) : v_(init), owner_(owner), mean_(mean) {}
    Lazy(const Lazy &) = delete;                       // members of ONE preintegrator: CpiBase's copy operations re-bind them
    Lazy &operator=(const Lazy &) = delete;
    Lazy &operator=(const T &v) { v_ = v; return *this; }
    operator const T &() const { sync(); return v_; }
    const T &get() const { sync(); return v_; }
    template <class U = T> auto operator[](size_t i) const -> decltype(std::declval<const U &>()[i]) { sync(); return v_[i]; }
    template <class U = T> auto begin() const -> decltype(std::declval<const U &>().begin()) { sync(); return v_.begin(); }
    template <class U = T> auto end() const -> decltype(std::declval<const U &>().end()) { sync(); return v_.end(); }
    template <class U = T> auto data() const -> decltype(std::declval<const U &>().data()) { sync(); return v_.data(); }
    template <class U = T> auto size() const -> decltype(std::declval<const U &>().size()) { return v_.size(); }
private:
    friend class CpiBase;
    inline void sync() const;
    T v_;
    const CpiBase *owner_;
    bool mean_;            // one of DT / alpha_tau / beta_tau / q_k2tau: valid after a mean-only flush
};

class CpiBase {
public:
    CpiBase(int model, double sigma_w, double sigma_wb, double sigma_a, double sigma_ab, bool imu_avg_ = false)
        : imu_avg(imu_avg_), model_(model) { sig_[0] = sigma_w; sig_[1] = sigma_wb; sig_[2] = sigma_a; sig_[3] = sigma_ab; }
    CpiBase(const CpiBase &o) { *this = o; }
    CpiBase &operator=(const CpiBase &o) {
        if (this == &o) return *this;
        imu_avg = o.imu_avg; state_transition_jacobians = o.state_transition_jacobians;
        b_w_lin = o.b_w_lin; b_a_lin = o.b_a_lin; q_k_lin = o.q_k_lin; grav = o.grav;
        knots_ = o.knots_; model_ = o.model_; ctx_ = o.ctx_; dirty_ = o.dirty_; means_only_ = o.means_only_;
        incremental_ = o.incremental_; carry_ = o.carry_; fed_ = o.fed_;
        for (int i = 0; i < 4; i++) sig_[i] = o.sig_[i];
        put(o.peek());
        return *this;
    }
    virtual ~CpiBase() {}
    // the context lazy reads run on (default: default_context()); the Context must outlive the reads
    void bind(const Context &ctx) { ctx_ = &ctx; }
    // Like the reference (CpiBase.h:73-80, which only stores the values; the recursion reads them at every feed_IMU), the
    // linearisation point belongs BEFORE the first feed_IMU.  Here the recursion runs at the first read, with the values current
    // then; a call after results were read marks them stale, so the next read recomputes the window at the new point (the
    // reference would keep integrating the old prefix with the old point -- a use it never makes).  Assigning the public members
    // b_w_lin / b_a_lin / q_k_lin / grav / imu_avg directly is NOT tracked: call invalidate() afterwards.
    void setLinearizationPoints(const Vec3 &b_w_lin_, const Vec3 &b_a_lin_, const Vec4 &q_k_lin_ = Vec4{{0, 0, 0, 0}},
                                const Vec3 &grav_ = Vec3{{0, 0, 0}}) {
        if (incremental_ && !carry_.empty())
            throw std::logic_error("setLinearizationPoints: an incremental preintegrator has already integrated intervals at the old point");
        b_w_lin = b_w_lin_; b_a_lin = b_a_lin_; q_k_lin = q_k_lin_; grav = grav_;
        if (!knots_.empty()) dirty_ = true;
    }
    void invalidate() { if (!knots_.empty()) dirty_ = true; }
    // Records interval [t_0, t_1] with readings (w_m_0, a_m_0) at t_0 and (w_m_1, a_m_1) at t_1.
    // Differences from CpiV1::feed_IMU / CpiV2::feed_IMU (CpiV1.h:62-74):
    //  * t_1 - t_0 < 0: the reference's feed_IMU integrates the interval with the negative dt (only its caller,
    //    GraphSolver_IMU.cpp:52, skips it); here -- as in the C-ABI -- such an interval is SKIPPED, like dt == 0.
    //  * imu_avg == false: the closing reading (w_m_1, a_m_1) takes no part in the arithmetic (CpiV1.h:77-86), and callers
    //    written like the reference's non-averaging use leave it at its default.  The interval then chains to the previous
    //    one whenever the TIMES chain (t_0 == previous t_1): the previous closing knot is overwritten with (w_m_0, a_m_0)
    //    and every interval costs ONE knot (no NaN separator, no 3 knots per interval -- the N <= 65535 limit of a window
    //    would otherwise be reached after ~21 k calls).  Set imu_avg before the first feed_IMU.
    void feed_IMU(double t_0, double t_1, const Vec3 &w_m_0, const Vec3 &a_m_0, const Vec3 &w_m_1 = Vec3{{0, 0, 0}},
                  const Vec3 &a_m_1 = Vec3{{0, 0, 0}}) {
        const size_t n = knots_.size() / 7;
        bool chained = false;
        if (n) {
            double *k = &knots_[(n - 1) * 7];
            if (!imu_avg && k[0] == t_0) {   // times chain, closing readings unused: this interval's reading opens it
                for (int i = 0; i < 3; i++) { k[1 + i] = w_m_0[i]; k[4 + i] = a_m_0[i]; }
                chained = true;
                touch();
            } else {
                chained = k[0] == t_0 && k[1] == w_m_0[0] && k[2] == w_m_0[1] && k[3] == w_m_0[2] && k[4] == a_m_0[0] &&
                          k[5] == a_m_0[1] && k[6] == a_m_0[2];
            }
        }
        if (!chained) {
            // The reference's feed_IMU only ever uses t_1 - t_0, so intervals need not chain.  A knot whose
            // time is NaN is a separator: both intervals touching it have a NaN dt and are skipped by the kernels.
            if (n) push(std::numeric_limits<double>::quiet_NaN(), Vec3{{0, 0, 0}}, Vec3{{0, 0, 0}});
            push(t_0, w_m_0, a_m_0);
        }
        push(t_1, w_m_1, a_m_1);
        if (incremental_) fed_.push_back((int32_t)(knots_.size() / 7 - 1));   // read_rows: this interval's closing knot
    }
    // Incremental mode (cpi_preintegrate_resume): a read runs only the intervals fed since the previous read, continuing
    // from the carried state, and keeps only the last knot -- O(1) per read instead of re-running the window.  Switch it on
    // before the first feed_IMU; the linearisation point cannot change once intervals were integrated.  The carry record is
    // host memory, so a copy of the preintegrator continues on its own.  The Forster comparator cannot be resumed.
    void set_incremental(bool on) {
        if (on && model_ == CPI_MODEL_FORSTER) throw std::logic_error("set_incremental: the Forster comparator cannot be resumed");
        if (!knots_.empty() || !carry_.empty()) throw std::logic_error("set_incremental: call it before the first feed_IMU");
        incremental_ = on;
    }
    bool incremental() const { return incremental_; }
    // Incremental preintegrators only: the members as they stood after EVERY feed_IMU since the previous read
    // (cpi_preintegrate_running_resume_host) -- one CpiResult per fed interval, in order; a skipped interval (dt <= 0) repeats the
    // entry before it, and the NaN separator knots feed_IMU places between intervals that do not chain produce no entry.  The
    // carry and the tail knot advance exactly as in a member read, and the result members then equal the last entry.  Model 2: the
    // entries hold no bias Jacobians (there is no running form of them); the members' Jacobians are read out of the carried
    // state-transition columns by the next member read.
    std::vector<CpiResult> read_rows(const Context &ctx) {
        if (!incremental_) throw std::logic_error("read_rows: set_incremental(true) first (the rows continue from the carried state)");
        if (model_ == CPI_MODEL_V2 && !state_transition_jacobians)
            throw std::logic_error("read_rows: model 2's analytic Jacobians (state_transition_jacobians = false) have no running form");
        std::vector<CpiResult> res;
        if (fed_.empty()) return res;
        cpi_params p = params();
        const double lin[6] = { b_w_lin[0], b_w_lin[1], b_w_lin[2], b_a_lin[0], b_a_lin[1], b_a_lin[2] };
        const int32_t n = (int32_t)(knots_.size() / 7 - 1);
        const bool jac = model_ == CPI_MODEL_V1;
        const size_t M = (size_t)n;
        std::vector<double> DT_(M), al(M * 3), be(M * 3), q(M * 4), Jq(jac ? M * 9 : 0), Ja(jac ? M * 9 : 0), Jb(jac ? M * 9 : 0),
            Ha(jac ? M * 9 : 0), Hb(jac ? M * 9 : 0), P(M * 225);
        cpi_outputs o{};   // every running field, so that the carry holds every part a later read needs
        o.DT = DT_.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data(); o.P = P.data();
        if (jac) { o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data(); }
        std::vector<double> next(cpi_carry_doubles(model_));
        ctx.check(cpi_preintegrate_running_resume_host(ctx.get(), &p, 1, n, knots_.data(), nullptr, nullptr, n + 1, lin, q_k_lin.data(),
                                                       carry_.empty() ? nullptr : carry_.data(), next.data(), &o));
        carry_.swap(next);
        res.resize(fed_.size());
        for (size_t e = 0; e < fed_.size(); e++) {
            const size_t r = (size_t)fed_[e] - 1;
            CpiResult &x = res[e];
            x.DT = DT_[r];
            for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
            for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
            if (jac)
                for (int k = 0; k < 9; k++) {
                    x.J_q[k] = Jq[r * 9 + k]; x.J_a[k] = Ja[r * 9 + k]; x.J_b[k] = Jb[r * 9 + k];
                    x.H_a[k] = Ha[r * 9 + k]; x.H_b[k] = Hb[r * 9 + k];
                }
            for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
        }
        knots_.erase(knots_.begin(), knots_.end() - 7);   // the next segment starts on this one's last knot
        fed_.clear();
        set_result(res.back());
        if (!jac) dirty_ = true;                          // model 2: the next member read is a zero-interval resume (its Jacobians)
        return res;
    }
    std::vector<CpiResult> read_rows() { return read_rows(ctx_ ? *ctx_ : default_context()); }
    // Incremental preintegrators only: the measurement AT each of `times` -- a camera frame stamped inside the chunk that has just
    // been fed (cpi_query_open_batch_host).  Runs the intervals fed since the previous read; the carry and the tail knot advance
    // exactly as in read_rows().  One CpiResult per time: the means, P_meas, and model 1's five Jacobians or model 2's seven.  A
    // time on a fed stamp gives the members as they stood there, a time inside an interval that state advanced with the interval's
    // opening reading held, a time before the first pending interval the state at the previous read, a time at or past the last
    // stamp the current state.  The pending intervals must chain (a separator knot is refused by the library).
    std::vector<CpiResult> at(const Context &ctx, const std::vector<double> &times) {
        if (!incremental_) throw std::logic_error("at: set_incremental(true) first (the queries continue from the carried state)");
        if (model_ == CPI_MODEL_V2 && !state_transition_jacobians)
            throw std::logic_error("at: model 2's analytic Jacobians (state_transition_jacobians = false) have no running form");
        std::vector<CpiResult> res;
        if (times.empty()) return res;
        cpi_params p = params();
        const double lin[6] = { b_w_lin[0], b_w_lin[1], b_w_lin[2], b_a_lin[0], b_a_lin[1], b_a_lin[2] };
        const int32_t n = knots_.empty() ? 0 : (int32_t)(knots_.size() / 7 - 1);
        static const double zero_knot[7] = { 0, 0, 0, 0, 0, 0, 0 };
        const size_t Q = times.size();
        const bool v2 = model_ == CPI_MODEL_V2;
        std::vector<double> DT_(Q), al(Q * 3), be(Q * 3), q(Q * 4), Jq(Q * 9), Ja(Q * 9), Jb(Q * 9), Ha(Q * 9), Hb(Q * 9),
            Oa(v2 ? Q * 9 : 0), Ob(v2 ? Q * 9 : 0), P(Q * 225);
        const std::vector<int32_t> qwin(Q, 0);
        cpi_outputs o{};   // every field, so that the carry holds every part a later read needs
        o.DT = DT_.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data(); o.P = P.data();
        o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data();
        if (v2) { o.O_a = Oa.data(); o.O_b = Ob.data(); }
        std::vector<double> next(cpi_carry_doubles(model_));
        ctx.check(cpi_query_open_batch_host(ctx.get(), &p, 1, n, knots_.empty() ? zero_knot : knots_.data(), nullptr, nullptr, n + 1, lin,
                                            q_k_lin.data(), carry_.empty() ? nullptr : carry_.data(), next.data(), (int64_t)Q, qwin.data(),
                                            times.data(), &o));
        carry_.swap(next);
        res.resize(Q);
        for (size_t r = 0; r < Q; r++) {
            CpiResult &x = res[r];
            x.DT = DT_[r];
            for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
            for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
            for (int k = 0; k < 9; k++) {
                x.J_q[k] = Jq[r * 9 + k]; x.J_a[k] = Ja[r * 9 + k]; x.J_b[k] = Jb[r * 9 + k];
                x.H_a[k] = Ha[r * 9 + k]; x.H_b[k] = Hb[r * 9 + k];
                if (v2) { x.O_a[k] = Oa[r * 9 + k]; x.O_b[k] = Ob[r * 9 + k]; }
            }
            for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
        }
        if (n > 0) knots_.erase(knots_.begin(), knots_.end() - 7);   // the next segment starts on this one's last knot
        fed_.clear();
        dirty_ = true;   // the next member read is a zero-interval resume from the carried state
        return res;
    }
    std::vector<CpiResult> at(const std::vector<double> &times) { return at(ctx_ ? *ctx_ : default_context(), times); }
    // Runs this single window on the GPU and fills the result members (what a first read of any member does by itself).
    void finalize(const Context &ctx) {
        if (incremental_) { finalize_incremental(ctx); return; }
        cpi_params p = params();
        const double lin[6] = { b_w_lin[0], b_w_lin[1], b_w_lin[2], b_a_lin[0], b_a_lin[1], b_a_lin[2] };
        CpiResult r;
        cpi_outputs o = outputs_of(r);
        const int32_t n = knots_.empty() ? 0 : (int32_t)(knots_.size() / 7 - 1);
        static const double zero_knot[7] = { 0, 0, 0, 0, 0, 0, 0 };
        ctx.check(cpi_preintegrate_batch_host(ctx.get(), &p, 1, n, knots_.empty() ? zero_knot : knots_.data(), nullptr, nullptr,
                                              n + 1, lin, q_k_lin.data(), &o));
        set_result(r);
    }
    // the result members as plain values (runs the pending intervals first) / stored from outside (CpiBatch)
    CpiResult result() const { ensure(true); return peek(); }
    void set_result(const CpiResult &r) { put(r); dirty_ = false; means_only_ = false; }
    // CpiBatch::flush_means: only DT / alpha_tau / beta_tau / q_k2tau were computed.  The Jacobian and covariance members are
    // NOT valid for the recorded intervals: the first read of one of them runs the whole window (finalize), reads of the four
    // means do not.
    void set_means(double DT_, const Vec3 &alpha, const Vec3 &beta, const Vec4 &q) {
        DT.v_ = DT_; alpha_tau.v_ = alpha; beta_tau.v_ = beta; q_k2tau.v_ = q; dirty_ = false; means_only_ = true;
    }
    cpi_params params() const {
        cpi_params p{};
        p.sigma_w = sig_[0]; p.sigma_wb = sig_[1]; p.sigma_a = sig_[2]; p.sigma_ab = sig_[3];
        for (int i = 0; i < 3; i++) p.grav[i] = grav[i];
        p.model = model_; p.imu_avg = imu_avg ? 1 : 0;
        p.state_transition_jacobians = state_transition_jacobians ? 1 : 0;
        p.lanes_per_window = 0;
        return p;
    }
    static cpi_outputs outputs_of(CpiResult &r) {
        cpi_outputs o{};
        o.DT = &r.DT; o.alpha = r.alpha_tau.data(); o.beta = r.beta_tau.data(); o.q = r.q_k2tau.data();
        o.J_q = r.J_q.data(); o.J_a = r.J_a.data(); o.J_b = r.J_b.data(); o.H_a = r.H_a.data(); o.H_b = r.H_b.data();
        o.O_a = r.O_a.data(); o.O_b = r.O_b.data(); o.P = r.P_meas.data();
        return o;
    }
    const std::vector<double> &knots() const { return knots_; }
    int model() const { return model_; }
    // the model an ImuFactorCPI built from this measurement evaluates: the Forster comparator's result is wrapped in
    // an ImuFactorCPIv1 by the reference (GraphSolver_IMU.cpp:227-231)
    int factor_model() const { return model_ == CPI_MODEL_FORSTER ? CPI_MODEL_V1 : model_; }

    bool imu_avg = false;
    bool state_transition_jacobians = true;  // CpiV2.h:58
    Vec3 b_w_lin{}, b_a_lin{};
    Vec4 q_k_lin{};
    Vec3 grav{};
    // CpiBase.h:99-124 (+ CpiV2.h O_a / O_b): computed on first read after a feed_IMU
    Lazy<double> DT{this, 0.0, true};
    Lazy<Vec3> alpha_tau{this, Vec3{}, true}, beta_tau{this, Vec3{}, true};
    Lazy<Vec4> q_k2tau{this, Vec4{{0, 0, 0, 1}}, true};
    Lazy<Mat3> J_q{this}, J_a{this}, J_b{this}, H_a{this}, H_b{this}, O_a{this}, O_b{this};
    Lazy<Mat15> P_meas{this};

protected:
    void push(double t, const Vec3 &w, const Vec3 &a) {
        knots_.push_back(t);
        for (int i = 0; i < 3; i++) knots_.push_back(w[i]);
        for (int i = 0; i < 3; i++) knots_.push_back(a[i]);
        dirty_ = true;
    }
    void touch() { dirty_ = true; }              // a recorded knot was rewritten in place
    std::vector<double> knots_;
private:
    void finalize_incremental(const Context &ctx) {
        cpi_params p = params();
        const double lin[6] = { b_w_lin[0], b_w_lin[1], b_w_lin[2], b_a_lin[0], b_a_lin[1], b_a_lin[2] };
        CpiResult r;
        cpi_outputs o = outputs_of(r);   // everything, so that the carry holds every part a later read may need
        const int32_t n = knots_.empty() ? 0 : (int32_t)(knots_.size() / 7 - 1);
        static const double zero_knot[7] = { 0, 0, 0, 0, 0, 0, 0 };
        std::vector<double> next(cpi_carry_doubles(model_));
        ctx.check(cpi_preintegrate_resume_host(ctx.get(), &p, 1, n, knots_.empty() ? zero_knot : knots_.data(), nullptr, nullptr,
                                               n + 1, lin, q_k_lin.data(), carry_.empty() ? nullptr : carry_.data(), next.data(), &o));
        carry_.swap(next);
        if (n > 0) knots_.erase(knots_.begin(), knots_.end() - 7);   // the next segment starts on this one's last knot
        fed_.clear();
        set_result(r);
    }
    template <class T> friend class Lazy;
    // full: the member being read is a Jacobian / covariance (not one of the four means)
    void ensure(bool full = true) const { if (dirty_ || (full && means_only_)) const_cast<CpiBase *>(this)->finalize(ctx_ ? *ctx_ : default_context()); }
    CpiResult peek() const {                     // the stored values, without running anything
        CpiResult r;
        r.DT = DT.v_; r.alpha_tau = alpha_tau.v_; r.beta_tau = beta_tau.v_; r.q_k2tau = q_k2tau.v_;
        r.J_q = J_q.v_; r.J_a = J_a.v_; r.J_b = J_b.v_; r.H_a = H_a.v_; r.H_b = H_b.v_; r.O_a = O_a.v_; r.O_b = O_b.v_;
        r.P_meas = P_meas.v_;
        return r;
    }
    void put(const CpiResult &r) {
        DT.v_ = r.DT; alpha_tau.v_ = r.alpha_tau; beta_tau.v_ = r.beta_tau; q_k2tau.v_ = r.q_k2tau;
        J_q.v_ = r.J_q; J_a.v_ = r.J_a; J_b.v_ = r.J_b; H_a.v_ = r.H_a; H_b.v_ = r.H_b; O_a.v_ = r.O_a; O_b.v_ = r.O_b;
        P_meas.v_ = r.P_meas;
    }
    int model_ = CPI_MODEL_V1;
    double sig_[4] = {0, 0, 0, 0};
    const Context *ctx_ = nullptr;
    bool dirty_ = false;                         // intervals recorded since the result members were last computed
    bool means_only_ = false;                    // the last computation (CpiBatch::flush_means) filled the four means only
    bool incremental_ = false;                   // set_incremental
    std::vector<int32_t> fed_;                   // incremental: per interval fed since the last read, the index of its closing knot
    std::vector<double> carry_;                  // incremental: the carry record of the intervals integrated so far
};
template <class T> inline void Lazy<T>::sync() const { owner_->ensure(!mean_); }

class CpiV1 : public CpiBase {
public:
    CpiV1(double sigma_w, double sigma_wb, double sigma_a, double sigma_ab, bool imu_avg_ = false)
        : CpiBase(CPI_MODEL_V1, sigma_w, sigma_wb, sigma_a, sigma_ab, imu_avg_) {}
};
class CpiV2 : public CpiBase {
public:
    CpiV2(double sigma_w, double sigma_wb, double sigma_a, double sigma_ab, bool imu_avg_ = false)
        : CpiBase(CPI_MODEL_V2, sigma_w, sigma_wb, sigma_a, sigma_ab, imu_avg_) {}
};

// The "Forster discrete" comparator: what GraphSolver::createimufactor_discrete (GraphSolver_IMU.cpp:141-232) builds
// with gtsam::PreintegratedCombinedMeasurements -- the four covariances of :152-155 are the constructor's sigmas^2, the
// bias estimate of :162 goes to setLinearizationPoints(bg_K, ba_K), the loop calls integrateMeasurement(acc, omega, dt)
// (:180, :194; GTSAM's argument order).  After finalize() / CpiBatch::flush() the result members hold what :204-225
// derive from the GTSAM object (alpha_tau = deltaPij, beta_tau = deltaVij, q_k2tau = rot_2_quat(deltaRij^T),
// J_q = -delRdelBiasOmega, J_b / J_a = delV / delP delBiasOmega, H_b / H_a = delV / delP delBiasAcc, P_meas = the
// block-swapped preintMeasCov), ready for ImuFactorCPI (:227-231).  GTSAM is not part of the reference tree: parity
// of this model is unpinned (oracle/forster_oracle.c).
class ForsterDiscrete : public CpiBase {
public:
    ForsterDiscrete(double sigma_g, double sigma_wg, double sigma_a, double sigma_wa)
        : CpiBase(CPI_MODEL_FORSTER, sigma_g, sigma_wg, sigma_a, sigma_wa, false) {}
    // reading (measuredAcc, measuredOmega) held over the next dt seconds; dt <= 0 is ignored (GraphSolver_IMU.cpp:171)
    void integrateMeasurement(const Vec3 &measuredAcc, const Vec3 &measuredOmega, double dt) {
        if (!(dt > 0)) return;
        if (knots_.empty()) push(0.0, measuredOmega, measuredAcc);
        else {   // the closing knot of the previous interval becomes the opening knot of this one: give it this reading
            double *k = &knots_[knots_.size() - 7];
            for (int i = 0; i < 3; i++) { k[1 + i] = measuredOmega[i]; k[4 + i] = measuredAcc[i]; }
            touch();
        }
        // intervals are stored as knot times; t += dt reproduces dt to within one rounding of the running time
        t_ += dt;
        push(t_, measuredOmega, measuredAcc);
    }
    double deltaTij() const { return DT; }
private:
    double t_ = 0.0;
};

// Collects many recorded windows (same model / flags / gravity) and runs them in ONE launch.
class CpiBatch {
public:
    void add(CpiBase *w) {
        // (many incremental windows at once: cpi_preintegrate_resume / Engine.preintegrate_resume)
        if (w->incremental()) throw std::logic_error("CpiBatch::add: an incremental preintegrator runs on its own");
        win_.push_back(w);
    }
    void flush(const Context &ctx) {
        if (win_.empty()) return;
        const int64_t W = (int64_t)win_.size();
        std::vector<double> knots, lin, qk;
        std::vector<int64_t> first;
        std::vector<int32_t> count;
        const int32_t N = ragged(knots, first, count, lin, qk);
        cpi_params p = win_[0]->params();
        std::vector<double> DT(W), al(W * 3), be(W * 3), q(W * 4), Jq(W * 9), Ja(W * 9), Jb(W * 9), Ha(W * 9), Hb(W * 9),
            Oa(W * 9), Ob(W * 9), P(W * 225);
        cpi_outputs o{ DT.data(), al.data(), be.data(), q.data(), Jq.data(), Ja.data(), Jb.data(), Ha.data(), Hb.data(),
                       Oa.data(), Ob.data(), P.data() };
        // windows of equal length lie back to back = the dense layout: that entry pipelines upload / kernels / download
        bool dense = true;
        for (int64_t w = 0; w < W && dense; w++) dense = (count[w] == N) && !win_[w]->knots().empty();
        ctx.check(cpi_preintegrate_batch_host(ctx.get(), &p, W, N, knots.data(), dense ? nullptr : first.data(), dense ? nullptr : count.data(),
                                              (int64_t)(knots.size() / 7), lin.data(), qk.data(), &o));
        for (int64_t w = 0; w < W; w++) {
            CpiResult r;
            r.DT = DT[w];
            for (int i = 0; i < 3; i++) { r.alpha_tau[i] = al[w * 3 + i]; r.beta_tau[i] = be[w * 3 + i]; }
            for (int i = 0; i < 4; i++) r.q_k2tau[i] = q[w * 4 + i];
            for (int i = 0; i < 9; i++) {
                r.J_q[i] = Jq[w * 9 + i]; r.J_a[i] = Ja[w * 9 + i]; r.J_b[i] = Jb[w * 9 + i]; r.H_a[i] = Ha[w * 9 + i];
                r.H_b[i] = Hb[w * 9 + i]; r.O_a[i] = Oa[w * 9 + i]; r.O_b[i] = Ob[w * 9 + i];
            }
            for (int i = 0; i < 225; i++) r.P_meas[i] = P[w * 225 + i];
            win_[w]->set_result(r);
        }
        win_.clear();
    }
    // The reference's members after EVERY feed_IMU (cpi_preintegrate_running_host): for each added window one CpiResult per
    // recorded knot interval, result[w][i] = the members after interval i (a skipped interval -- dt <= 0, the NaN separator
    // feed_IMU places between intervals that do not chain -- repeats the previous one).  Models 1 and 2; the bias Jacobians
    // are filled for model 1 only.  The windows stay added and their own result members are not touched: flush() still
    // computes them.
    std::vector<std::vector<CpiResult>> running(const Context &ctx) const { return running_impl(ctx, false); }
    // running() with model 2's bias Jacobians (cpi_running_stj_batch_host): J_q ... O_b are filled for model 2 as well (all
    // seven, read out of the state transition columns after every interval; the windows' params must have
    // state_transition_jacobians set).  Model 1: running().
    std::vector<std::vector<CpiResult>> running_stj(const Context &ctx) const { return running_impl(ctx, true); }
    // The members of every added window at ARBITRARY times (cpi_query_batch_host): result[w][k] = window w at times[w][k] -- on a
    // knot stamp what running() holds after that knot's interval, inside an interval that state advanced over the partial
    // interval with the reading held (the reference's tail, GraphSolver_IMU.cpp:64-69), before the window's first stamp the zero
    // state, at or past its last stamp the window's measurement.  times holds one vector per added window, in any order.  A
    // window that holds a separator knot (feed_IMU calls that do not chain) has no time axis to query: std::logic_error.  Models
    // 1 and 2; the bias Jacobians are filled for model 1 only, P_meas is not computed (at_cov computes it).  The windows stay added.
    std::vector<std::vector<CpiResult>> at(const Context &ctx, const std::vector<std::vector<double>> &times) const {
        return at_impl(ctx, times, false);
    }
    // at() with the covariance: P_meas is filled as well (cpi_query_cov_batch_host) -- the complete measurement of a factor at a
    // query time.
    std::vector<std::vector<CpiResult>> at_cov(const Context &ctx, const std::vector<std::vector<double>> &times) const {
        return at_impl(ctx, times, true);
    }
    // at_cov() with model 2's bias Jacobians (cpi_query_stj_batch_host): J_q ... O_b are filled for model 2 as well, all seven -- what
    // a model-2 factor at a query time needs (the windows' params must have state_transition_jacobians set).  Model 1: at_cov().
    std::vector<std::vector<CpiResult>> at_stj(const Context &ctx, const std::vector<std::vector<double>> &times) const {
        return at_impl(ctx, times, true, true);
    }
    // Mean outputs only (DT, alpha_tau, beta_tau, q_k2tau): the HBM-bound request.  The recorded windows are written
    // straight into the TILED layout (include/cpi_amd.h: tiles[ceil(W/64)][N+1][7][64], knot s of window w at
    // (((w / 64) (N+1) + s) 7 + k) 64 + w % 64 -- no dense copy is ever made) with their own interval counts, and go
    // through cpi_preintegrate_tiled_batch_host (chunked upload / kernel / download pipeline).  Models 1 and 2.
    void flush_means(const Context &ctx) {
        if (win_.empty()) return;
        const int64_t W = (int64_t)win_.size();
        std::vector<int32_t> count(W);
        int32_t N = 0;
        for (int64_t w = 0; w < W; w++) {
            const std::vector<double> &k = win_[w]->knots();
            count[w] = k.empty() ? 0 : (int32_t)(k.size() / 7 - 1);
            if (count[w] > N) N = count[w];
        }
        const int64_t nb = (W + 63) / 64;
        std::vector<double> tiles((size_t)nb * (N + 1) * 448, 0.0), lin(W * 6), qk(W * 4);
        for (int64_t w = 0; w < W; w++) {
            const std::vector<double> &k = win_[w]->knots();
            double *col = &tiles[(size_t)(w / 64) * (N + 1) * 448 + (size_t)(w % 64)];
            for (int32_t s = 0; s <= count[w] && !k.empty(); s++)
                for (int f = 0; f < 7; f++) col[((size_t)s * 7 + f) * 64] = k[(size_t)s * 7 + f];
            for (int i = 0; i < 3; i++) { lin[w * 6 + i] = win_[w]->b_w_lin[i]; lin[w * 6 + 3 + i] = win_[w]->b_a_lin[i]; }
            for (int i = 0; i < 4; i++) qk[w * 4 + i] = win_[w]->q_k_lin[i];
        }
        cpi_params p = win_[0]->params();
        std::vector<double> DT(W), al(W * 3), be(W * 3), q(W * 4);
        cpi_outputs o{};
        o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data();
        ctx.check(cpi_preintegrate_tiled_batch_host(ctx.get(), &p, W, N, tiles.data(), count.data(), lin.data(), qk.data(), &o));
        for (int64_t w = 0; w < W; w++)
            win_[w]->set_means(DT[w], Vec3{{al[w * 3], al[w * 3 + 1], al[w * 3 + 2]}}, Vec3{{be[w * 3], be[w * 3 + 1], be[w * 3 + 2]}},
                               Vec4{{q[w * 4], q[w * 4 + 1], q[w * 4 + 2], q[w * 4 + 3]}});
        win_.clear();
    }
private:
    // running / running_stj: the rows of all windows in one call; stj: model 2's seven Jacobians as well
    std::vector<std::vector<CpiResult>> running_impl(const Context &ctx, bool stj) const {
        std::vector<std::vector<CpiResult>> res(win_.size());
        if (win_.empty()) return res;
        const int64_t W = (int64_t)win_.size();
        std::vector<double> knots, lin, qk;
        std::vector<int64_t> first;
        std::vector<int32_t> count;
        const int32_t N = ragged(knots, first, count, lin, qk);
        if (N == 0) return res;
        cpi_params p = win_[0]->params();
        const bool v2 = stj && p.model == CPI_MODEL_V2;    // all seven matrices from the transition columns
        const bool jac = p.model == CPI_MODEL_V1 || v2;
        const size_t M = (size_t)W * (size_t)N;
        std::vector<double> DT(M), al(M * 3), be(M * 3), q(M * 4), Jq(jac ? M * 9 : 0), Ja(jac ? M * 9 : 0), Jb(jac ? M * 9 : 0),
            Ha(jac ? M * 9 : 0), Hb(jac ? M * 9 : 0), Oa(v2 ? M * 9 : 0), Ob(v2 ? M * 9 : 0), P(M * 225);
        cpi_outputs o{};
        o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data(); o.P = P.data();
        if (jac) { o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data(); }
        if (v2) { o.O_a = Oa.data(); o.O_b = Ob.data(); }
        const int64_t K = (int64_t)(knots.size() / 7);
        ctx.check(stj ? cpi_running_stj_batch_host(ctx.get(), &p, W, N, knots.data(), first.data(), count.data(), K, lin.data(), qk.data(), &o)
                      : cpi_preintegrate_running_host(ctx.get(), &p, W, N, knots.data(), first.data(), count.data(), K, lin.data(), qk.data(), &o));
        for (int64_t w = 0; w < W; w++) {
            res[w].resize(count[w]);
            for (int32_t i = 0; i < count[w]; i++) {
                const size_t r = (size_t)w * N + i;
                CpiResult &x = res[w][i];
                x.DT = DT[r];
                for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
                for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
                if (jac)
                    for (int k = 0; k < 9; k++) {
                        x.J_q[k] = Jq[r * 9 + k]; x.J_a[k] = Ja[r * 9 + k]; x.J_b[k] = Jb[r * 9 + k];
                        x.H_a[k] = Ha[r * 9 + k]; x.H_b[k] = Hb[r * 9 + k];
                        if (v2) { x.O_a[k] = Oa[r * 9 + k]; x.O_b[k] = Ob[r * 9 + k]; }
                    }
                for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
            }
        }
        return res;
    }
    // at / at_cov / at_stj: the queries of all windows in one call; cov: P_meas as well; stj: model 2's seven Jacobians as well
    std::vector<std::vector<CpiResult>> at_impl(const Context &ctx, const std::vector<std::vector<double>> &times, bool cov, bool stj = false) const {
        if (times.size() != win_.size()) throw std::logic_error("CpiBatch::at: one vector of times per added window");
        std::vector<std::vector<CpiResult>> res(win_.size());
        std::vector<int32_t> qwin;
        std::vector<double> qtime;
        for (size_t w = 0; w < win_.size(); w++) {
            const std::vector<double> &k = win_[w]->knots();
            for (size_t i = 0; i < k.size(); i += 7)
                if (k[i] != k[i]) throw std::logic_error("CpiBatch::at: window " + std::to_string(w) + " holds a separator knot (its intervals do not chain)");
            qwin.insert(qwin.end(), times[w].size(), (int32_t)w);
            qtime.insert(qtime.end(), times[w].begin(), times[w].end());
            res[w].resize(times[w].size());
        }
        const int64_t Q = (int64_t)qtime.size();
        if (Q == 0) return res;
        const int64_t W = (int64_t)win_.size();
        std::vector<double> knots, lin, qk;
        std::vector<int64_t> first;
        std::vector<int32_t> count;
        const int32_t N = ragged(knots, first, count, lin, qk);
        cpi_params p = win_[0]->params();
        const bool v2 = stj && p.model == CPI_MODEL_V2;
        const bool jac = p.model == CPI_MODEL_V1 || v2;
        std::vector<double> DT(Q), al(Q * 3), be(Q * 3), q(Q * 4), Jq(jac ? Q * 9 : 0), Ja(jac ? Q * 9 : 0), Jb(jac ? Q * 9 : 0),
            Ha(jac ? Q * 9 : 0), Hb(jac ? Q * 9 : 0), Oa(v2 ? Q * 9 : 0), Ob(v2 ? Q * 9 : 0), P(cov ? Q * 225 : 0);
        cpi_outputs o{};
        o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data();
        if (jac) { o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data(); }
        if (v2) { o.O_a = Oa.data(); o.O_b = Ob.data(); }
        if (cov) o.P = P.data();
        const int64_t K = (int64_t)(knots.size() / 7);
        ctx.check(stj ? cpi_query_stj_batch_host(ctx.get(), &p, W, N, knots.data(), first.data(), count.data(), K, lin.data(), qk.data(), Q,
                                                 qwin.data(), qtime.data(), &o)
                  : cov ? cpi_query_cov_batch_host(ctx.get(), &p, W, N, knots.data(), first.data(), count.data(), K, lin.data(), qk.data(), Q,
                                                 qwin.data(), qtime.data(), &o)
                      : cpi_query_batch_host(ctx.get(), &p, W, N, knots.data(), first.data(), count.data(), K, lin.data(), qk.data(), Q,
                                             qwin.data(), qtime.data(), &o));
        size_t r = 0;
        for (std::vector<CpiResult> &win : res)
            for (CpiResult &x : win) {
                x.DT = DT[r];
                for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
                for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
                if (jac)
                    for (int k = 0; k < 9; k++) {
                        x.J_q[k] = Jq[r * 9 + k]; x.J_a[k] = Ja[r * 9 + k]; x.J_b[k] = Jb[r * 9 + k];
                        x.H_a[k] = Ha[r * 9 + k]; x.H_b[k] = Hb[r * 9 + k];
                        if (v2) { x.O_a[k] = Oa[r * 9 + k]; x.O_b[k] = Ob[r * 9 + k]; }
                    }
                if (cov)
                    for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
                r++;
            }
        return res;
    }
    // the added windows in the ragged layout of include/cpi_amd.h (a window without knots: one zero knot, count 0); returns N
    int32_t ragged(std::vector<double> &knots, std::vector<int64_t> &first, std::vector<int32_t> &count, std::vector<double> &lin,
                   std::vector<double> &qk) const {
        const int64_t W = (int64_t)win_.size();
        first.resize(W); count.resize(W); lin.resize(W * 6); qk.resize(W * 4);
        int32_t N = 0;
        for (int64_t w = 0; w < W; w++) {
            const std::vector<double> &k = win_[w]->knots();
            first[w] = (int64_t)(knots.size() / 7);
            count[w] = k.empty() ? 0 : (int32_t)(k.size() / 7 - 1);
            if (count[w] > N) N = count[w];
            if (k.empty()) knots.insert(knots.end(), 7, 0.0); else knots.insert(knots.end(), k.begin(), k.end());
            for (int i = 0; i < 3; i++) { lin[w * 6 + i] = win_[w]->b_w_lin[i]; lin[w * 6 + 3 + i] = win_[w]->b_a_lin[i]; }
            for (int i = 0; i < 4; i++) qk[w * 4 + i] = win_[w]->q_k_lin[i];
        }
        return N;
    }
    std::vector<CpiBase *> win_;
};

// ---- caller-side data formats --------------------------------------------
// The reference's simulated-IMU wire format, one reading per line "wx wy wz ax ay az 0 t_ms"
// (cpi_compare/src/sim/SimParser.h:130-193: fields split on single spaces, empty fields skipped, column 8 is
// the stamp in milliseconds).  Returns knot records {t[s], w[3], a[3]}.
inline std::vector<double> parse_imu_text(const std::string &text) {
    std::vector<double> knots;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        double f[8];
        int nf = 0;
        size_t p = pos;
        while (p < eol && nf < 8) {
            while (p < eol && text[p] == ' ') p++;
            if (p >= eol) break;
            size_t q = p;
            while (q < eol && text[q] != ' ') q++;
            f[nf++] = std::atof(text.substr(p, q - p).c_str());
            p = q;
        }
        if (nf == 8) {
            knots.push_back(1e-3 * f[7]);
            for (int i = 0; i < 6; i++) knots.push_back(f[i]);
        }
        pos = eol + 1;
    }
    return knots;
}

// Cutting ONE IMU stream into preintegration windows at successive update times exactly like
// GraphSolver::createimufactor_cpi_v1/v2 (GraphSolver_IMU.cpp:50-69): whole intervals while
// imu_times[1] <= updatetime, then the partial tail interval with the front reading repeated, after which the
// front stamp is overwritten by the update time.  Output is the knots/first/count layout of cpi_amd.h.
struct WindowSet {
    std::vector<double> knots;
    std::vector<int64_t> first;
    std::vector<int32_t> count;
    int32_t max_count = 0;
};
inline WindowSet assemble_windows(const std::vector<double> &stream, const std::vector<double> &update_times) {
    WindowSet ws;
    const size_t K = stream.size() / 7;
    if (K == 0) return ws;
    size_t front = 0;
    double front_t = stream[0];
    auto push = [&](double t, const double *r) { ws.knots.push_back(t); for (int i = 1; i < 7; i++) ws.knots.push_back(r[i]); };
    for (double T : update_times) {
        ws.first.push_back((int64_t)(ws.knots.size() / 7));
        push(front_t, &stream[front * 7]);
        int32_t n = 0;
        while (K - front > 1 && stream[(front + 1) * 7] <= T) {
            front++;
            front_t = stream[front * 7];
            push(front_t, &stream[front * 7]);   // dt < 0 intervals stay in the list: the kernels skip them
            n++;
        }
        if (T - front_t > 0) { push(T, &stream[front * 7]); front_t = T; n++; }
        ws.count.push_back(n);
        if (n > ws.max_count) ws.max_count = n;
    }
    return ws;
}

// The same cutting written STRAIGHT into the tiled layout of cpi_preintegrate_tiled_batch (mean-only requests; DESIGN.md
// 3.1a): pass 1 walks the deque loop and records where each window starts and how long it is, pass 2 places knot s of
// window w at its tile slot.  No intermediate knots / first / count copy.  N = the largest count (or min_N if larger).
struct TiledWindowSet {
    std::vector<double> tiles;     // [ceil(W/64)][N+1][7][64]
    std::vector<int32_t> count;    // [W]
    int64_t W = 0;
    int32_t N = 0;
};
inline TiledWindowSet assemble_windows_tiled(const std::vector<double> &stream, const std::vector<double> &update_times, int32_t min_N = 0) {
    TiledWindowSet ts;
    const size_t K = stream.size() / 7;
    if (K == 0) return ts;
    struct Win { size_t front0; double start_t; int32_t whole; bool tail; double T; };
    std::vector<Win> win;
    win.reserve(update_times.size());
    size_t front = 0;
    double front_t = stream[0];
    int32_t N = min_N;
    for (double T : update_times) {
        Win w{front, front_t, 0, false, T};
        while (K - front > 1 && stream[(front + 1) * 7] <= T) { front++; front_t = stream[front * 7]; w.whole++; }
        if (T - front_t > 0) { w.tail = true; front_t = T; }
        win.push_back(w);
        const int32_t n = w.whole + (w.tail ? 1 : 0);
        ts.count.push_back(n);
        if (n > N) N = n;
    }
    ts.W = (int64_t)win.size();
    ts.N = N;
    const size_t nb = (size_t)((ts.W + 63) / 64), tstride = (size_t)(N + 1) * 448;
    ts.tiles.assign(nb * tstride, 0.0);
    for (size_t w = 0; w < win.size(); w++) {
        double *col = &ts.tiles[(w / 64) * tstride + (w % 64)];
        auto put = [&](int32_t s, double t, const double *r) { col[((size_t)s * 7) * 64] = t; for (int f = 1; f < 7; f++) col[((size_t)s * 7 + f) * 64] = r[f]; };
        put(0, win[w].start_t, &stream[win[w].front0 * 7]);
        for (int32_t s = 1; s <= win[w].whole; s++) put(s, stream[(win[w].front0 + s) * 7], &stream[(win[w].front0 + s) * 7]);
        if (win[w].tail) put(win[w].whole + 1, win[w].T, &stream[(win[w].front0 + win[w].whole) * 7]);
    }
    return ts;
}

// The longest window (whole intervals + tail) that cutting K readings at update_times gives: the deque loop of assemble_windows,
// counts only -- the TIGHT row bound of ImuStream::running / ImuStreamSet::running (their output is U * N rows).
inline int32_t longest_window(const double *stream, size_t K, const double *update_times, size_t U) {
    if (K == 0) return 0;
    size_t front = 0;
    double front_t = stream[0];
    int64_t longest = 0;
    for (size_t u = 0; u < U; u++) {
        const double T = update_times[u];
        int64_t n = 0;
        while (K - front > 1 && stream[(front + 1) * 7] <= T) { front++; front_t = stream[front * 7]; n++; }
        if (T - front_t > 0) { front_t = T; n++; }
        if (n > longest) longest = n;
    }
    return (int32_t)std::min<int64_t>(longest, 65535);
}
// The row arrays of a running call (U * N rows: means, P, the five bias Jacobians of model 1) and their unpacking into one
// CpiResult per interval of a window's count.
struct RunningRows {
    std::vector<double> DT, al, be, q, Jq, Ja, Jb, Ha, Hb, P;
    bool jac = false;
    int32_t N = 0;
    cpi_outputs bind(int model, int64_t U, int32_t N_) {
        jac = model == CPI_MODEL_V1;
        N = N_;
        const size_t M = (size_t)U * (size_t)N;
        DT.resize(M); al.resize(M * 3); be.resize(M * 3); q.resize(M * 4); P.resize(M * 225);
        if (jac) { Jq.resize(M * 9); Ja.resize(M * 9); Jb.resize(M * 9); Ha.resize(M * 9); Hb.resize(M * 9); }
        cpi_outputs o{};
        o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data(); o.P = P.data();
        if (jac) { o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data(); }
        return o;
    }
    std::vector<CpiResult> window(int64_t w, int32_t count) const {
        std::vector<CpiResult> res((size_t)count);
        for (int32_t i = 0; i < count; i++) {
            const size_t r = (size_t)w * N + i;
            CpiResult &x = res[i];
            x.DT = DT[r];
            for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
            for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
            if (jac)
                for (int k = 0; k < 9; k++) {
                    x.J_q[k] = Jq[r * 9 + k]; x.J_a[k] = Ja[r * 9 + k]; x.J_b[k] = Jb[r * 9 + k];
                    x.H_a[k] = Ha[r * 9 + k]; x.H_b[k] = Hb[r * 9 + k];
                }
            for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
        }
        return res;
    }
};

// The members at ABSOLUTE query times over IMU stream(s) read in place (cpi_query_stream_batch_host), one CpiResult per time: what
// ImuStream::at* / ImuStreamSet::at* share.  soff / uoff / qrun NULL: one stream.  cov: P_meas as well; stj: model 2's seven bias
// Jacobians as well (model 1's five are always filled).  windows (optional) receives the GLOBAL window index of every time (-1: a
// run without update times, whose members are NaN).
inline std::vector<CpiResult> query_stream_results(const Context &ctx, const cpi_params &prm, int64_t R, const std::vector<double> &knots,
                                                   const int64_t *soff, const std::vector<double> &ut, const int64_t *uoff, int32_t N,
                                                   const std::vector<double> &lin, const std::vector<double> &qk, const int32_t *qrun,
                                                   const std::vector<double> &times, bool cov, bool stj, std::vector<int32_t> *windows) {
    const int64_t Q = (int64_t)times.size(), K = (int64_t)(knots.size() / 7), U = (int64_t)ut.size();
    std::vector<CpiResult> res((size_t)Q);
    if (windows) windows->assign((size_t)Q, -1);
    if (Q == 0) return res;
    const bool v2 = stj && prm.model == CPI_MODEL_V2;
    const bool jac = prm.model == CPI_MODEL_V1 || v2;
    std::vector<double> DT(Q), al(Q * 3), be(Q * 3), q(Q * 4), Jq(jac ? Q * 9 : 0), Ja(jac ? Q * 9 : 0), Jb(jac ? Q * 9 : 0),
        Ha(jac ? Q * 9 : 0), Hb(jac ? Q * 9 : 0), Oa(v2 ? Q * 9 : 0), Ob(v2 ? Q * 9 : 0), P(cov ? Q * 225 : 0);
    std::vector<int32_t> qwin((size_t)Q, -1);
    cpi_outputs o{};
    o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data();
    if (jac) { o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data(); }
    if (v2) { o.O_a = Oa.data(); o.O_b = Ob.data(); }
    if (cov) o.P = P.data();
    ctx.check(cpi_query_stream_batch_host(ctx.get(), &prm, R, K, knots.data(), soff, U, ut.data(), uoff, N, lin.data(),
                                          qk.empty() ? nullptr : qk.data(), Q, qrun, times.data(), qwin.data(), &o));
    for (size_t r = 0; r < (size_t)Q; r++) {
        CpiResult &x = res[r];
        x.DT = DT[r];
        for (int k = 0; k < 3; k++) { x.alpha_tau[k] = al[r * 3 + k]; x.beta_tau[k] = be[r * 3 + k]; }
        for (int k = 0; k < 4; k++) x.q_k2tau[k] = q[r * 4 + k];
        if (jac)
            for (int k = 0; k < 9; k++) {
                x.J_q[k] = Jq[r * 9 + k]; x.J_a[k] = Ja[r * 9 + k]; x.J_b[k] = Jb[r * 9 + k];
                x.H_a[k] = Ha[r * 9 + k]; x.H_b[k] = Hb[r * 9 + k];
                if (v2) { x.O_a[k] = Oa[r * 9 + k]; x.O_b[k] = Ob[r * 9 + k]; }
            }
        if (cov)
            for (int k = 0; k < 225; k++) x.P_meas[k] = P[r * 225 + k];
    }
    if (windows) *windows = qwin;
    return res;
}

// Consecutive preintegrated windows JOINED (cpi_merge_batch_host): result j = rows[first[j]] o ... o rows[first[j] + count[j] - 1],
// oldest first -- keyframe decimation, or the one factor that replaces the two that met at a removed state -- without the IMU
// readings.  Model-1 results (CpiV1 / CpiBatch / ImuStream with model 1: the five bias Jacobians and P_meas filled), ALL
// PREINTEGRATED AT THE SAME b_w_lin / b_a_lin: the call cannot check that.  count is clamped into [0, G] and groups are clipped at
// the end of rows; count 0 gives the zero state, count 1 the row itself bit for bit.
inline std::vector<CpiResult> merge(const Context &ctx, const std::vector<CpiResult> &rows, int32_t G,
                                    const std::vector<int64_t> *first = nullptr, const std::vector<int32_t> *count = nullptr) {
    const size_t R = rows.size();
    if (G < 1) throw std::invalid_argument("cpi_host::merge: G must be >= 1");
    if (first && count && first->size() != count->size()) throw std::invalid_argument("cpi_host::merge: first and count differ in length");
    const size_t M = first ? first->size() : count ? count->size() : (R + (size_t)G - 1) / (size_t)G;
    std::vector<CpiResult> res(M);
    if (M == 0) return res;
    struct Rows {
        std::vector<double> DT, al, be, q, Jq, Ja, Jb, Ha, Hb, P;
        cpi_outputs bind(size_t n) {
            DT.resize(n); al.resize(n * 3); be.resize(n * 3); q.resize(n * 4); P.resize(n * 225);
            Jq.resize(n * 9); Ja.resize(n * 9); Jb.resize(n * 9); Ha.resize(n * 9); Hb.resize(n * 9);
            cpi_outputs o{};
            o.DT = DT.data(); o.alpha = al.data(); o.beta = be.data(); o.q = q.data(); o.P = P.data();
            o.J_q = Jq.data(); o.J_a = Ja.data(); o.J_b = Jb.data(); o.H_a = Ha.data(); o.H_b = Hb.data();
            return o;
        }
    } in, out;
    const cpi_outputs i = in.bind(R), o = out.bind(M);
    for (size_t r = 0; r < R; r++) {
        const CpiResult &x = rows[r];
        in.DT[r] = x.DT;
        for (int k = 0; k < 3; k++) { in.al[r * 3 + k] = x.alpha_tau[k]; in.be[r * 3 + k] = x.beta_tau[k]; }
        for (int k = 0; k < 4; k++) in.q[r * 4 + k] = x.q_k2tau[k];
        for (int k = 0; k < 9; k++) {
            in.Jq[r * 9 + k] = x.J_q[k]; in.Ja[r * 9 + k] = x.J_a[k]; in.Jb[r * 9 + k] = x.J_b[k];
            in.Ha[r * 9 + k] = x.H_a[k]; in.Hb[r * 9 + k] = x.H_b[k];
        }
        for (int k = 0; k < 225; k++) in.P[r * 225 + k] = x.P_meas[k];
    }
    ctx.check(cpi_merge_batch_host(ctx.get(), CPI_MODEL_V1, (int64_t)M, G, (int64_t)R, &i, first ? first->data() : nullptr,
                                   count ? count->data() : nullptr, &o));
    for (size_t r = 0; r < M; r++) {
        CpiResult &x = res[r];
        x.DT = out.DT[r];
        for (int k = 0; k < 3; k++) { x.alpha_tau[k] = out.al[r * 3 + k]; x.beta_tau[k] = out.be[r * 3 + k]; }
        for (int k = 0; k < 4; k++) x.q_k2tau[k] = out.q[r * 4 + k];
        for (int k = 0; k < 9; k++) {
            x.J_q[k] = out.Jq[r * 9 + k]; x.J_a[k] = out.Ja[r * 9 + k]; x.J_b[k] = out.Jb[r * 9 + k];
            x.H_a[k] = out.Ha[r * 9 + k]; x.H_b[k] = out.Hb[r * 9 + k];
        }
        for (int k = 0; k < 225; k++) x.P_meas[k] = out.P[r * 225 + k];
    }
    return res;
}

// JPLNavState::retract / localCoordinates (JPLNavState.cpp:37-88) over batches of states held as flat vectors: states [S * 16] =
// [q(4) bg(3) v(3) ba(3) p(3)] per state, delta / the result of local_coordinates [S * 15] = [dtheta bg v ba p]
// (cpi_retract_batch_host / cpi_local_batch_host: the device kernels' bits).
inline std::vector<double> retract(const Context &ctx, const std::vector<double> &states, const std::vector<double> &delta) {
    if (states.size() % 16 || delta.size() != states.size() / 16 * 15) throw std::invalid_argument("cpi_host::retract: states [S * 16], delta [S * 15]");
    std::vector<double> out(states.size());
    ctx.check(cpi_retract_batch_host(ctx.get(), (int64_t)(states.size() / 16), states.data(), delta.data(), out.data()));
    return out;
}
inline std::vector<double> local_coordinates(const Context &ctx, const std::vector<double> &x, const std::vector<double> &other) {
    if (x.size() % 16 || other.size() != x.size()) throw std::invalid_argument("cpi_host::local_coordinates: x and other [S * 16]");
    std::vector<double> xi(x.size() / 16 * 15);
    ctx.check(cpi_local_batch_host(ctx.get(), (int64_t)(x.size() / 16), x.data(), other.data(), xi.data()));
    return xi;
}

// The Gauss-Newton / Levenberg-Marquardt step of chains of IMU factors (cpi_chain_solve_batch_host: the device kernel's bits).  C
// chains of G states each, back to back: hess [C * (G - 1) * 496] the rows of the Hessian sweep in chain order, prior empty or
// [C * G * 136], lambda empty or [C]; diagonal: CPI_DAMP_DIAGONAL instead of CPI_DAMP_IDENTITY.  Returns delta [C * G * 15] (what
// retract takes); status, when given, receives the per-chain codes of include/cpi_amd.h (a failed chain's rows are NaN).
inline std::vector<double> chain_solve(const Context &ctx, int64_t C, int64_t G, const std::vector<double> &hess,
                                       const std::vector<double> &prior = {}, const std::vector<double> &lambda = {},
                                       bool diagonal = false, std::vector<int32_t> *status = nullptr) {
    if (C < 0 || G < 1 || hess.size() != (size_t)(C * (G - 1)) * 496 || (!prior.empty() && prior.size() != (size_t)(C * G) * 136) ||
        (!lambda.empty() && lambda.size() != (size_t)C))
        throw std::invalid_argument("cpi_host::chain_solve: hess [C * (G - 1) * 496], prior empty or [C * G * 136], lambda empty or [C]");
    std::vector<double> delta((size_t)(C * G) * 15);
    if (status) status->assign((size_t)C, 0);
    static const double none = 0.0;      // G == 1: no factor rows, and the entry wants no pointer either; G > 1 with C == 0: never read
    ctx.check(cpi_chain_solve_batch_host(ctx.get(), C, G, C * G, C * (G - 1), nullptr, nullptr, nullptr, hess.empty() ? &none : hess.data(),
                                         prior.empty() ? nullptr : prior.data(), lambda.empty() ? nullptr : lambda.data(),
                                         diagonal ? CPI_DAMP_DIAGONAL : CPI_DAMP_IDENTITY, delta.data(), status ? status->data() : nullptr));
    return delta;
}

// The covariance of every state of chains of IMU factors at the states hess was linearised at (cpi_chain_marginals_batch_host: the
// UNDAMPED system of chain_solve's hess / prior, factorised and inverted block by block on the device; the device kernels' bits).
// Returns cov [C * G * 120]: Sigma[s][s] of every state as the packed upper triangle ((i, j), i <= j, at i + j (j + 1) / 2 -- a row
// of cpi_sqrt_information_packed_batch_host's input).  cross, when given, receives [C * G * 225]: Sigma[s][s+1] column-major in row s
// (the row of a chain's last state stays zero); status the solve's per-chain codes (a failed chain's rows are NaN).
inline std::vector<double> chain_marginals(const Context &ctx, int64_t C, int64_t G, const std::vector<double> &hess,
                                           const std::vector<double> &prior = {}, std::vector<double> *cross = nullptr,
                                           std::vector<int32_t> *status = nullptr) {
    if (C < 0 || G < 1 || hess.size() != (size_t)(C * (G - 1)) * 496 || (!prior.empty() && prior.size() != (size_t)(C * G) * 136))
        throw std::invalid_argument("cpi_host::chain_marginals: hess [C * (G - 1) * 496], prior empty or [C * G * 136]");
    std::vector<double> cov((size_t)(C * G) * 120);
    if (cross) cross->assign((size_t)(C * G) * 225, 0.0);
    if (status) status->assign((size_t)C, 0);
    static const double none = 0.0;      // G == 1: no factor rows; G > 1 with C == 0: never read
    ctx.check(cpi_chain_marginals_batch_host(ctx.get(), C, G, C * G, C * (G - 1), nullptr, nullptr, nullptr, hess.empty() ? &none : hess.data(),
                                             prior.empty() ? nullptr : prior.data(), cov.data(), cross ? cross->data() : nullptr,
                                             status ? status->data() : nullptr));
    return cov;
}

// What a fixed-lag window carries on when it slides (cpi_chain_marginalize_batch_host: the device kernel's bits): the leading drop
// states of every chain eliminated into a prior on the first state that stays.  C chains of G states back to back, hess and prior as
// chain_solve takes them, 0 <= drop < G.  Returns [C * 136]: per chain the packed [Lam eta; eta^T .] of state drop -- the row to put
// there in the next window's prior; status, when given, receives the per-chain codes of include/cpi_amd.h (a failed chain's row is NaN).
inline std::vector<double> chain_marginalize(const Context &ctx, int64_t C, int64_t G, const std::vector<double> &hess,
                                             const std::vector<double> &prior = {}, int32_t drop = 1,
                                             std::vector<int32_t> *status = nullptr) {
    if (C < 0 || G < 1 || hess.size() != (size_t)(C * (G - 1)) * 496 || (!prior.empty() && prior.size() != (size_t)(C * G) * 136))
        throw std::invalid_argument("cpi_host::chain_marginalize: hess [C * (G - 1) * 496], prior empty or [C * G * 136]");
    std::vector<double> out((size_t)C * 136);
    if (status) status->assign((size_t)C, 0);
    static const double none = 0.0;      // G == 1: no factor rows; G > 1 with C == 0: never read
    ctx.check(cpi_chain_marginalize_batch_host(ctx.get(), C, G, C * G, C * (G - 1), nullptr, nullptr, nullptr, hess.empty() ? &none : hess.data(),
                                               prior.empty() ? nullptr : prior.data(), drop, nullptr, out.data(), status ? status->data() : nullptr));
    return out;
}

// Long chains, solved in parallel ALONG the chain (cpi_chain_condense_batch_host, cpi_chain_expand_batch_host: the device kernels'
// bits).  C chains of G states back to back, hess / prior / lambda / diagonal as chain_solve takes them, K >= 1 the factors of a
// segment.  chain_condense eliminates the states between the ends of every segment: the reduced chains of Gr =
// cpi_chain_condense_states(G, K) states each, for chain_solve(ctx, C, Gr, rhess, rprior) WITHOUT lambda (the damping is in the
// reduced system), and the workspace chain_expand substitutes back from.  status: per segment, [C * (Gr - 1)], the codes of
// include/cpi_amd.h.  chain_expand returns delta [C * G * 15] from the reduced solve's rdelta [C * Gr * 15].
struct CondensedChains {
    int64_t Gr = 0;
    std::vector<double> rhess, rprior, workspace;
    std::vector<int32_t> rcount, status;
};
inline CondensedChains chain_condense(const Context &ctx, int64_t C, int64_t G, int64_t K, const std::vector<double> &hess,
                                      const std::vector<double> &prior = {}, const std::vector<double> &lambda = {}, bool diagonal = false) {
    if (C < 0 || G < 1 || K < 1 || hess.size() != (size_t)(C * (G - 1)) * 496 || (!prior.empty() && prior.size() != (size_t)(C * G) * 136) ||
        (!lambda.empty() && lambda.size() != (size_t)C))
        throw std::invalid_argument("cpi_host::chain_condense: K >= 1, hess [C * (G - 1) * 496], prior empty or [C * G * 136], lambda empty or [C]");
    CondensedChains r;
    r.Gr = cpi_chain_condense_states(G, K);
    r.rhess.assign((size_t)(C * (r.Gr - 1)) * 496 + 1, 0.0);       // + 1: G == 1 has no reduced factor, and data() stays a pointer
    r.rprior.assign((size_t)(C * r.Gr) * 136, 0.0);
    r.workspace.assign(cpi_chain_condense_workspace_doubles(C * G), 0.0);
    r.rcount.assign((size_t)C, 0);
    r.status.assign((size_t)(C * (r.Gr - 1)), 0);
    static const double none = 0.0;      // G == 1: no factor rows; G > 1 with C == 0: never read
    ctx.check(cpi_chain_condense_batch_host(ctx.get(), C, G, C * G, C * (G - 1), nullptr, nullptr, nullptr, hess.empty() ? &none : hess.data(),
                                            prior.empty() ? nullptr : prior.data(), lambda.empty() ? nullptr : lambda.data(),
                                            diagonal ? CPI_DAMP_DIAGONAL : CPI_DAMP_IDENTITY, K, r.rhess.data(), r.rprior.data(), r.rcount.data(),
                                            r.status.empty() ? nullptr : r.status.data(), r.workspace.data()));
    r.rhess.pop_back();
    return r;
}
inline std::vector<double> chain_expand(const Context &ctx, int64_t C, int64_t G, int64_t K, const std::vector<double> &rdelta,
                                        const std::vector<double> &workspace) {
    if (C < 0 || G < 1 || K < 1 || rdelta.size() != (size_t)(C * cpi_chain_condense_states(G, K)) * 15 ||
        workspace.size() < cpi_chain_condense_workspace_doubles(C * G))
        throw std::invalid_argument("cpi_host::chain_expand: K >= 1, rdelta [C * Gr * 15], workspace as chain_condense returned it");
    std::vector<double> delta((size_t)(C * G) * 15 + 1, 0.0);
    ctx.check(cpi_chain_expand_batch_host(ctx.get(), C, G, C * G, nullptr, nullptr, K, rdelta.empty() ? delta.data() + delta.size() - 1 : rdelta.data(),
                                          workspace.data(), delta.data()));
    delta.pop_back();
    return delta;
}
// The three calls: condense at segment length K, the reduced solve, expand.  Returns delta [C * G * 15], chain_solve's result to
// rounding; status, when given, receives the REDUCED solve's per-chain codes (a failed chain's rows are NaN).
inline std::vector<double> chain_solve_segmented(const Context &ctx, int64_t C, int64_t G, int64_t K, const std::vector<double> &hess,
                                                 const std::vector<double> &prior = {}, const std::vector<double> &lambda = {},
                                                 bool diagonal = false, std::vector<int32_t> *status = nullptr) {
    const CondensedChains r = chain_condense(ctx, C, G, K, hess, prior, lambda, diagonal);
    std::vector<double> rdelta((size_t)(C * r.Gr) * 15 + 1, 0.0);
    std::vector<int32_t> st((size_t)C + 1, 0);
    static const double none = 0.0;
    ctx.check(cpi_chain_solve_batch_host(ctx.get(), C, r.Gr, C * r.Gr, C * (r.Gr - 1), nullptr, r.rcount.data(), nullptr,
                                         r.rhess.empty() ? &none : r.rhess.data(), r.rprior.empty() ? &none : r.rprior.data(), nullptr,
                                         CPI_DAMP_IDENTITY, rdelta.data(), st.data()));
    rdelta.pop_back();
    st.pop_back();
    if (status) *status = st;
    return chain_expand(ctx, C, G, K, rdelta, r.workspace);
}

// The Levenberg-Marquardt step per chain (cpi_prior_relinearize_batch_host, cpi_chain_cost_batch_host, cpi_chain_accept_batch_host: the
// device kernels' bits), for C chains of G states back to back.
// prior_relinearize: the priors of P records at `states` [S * 16] -- anchor [P * 16] the state each was linearised at, prior0 [P * 136]
// = [Lam eta0; . .], idx empty (record p belongs to state p) or [P].  Returns the prior rows [S * 136] chain_solve takes and pcost [S];
// rows of states without a record are zero.
struct PriorRows {
    std::vector<double> prior, pcost;
};
inline PriorRows prior_relinearize(const Context &ctx, const std::vector<double> &states, const std::vector<double> &anchor,
                                   const std::vector<double> &prior0, const std::vector<int32_t> &idx = {}) {
    const size_t S = states.size() / 16, P = anchor.size() / 16;
    if (states.size() != S * 16 || anchor.size() != P * 16 || prior0.size() != P * 136 || (!idx.empty() && idx.size() != P) || (idx.empty() && P > S))
        throw std::invalid_argument("cpi_host::prior_relinearize: states [S * 16], anchor [P * 16], prior0 [P * 136], idx empty (P <= S) or [P]");
    PriorRows r;
    r.prior.assign(S * 136, 0.0);
    r.pcost.assign(S, 0.0);
    if (P && S)
        ctx.check(cpi_prior_relinearize_batch_host(ctx.get(), (int64_t)S, (int64_t)P, idx.empty() ? nullptr : idx.data(), states.data(), anchor.data(),
                                                   prior0.data(), r.prior.data(), r.pcost.data()));
    return r;
}
// chain_cost: cost[c] = 0.5 sum of the chain's chi2 rows + the sum of its pcost rows, in the fixed summation shape of include/cpi_amd.h.
// chi2 [C * (G - 1)] (cpi_factor_cost_*), pcost empty or [C * G].
inline std::vector<double> chain_cost(const Context &ctx, int64_t C, int64_t G, const std::vector<double> &chi2, const std::vector<double> &pcost = {}) {
    if (C < 0 || G < 1 || chi2.size() != (size_t)(C * (G - 1)) || (!pcost.empty() && pcost.size() != (size_t)(C * G)))
        throw std::invalid_argument("cpi_host::chain_cost: chi2 [C * (G - 1)], pcost empty or [C * G]");
    std::vector<double> cost((size_t)C);
    static const double none = 0.0;      // G == 1: no factor rows; G > 1 with C == 0: never read
    ctx.check(cpi_chain_cost_batch_host(ctx.get(), C, G, C * G, C * (G - 1), nullptr, nullptr, nullptr, chi2.empty() ? &none : chi2.data(),
                                        pcost.empty() ? nullptr : pcost.data(), cost.data()));
    return cost;
}
// chain_accept: the decision, on what the loop keeps per chain.  st is updated in place as include/cpi_amd.h says (an accepted chain
// takes the trial's rows, the new cost and a smaller lambda; a rejected one a larger lambda; phase: CPI_LM_*); returns accepted [C].
// params NULL: the library's defaults.
struct LmState {
    std::vector<double> cost, states, chi2, lambda;   // [C], [C * G * 16], [C * (G - 1)] or empty (not kept), [C]
    std::vector<int32_t> phase;                       // [C]
};
inline std::vector<int32_t> chain_accept(const Context &ctx, int64_t C, int64_t G, const std::vector<double> &chi2_new,
                                         const std::vector<double> &pcost_new, const std::vector<double> &trial, LmState &st,
                                         const cpi_lm_params *params = nullptr) {
    if (C < 0 || G < 1 || chi2_new.size() != (size_t)(C * (G - 1)) || (!pcost_new.empty() && pcost_new.size() != (size_t)(C * G)) ||
        trial.size() != (size_t)(C * G) * 16 || st.states.size() != trial.size() || st.cost.size() != (size_t)C || st.lambda.size() != (size_t)C ||
        st.phase.size() != (size_t)C || (!st.chi2.empty() && st.chi2.size() != chi2_new.size()))
        throw std::invalid_argument("cpi_host::chain_accept: chi2_new [C * (G - 1)], pcost_new empty or [C * G], trial and st.states [C * G * 16], "
                                    "st.cost / lambda / phase [C], st.chi2 empty or [C * (G - 1)]");
    std::vector<int32_t> accepted((size_t)C, 0);
    static const double none = 0.0;
    ctx.check(cpi_chain_accept_batch_host(ctx.get(), C, G, C * G, C * (G - 1), nullptr, nullptr, nullptr, params,
                                          chi2_new.empty() ? &none : chi2_new.data(), pcost_new.empty() ? nullptr : pcost_new.data(), trial.data(),
                                          st.cost.data(), st.states.data(), st.chi2.empty() ? nullptr : st.chi2.data(), st.lambda.data(),
                                          st.phase.data(), accepted.data()));
    return accepted;
}

// state_fix: absolute measurements of states (cpi_state_fix_batch_host: the device kernel's bits).  kind CPI_FIX_*; z [M * 3 | 3 | 4 | 7]
// and R [M * 6 | 6 | 6 | 21] (the packed upper-triangular square-root information) for M fixes sorted by state, mfirst [S + 1] the
// first fix of every state; weight empty or [M]; base empty or [S * 136], pcost_base empty or [S]: what an earlier sensor or
// prior_relinearize wrote.  Returns the rows [S * 136] chain_solve takes as prior, pcost [S] and chi2 [M] (without the weight).
struct FixRows {
    std::vector<double> rows, pcost, chi2;
};
inline FixRows state_fix(const Context &ctx, int32_t kind, const std::vector<double> &states, const std::vector<double> &z, const std::vector<double> &R,
                         const std::vector<int64_t> &mfirst, const std::vector<double> &weight = {}, const std::vector<double> &base = {},
                         const std::vector<double> &pcost_base = {}) {
    static const size_t zn[4] = {3, 3, 4, 7}, rn[4] = {6, 6, 6, 21};
    if (kind < CPI_FIX_POSITION || kind > CPI_FIX_POSE) throw std::invalid_argument("cpi_host::state_fix: kind is CPI_FIX_POSITION .. CPI_FIX_POSE");
    const size_t S = states.size() / 16, M = z.size() / zn[kind];
    if (states.size() != S * 16 || z.size() != M * zn[kind] || R.size() != M * rn[kind] || mfirst.size() != S + 1 || (!weight.empty() && weight.size() != M) ||
        (!base.empty() && base.size() != S * 136) || (!pcost_base.empty() && pcost_base.size() != S))
        throw std::invalid_argument("cpi_host::state_fix: states [S * 16], z [M * 3 | 3 | 4 | 7], R [M * 6 | 6 | 6 | 21], mfirst [S + 1], weight empty or [M], "
                                    "base empty or [S * 136], pcost_base empty or [S]");
    FixRows r;
    r.rows.assign(S * 136, 0.0);
    r.pcost.assign(S, 0.0);
    r.chi2.assign(M, 0.0);
    if (S)
        ctx.check(cpi_state_fix_batch_host(ctx.get(), (int64_t)S, (int64_t)M, kind, mfirst.data(), states.data(), M ? z.data() : nullptr, M ? R.data() : nullptr,
                                           weight.empty() ? nullptr : weight.data(), base.empty() ? nullptr : base.data(),
                                           pcost_base.empty() ? nullptr : pcost_base.data(), r.rows.data(), r.pcost.data(), M ? r.chi2.data() : nullptr));
    return r;
}

// state_between: measurements between the two consecutive states of IMU factors (cpi_state_between_batch_host: the device kernel's
// bits).  kind CPI_BETWEEN_*; z [M * 3 | 4 | 7] and R [M * 6 | 6 | 21] (the packed upper-triangular square-root information) for M
// measurements sorted by factor, mfirst [F + 1] the first measurement of every factor; idx_i / idx_j empty (factor f joins the states
// f and f + 1) or [F]; weight empty or [M]; hess_base empty or [F * 496] (what factor_hessian wrote), chi2_base empty or [F].  Returns
// the rows [F * 496] chain_solve takes as hess, chi2 [F] and chi2_m [M] (without the weight).
struct BetweenRows {
    std::vector<double> rows, chi2, chi2_m;
};
inline BetweenRows state_between(const Context &ctx, int32_t kind, const std::vector<double> &states, const std::vector<double> &z,
                                 const std::vector<double> &R, const std::vector<int64_t> &mfirst, const std::vector<int32_t> &idx_i = {},
                                 const std::vector<int32_t> &idx_j = {}, const std::vector<double> &weight = {},
                                 const std::vector<double> &hess_base = {}, const std::vector<double> &chi2_base = {}) {
    static const size_t zn[3] = {3, 4, 7}, rn[3] = {6, 6, 21};
    if (kind < CPI_BETWEEN_POSITION || kind > CPI_BETWEEN_POSE)
        throw std::invalid_argument("cpi_host::state_between: kind is CPI_BETWEEN_POSITION .. CPI_BETWEEN_POSE");
    const size_t S = states.size() / 16, M = z.size() / zn[kind], F = mfirst.empty() ? 0 : mfirst.size() - 1;
    if (states.size() != S * 16 || z.size() != M * zn[kind] || R.size() != M * rn[kind] || mfirst.size() != F + 1 || (!idx_i.empty() && idx_i.size() != F) ||
        (!idx_j.empty() && idx_j.size() != F) || (!weight.empty() && weight.size() != M) || (!hess_base.empty() && hess_base.size() != F * 496) ||
        (!chi2_base.empty() && chi2_base.size() != F))
        throw std::invalid_argument("cpi_host::state_between: states [S * 16], z [M * 3 | 4 | 7], R [M * 6 | 6 | 21], mfirst [F + 1], idx_i / idx_j empty or "
                                    "[F], weight empty or [M], hess_base empty or [F * 496], chi2_base empty or [F]");
    BetweenRows r;
    r.rows.assign(F * 496, 0.0);
    r.chi2.assign(F, 0.0);
    r.chi2_m.assign(M, 0.0);
    if (F)
        ctx.check(cpi_state_between_batch_host(ctx.get(), (int64_t)F, (int64_t)M, kind, mfirst.data(), states.data(), (int64_t)S,
                                               idx_i.empty() ? nullptr : idx_i.data(), idx_j.empty() ? nullptr : idx_j.data(), M ? z.data() : nullptr,
                                               M ? R.data() : nullptr, weight.empty() ? nullptr : weight.data(), hess_base.empty() ? nullptr : hess_base.data(),
                                               chi2_base.empty() ? nullptr : chi2_base.data(), r.rows.data(), r.chi2.data(), M ? r.chi2_m.data() : nullptr));
    return r;
}

// ---- the caller's loop for MANY windows at once --------------------------------------------------------------------
// What GraphSolver keeps between two states is a deque of IMU readings (GraphSolver.h: imu_times / imu_linaccs /
// imu_angvel, filled by addmeasurement_imu); createimufactor_cpi_v1 / _v2 (GraphSolver_IMU.cpp:34-134) walk it up to the
// update time, feed a CpiV1 / CpiV2 and read its members.  ImuStream is that deque as one array, and preintegrate() is that
// loop for EVERY update time in one call: the stream goes to the device once, the kernels cut the windows themselves
// (cpi_preintegrate_stream_host), one CpiResult per update time comes back -- window u covers (update[u-1], update[u]]
// (the first one starts at the stream's first reading), its tail interval holds the front reading until the update time.
class ImuStream {
public:
    void push(double t, const Vec3 &w, const Vec3 &a) {           // GraphSolver::addmeasurement_imu
        knots_.push_back(t);
        for (int i = 0; i < 3; i++) knots_.push_back(w[i]);
        for (int i = 0; i < 3; i++) knots_.push_back(a[i]);
    }
    void assign(const std::vector<double> &knots) { knots_ = knots; }   // e.g. parse_imu_text's records
    size_t size() const { return knots_.size() / 7; }
    const std::vector<double> &knots() const { return knots_; }
    // prm: cpi_params as CpiBase::params() builds them (model, sigmas, gravity, flags).  lin [U][6] = b_w_lin, b_a_lin per window;
    // q_k_lin [U][4] (model 2; may be empty otherwise).  counts (optional) receives every window's interval count.
    // A window longer than max_intervals (default: as long as the stream) is an error, not a truncation.
    std::vector<CpiResult> preintegrate(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times,
                                        const std::vector<double> &lin, const std::vector<double> &q_k_lin = std::vector<double>(),
                                        std::vector<int32_t> *counts = nullptr, int32_t max_intervals = 0) const {
        const int64_t U = (int64_t)update_times.size(), K = (int64_t)size();
        if ((int64_t)lin.size() != U * 6) throw std::runtime_error("ImuStream::preintegrate: lin must hold 6 doubles per update time");
        if (!q_k_lin.empty() && (int64_t)q_k_lin.size() != U * 4) throw std::runtime_error("ImuStream::preintegrate: q_k_lin must hold 4 doubles per update time");
        std::vector<CpiResult> res((size_t)U);
        if (U == 0) return res;
        const int32_t N = max_intervals > 0 ? max_intervals : (int32_t)std::min<int64_t>(std::max<int64_t>(K, 1), 65535);
        std::vector<double> DT(U), al(U * 3), be(U * 3), q(U * 4), Jq(U * 9), Ja(U * 9), Jb(U * 9), Ha(U * 9), Hb(U * 9), Oa(U * 9),
            Ob(U * 9), P(U * 225);
        cpi_outputs o{ DT.data(), al.data(), be.data(), q.data(), Jq.data(), Ja.data(), Jb.data(), Ha.data(), Hb.data(),
                       prm.model == CPI_MODEL_V2 ? Oa.data() : nullptr, prm.model == CPI_MODEL_V2 ? Ob.data() : nullptr, P.data() };
        std::vector<int32_t> cnt((size_t)U);
        ctx.check(cpi_preintegrate_stream_host(ctx.get(), &prm, K, knots_.data(), U, update_times.data(), N, lin.data(),
                                               q_k_lin.empty() ? nullptr : q_k_lin.data(), &o, cnt.data()));
        for (int64_t u = 0; u < U; u++)
            if (cnt[u] > N) throw std::runtime_error("ImuStream::preintegrate: window " + std::to_string(u) + " holds " + std::to_string(cnt[u]) +
                                                     " intervals, more than max_intervals = " + std::to_string(N));
        for (int64_t w = 0; w < U; w++) {
            CpiResult &r = res[w];
            r.DT = DT[w];
            for (int i = 0; i < 3; i++) { r.alpha_tau[i] = al[w * 3 + i]; r.beta_tau[i] = be[w * 3 + i]; }
            for (int i = 0; i < 4; i++) r.q_k2tau[i] = q[w * 4 + i];
            for (int i = 0; i < 9; i++) {
                r.J_q[i] = Jq[w * 9 + i]; r.J_a[i] = Ja[w * 9 + i]; r.J_b[i] = Jb[w * 9 + i]; r.H_a[i] = Ha[w * 9 + i];
                r.H_b[i] = Hb[w * 9 + i]; r.O_a[i] = Oa[w * 9 + i]; r.O_b[i] = Ob[w * 9 + i];
            }
            for (int i = 0; i < 225; i++) r.P_meas[i] = P[w * 225 + i];
        }
        if (counts) *counts = cnt;
        return res;
    }
    // The reference's members after EVERY feed_IMU of every window (cpi_preintegrate_stream_running_host): result[u][i] = window u
    // after interval i, one per interval of the window's TRUE count (as CpiBatch::running returns one per recorded interval); a
    // skipped interval (dt <= 0) repeats the previous one.  Models 1 and 2; the bias Jacobians are filled for model 1 only.
    // The call returns U * max_intervals rows, so the default bound (max_intervals = 0) is TIGHT: the longest window, found on
    // the host from the stamps.  A window longer than max_intervals is an error, not a truncation.
    std::vector<std::vector<CpiResult>> running(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times,
                                                const std::vector<double> &lin, const std::vector<double> &q_k_lin = std::vector<double>(),
                                                std::vector<int32_t> *counts = nullptr, int32_t max_intervals = 0) const {
        const int64_t U = (int64_t)update_times.size(), K = (int64_t)size();
        if ((int64_t)lin.size() != U * 6) throw std::runtime_error("ImuStream::running: lin must hold 6 doubles per update time");
        if (!q_k_lin.empty() && (int64_t)q_k_lin.size() != U * 4) throw std::runtime_error("ImuStream::running: q_k_lin must hold 4 doubles per update time");
        std::vector<std::vector<CpiResult>> res((size_t)U);
        if (counts) counts->assign((size_t)U, 0);
        if (U == 0) return res;
        const int32_t N = max_intervals > 0 ? max_intervals : longest_window(knots_.data(), (size_t)K, update_times.data(), (size_t)U);
        RunningRows rows;
        cpi_outputs o = rows.bind(prm.model, U, N);
        std::vector<int32_t> cnt((size_t)U, 0);
        // (N == 0: no window holds an interval -- or the stream is empty, which the entry refuses as preintegrate()'s does)
        if (N > 0 || K == 0)
            ctx.check(cpi_preintegrate_stream_running_host(ctx.get(), &prm, K, knots_.data(), U, update_times.data(), std::max<int32_t>(N, 1),
                                                           lin.data(), q_k_lin.empty() ? nullptr : q_k_lin.data(), &o, cnt.data()));
        for (int64_t u = 0; u < U; u++) {
            if (cnt[u] > N) throw std::runtime_error("ImuStream::running: window " + std::to_string(u) + " holds " + std::to_string(cnt[u]) +
                                                     " intervals, more than max_intervals = " + std::to_string(N));
            res[u] = rows.window(u, cnt[u]);
        }
        if (counts) *counts = cnt;
        return res;
    }
    // The members at ABSOLUTE times (cpi_query_stream_batch_host; the lidar points of a sweep, keyframes chosen after the fact):
    // result[k] = the window that holds times[k] -- the first whose update time is not before it, the last one for a later time --
    // at that time, as CpiBatch::at returns it for a window it was given: on a stamp what running() holds there, inside an interval
    // that state advanced with the reading held, at or past the window's end its measurement.  Nothing is assembled on the host.
    // windows (optional) receives the window of every time.  A window longer than max_intervals (default: the longest window, found
    // on the host from the stamps) is queried as truncated to it.  Models 1 and 2; the bias Jacobians are filled for model 1 only,
    // P_meas by at_cov / at_stj, model 2's seven Jacobians by at_stj (prm.state_transition_jacobians set).
    std::vector<CpiResult> at(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times, const std::vector<double> &lin,
                              const std::vector<double> &times, const std::vector<double> &q_k_lin = std::vector<double>(),
                              std::vector<int32_t> *windows = nullptr, int32_t max_intervals = 0) const {
        return at_impl(ctx, prm, update_times, lin, times, q_k_lin, windows, max_intervals, false, false);
    }
    std::vector<CpiResult> at_cov(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times, const std::vector<double> &lin,
                                  const std::vector<double> &times, const std::vector<double> &q_k_lin = std::vector<double>(),
                                  std::vector<int32_t> *windows = nullptr, int32_t max_intervals = 0) const {
        return at_impl(ctx, prm, update_times, lin, times, q_k_lin, windows, max_intervals, true, false);
    }
    std::vector<CpiResult> at_stj(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times, const std::vector<double> &lin,
                                  const std::vector<double> &times, const std::vector<double> &q_k_lin = std::vector<double>(),
                                  std::vector<int32_t> *windows = nullptr, int32_t max_intervals = 0) const {
        return at_impl(ctx, prm, update_times, lin, times, q_k_lin, windows, max_intervals, true, true);
    }
private:
    std::vector<CpiResult> at_impl(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times, const std::vector<double> &lin,
                                   const std::vector<double> &times, const std::vector<double> &q_k_lin, std::vector<int32_t> *windows,
                                   int32_t max_intervals, bool cov, bool stj) const {
        const size_t U = update_times.size();
        if (lin.size() != U * 6) throw std::runtime_error("ImuStream::at: lin must hold 6 doubles per update time");
        if (!q_k_lin.empty() && q_k_lin.size() != U * 4) throw std::runtime_error("ImuStream::at: q_k_lin must hold 4 doubles per update time");
        const int32_t N = max_intervals > 0 ? max_intervals : longest_window(knots_.data(), size(), update_times.data(), U);
        return query_stream_results(ctx, prm, 1, knots_, nullptr, update_times, nullptr, N, lin, q_k_lin, nullptr, times, cov, stj, windows);
    }
    std::vector<double> knots_;
};

// Many trajectories at once: one ImuStream per run (e.g. per dataset of a Monte-Carlo batch), each with its own update times,
// preintegrated by ONE call (cpi_preintegrate_streams_host) -- every run's clock may start at 0.  preintegrate() returns, per
// run, one CpiResult per update time of that run, equal to what that run's ImuStream::preintegrate would return with the same
// bound and lane split (prm.lanes_per_window: the automatic choice depends on the total number of windows).
class ImuStreamSet {
public:
    // the run's readings and its update times (non-decreasing); lin [U_r][6] and q_k_lin [U_r][4] (model 2) per window
    void add_run(const ImuStream &run, const std::vector<double> &update_times, const std::vector<double> &lin,
                 const std::vector<double> &q_k_lin = std::vector<double>()) {
        if (lin.size() != update_times.size() * 6) throw std::runtime_error("ImuStreamSet::add_run: lin must hold 6 doubles per update time");
        if (!q_k_lin.empty() && q_k_lin.size() != update_times.size() * 4) throw std::runtime_error("ImuStreamSet::add_run: q_k_lin must hold 4 doubles per update time");
        knots_.insert(knots_.end(), run.knots().begin(), run.knots().end());
        ut_.insert(ut_.end(), update_times.begin(), update_times.end());
        lin_.insert(lin_.end(), lin.begin(), lin.end());
        qk_.insert(qk_.end(), q_k_lin.begin(), q_k_lin.end());
        soff_.push_back((int64_t)(knots_.size() / 7));
        uoff_.push_back((int64_t)ut_.size());
        runs_.push_back(update_times.size());
    }
    size_t runs() const { return runs_.size(); }
    // counts (optional) receives every window's interval count, per run.  A window longer than max_intervals (default: as
    // long as the longest run) is an error, not a truncation.
    std::vector<std::vector<CpiResult>> preintegrate(const Context &ctx, const cpi_params &prm,
                                                     std::vector<std::vector<int32_t>> *counts = nullptr, int32_t max_intervals = 0) const {
        const int64_t R = (int64_t)runs_.size(), K = (int64_t)(knots_.size() / 7), U = (int64_t)ut_.size();
        std::vector<std::vector<CpiResult>> res((size_t)R);
        for (int64_t r = 0; r < R; r++) res[r].resize(runs_[r]);
        if (counts) { counts->assign((size_t)R, std::vector<int32_t>()); }
        if (U == 0) return res;
        if (!qk_.empty() && qk_.size() != ut_.size() * 4) throw std::runtime_error("ImuStreamSet::preintegrate: q_k_lin given for some runs and not for others");
        int64_t longest = 1;
        for (int64_t r = 0; r < R; r++) longest = std::max<int64_t>(longest, soff_[r + 1] - soff_[r]);
        const int32_t N = max_intervals > 0 ? max_intervals : (int32_t)std::min<int64_t>(longest, 65535);
        std::vector<double> DT(U), al(U * 3), be(U * 3), q(U * 4), Jq(U * 9), Ja(U * 9), Jb(U * 9), Ha(U * 9), Hb(U * 9), Oa(U * 9),
            Ob(U * 9), P(U * 225);
        cpi_outputs o{ DT.data(), al.data(), be.data(), q.data(), Jq.data(), Ja.data(), Jb.data(), Ha.data(), Hb.data(),
                       prm.model == CPI_MODEL_V2 ? Oa.data() : nullptr, prm.model == CPI_MODEL_V2 ? Ob.data() : nullptr, P.data() };
        std::vector<int32_t> cnt((size_t)U);
        ctx.check(cpi_preintegrate_streams_host(ctx.get(), &prm, R, K, knots_.data(), soff_.data(), U, ut_.data(), uoff_.data(), N,
                                                lin_.data(), qk_.empty() ? nullptr : qk_.data(), &o, cnt.data()));
        for (int64_t u = 0; u < U; u++)
            if (cnt[u] > N) throw std::runtime_error("ImuStreamSet::preintegrate: window " + std::to_string(u) + " holds " + std::to_string(cnt[u]) +
                                                     " intervals, more than max_intervals = " + std::to_string(N));
        for (int64_t r = 0; r < R; r++) {
            for (int64_t j = 0; j < (int64_t)runs_[r]; j++) {
                const int64_t w = uoff_[r] + j;
                CpiResult &x = res[r][j];
                x.DT = DT[w];
                for (int i = 0; i < 3; i++) { x.alpha_tau[i] = al[w * 3 + i]; x.beta_tau[i] = be[w * 3 + i]; }
                for (int i = 0; i < 4; i++) x.q_k2tau[i] = q[w * 4 + i];
                for (int i = 0; i < 9; i++) {
                    x.J_q[i] = Jq[w * 9 + i]; x.J_a[i] = Ja[w * 9 + i]; x.J_b[i] = Jb[w * 9 + i]; x.H_a[i] = Ha[w * 9 + i];
                    x.H_b[i] = Hb[w * 9 + i]; x.O_a[i] = Oa[w * 9 + i]; x.O_b[i] = Ob[w * 9 + i];
                }
                for (int i = 0; i < 225; i++) x.P_meas[i] = P[w * 225 + i];
            }
            if (counts) (*counts)[r].assign(cnt.begin() + uoff_[r], cnt.begin() + uoff_[r + 1]);
        }
        return res;
    }
    // ImuStream::running for every run in ONE call (cpi_preintegrate_streams_running_host): result[r][j][i] = window j of run r
    // after interval i.  The default bound is the longest window of any run (found on the host from the stamps); a window longer
    // than max_intervals is an error.
    std::vector<std::vector<std::vector<CpiResult>>> running(const Context &ctx, const cpi_params &prm,
                                                             std::vector<std::vector<int32_t>> *counts = nullptr,
                                                             int32_t max_intervals = 0) const {
        const int64_t R = (int64_t)runs_.size(), K = (int64_t)(knots_.size() / 7), U = (int64_t)ut_.size();
        std::vector<std::vector<std::vector<CpiResult>>> res((size_t)R);
        for (int64_t r = 0; r < R; r++) res[r].resize(runs_[r]);
        if (counts) { counts->assign((size_t)R, std::vector<int32_t>()); for (int64_t r = 0; r < R; r++) (*counts)[r].assign(runs_[r], 0); }
        if (U == 0) return res;
        if (!qk_.empty() && qk_.size() != ut_.size() * 4) throw std::runtime_error("ImuStreamSet::running: q_k_lin given for some runs and not for others");
        int32_t N = max_intervals;
        if (N <= 0)
            for (int64_t r = 0; r < R; r++)
                N = std::max(N, longest_window(knots_.data() + soff_[r] * 7, (size_t)(soff_[r + 1] - soff_[r]), ut_.data() + uoff_[r], runs_[r]));
        RunningRows rows;
        cpi_outputs o = rows.bind(prm.model, U, N);
        std::vector<int32_t> cnt((size_t)U, 0);
        if (N > 0 || K == 0)
            ctx.check(cpi_preintegrate_streams_running_host(ctx.get(), &prm, R, K, knots_.data(), soff_.data(), U, ut_.data(), uoff_.data(),
                                                            std::max<int32_t>(N, 1), lin_.data(), qk_.empty() ? nullptr : qk_.data(), &o,
                                                            cnt.data()));
        for (int64_t r = 0; r < R; r++)
            for (int64_t j = 0; j < (int64_t)runs_[r]; j++) {
                const int64_t w = uoff_[r] + j;
                if (cnt[w] > N) throw std::runtime_error("ImuStreamSet::running: window " + std::to_string(w) + " holds " + std::to_string(cnt[w]) +
                                                         " intervals, more than max_intervals = " + std::to_string(N));
                res[r][j] = rows.window(w, cnt[w]);
                if (counts) (*counts)[r][j] = cnt[w];
            }
        return res;
    }
    // ImuStream::at / at_cov / at_stj for the runs of the set in ONE call: result[k] = run runs[k] at the absolute time times[k] (of
    // that run's clock).  windows (optional) receives the GLOBAL window index of every time, -1 (and NaN members) for a run without
    // update times; a run index outside the set is an error.
    std::vector<CpiResult> at(const Context &ctx, const cpi_params &prm, const std::vector<int32_t> &runs, const std::vector<double> &times,
                              std::vector<int32_t> *windows = nullptr, int32_t max_intervals = 0) const {
        return at_impl(ctx, prm, runs, times, windows, max_intervals, false, false);
    }
    std::vector<CpiResult> at_cov(const Context &ctx, const cpi_params &prm, const std::vector<int32_t> &runs, const std::vector<double> &times,
                                  std::vector<int32_t> *windows = nullptr, int32_t max_intervals = 0) const {
        return at_impl(ctx, prm, runs, times, windows, max_intervals, true, false);
    }
    std::vector<CpiResult> at_stj(const Context &ctx, const cpi_params &prm, const std::vector<int32_t> &runs, const std::vector<double> &times,
                                  std::vector<int32_t> *windows = nullptr, int32_t max_intervals = 0) const {
        return at_impl(ctx, prm, runs, times, windows, max_intervals, true, true);
    }
private:
    std::vector<CpiResult> at_impl(const Context &ctx, const cpi_params &prm, const std::vector<int32_t> &runs, const std::vector<double> &times,
                                   std::vector<int32_t> *windows, int32_t max_intervals, bool cov, bool stj) const {
        if (runs.size() != times.size()) throw std::runtime_error("ImuStreamSet::at: one run index per time");
        if (!qk_.empty() && qk_.size() != ut_.size() * 4) throw std::runtime_error("ImuStreamSet::at: q_k_lin given for some runs and not for others");
        const int64_t R = (int64_t)runs_.size();
        int32_t N = max_intervals;
        if (N <= 0)
            for (int64_t r = 0; r < R; r++)
                N = std::max(N, longest_window(knots_.data() + soff_[r] * 7, (size_t)(soff_[r + 1] - soff_[r]), ut_.data() + uoff_[r], runs_[r]));
        return query_stream_results(ctx, prm, R, knots_, soff_.data(), ut_, uoff_.data(), N, lin_, qk_, runs.data(), times, cov, stj, windows);
    }
    std::vector<double> knots_, ut_, lin_, qk_;
    std::vector<int64_t> soff_{0}, uoff_{0};   // [R + 1]
    std::vector<size_t> runs_;                 // update times per run
};

// evaluateError-shaped evaluator (ImuFactorCPIv1.h:139 / ImuFactorCPIv2.h:151).  state = 16 doubles
// [q(4) bg(3) v(3) ba(3) p(3)]; error[15]; H1/H2 column-major 15x15, may be nullptr.
class ImuFactorCPI {
public:
    // built straight from a finished preintegrator, with the field->ctor mapping of GraphSolver_IMU.cpp:74-75,129-130
    explicit ImuFactorCPI(const CpiBase &cpi) : model_(cpi.factor_model()), m_(cpi.result()), grav_(cpi.grav), qk_(cpi.q_k_lin) {
        for (int i = 0; i < 3; i++) { lin_[i] = cpi.b_w_lin[i]; lin_[3 + i] = cpi.b_a_lin[i]; }
    }
    // the reference's constructor shape (ImuFactorCPIv1.h:78-81 / ImuFactorCPIv2.h:82-85 without the two keys), so that the last
    // line of createimufactor_cpi_v1 (GraphSolver_IMU.cpp:74-75) keeps its argument list:
    //   ImuFactorCPI(cpi.P_meas, cpi.DT, cpi.grav, cpi.alpha_tau, cpi.beta_tau, cpi.q_k2tau, cpi.b_a_lin, cpi.b_w_lin,
    //                cpi.J_q, cpi.J_b, cpi.J_a, cpi.H_b, cpi.H_a)                                    model 1
    //   ImuFactorCPI(..., cpi.q_k2tau, cpi.q_k_lin, cpi.b_a_lin, ..., cpi.H_a, cpi.O_b, cpi.O_a)     model 2 (:129-130)
    ImuFactorCPI(const Mat15 &covariance, double deltatime, const Vec3 &grav, const Vec3 &alpha, const Vec3 &beta, const Vec4 &q_KtoK1,
                 const Vec3 &ba_lin, const Vec3 &bg_lin, const Mat3 &J_q, const Mat3 &J_beta, const Mat3 &J_alpha, const Mat3 &H_beta,
                 const Mat3 &H_alpha)
        : model_(CPI_MODEL_V1), grav_(grav), qk_(Vec4{{0, 0, 0, 1}}) {
        m_.P_meas = covariance; m_.DT = deltatime; m_.alpha_tau = alpha; m_.beta_tau = beta; m_.q_k2tau = q_KtoK1;
        m_.J_q = J_q; m_.J_b = J_beta; m_.J_a = J_alpha; m_.H_b = H_beta; m_.H_a = H_alpha;
        for (int i = 0; i < 3; i++) { lin_[i] = bg_lin[i]; lin_[3 + i] = ba_lin[i]; }
    }
    ImuFactorCPI(const Mat15 &covariance, double deltatime, const Vec3 &grav, const Vec3 &alpha, const Vec3 &beta, const Vec4 &q_KtoK1,
                 const Vec4 &q_K_lin, const Vec3 &ba_lin, const Vec3 &bg_lin, const Mat3 &J_q, const Mat3 &J_beta, const Mat3 &J_alpha,
                 const Mat3 &H_beta, const Mat3 &H_alpha, const Mat3 &O_beta, const Mat3 &O_alpha)
        : model_(CPI_MODEL_V2), grav_(grav), qk_(q_K_lin) {
        m_.P_meas = covariance; m_.DT = deltatime; m_.alpha_tau = alpha; m_.beta_tau = beta; m_.q_k2tau = q_KtoK1;
        m_.J_q = J_q; m_.J_b = J_beta; m_.J_a = J_alpha; m_.H_b = H_beta; m_.H_a = H_alpha; m_.O_b = O_beta; m_.O_a = O_alpha;
        for (int i = 0; i < 3; i++) { lin_[i] = bg_lin[i]; lin_[3 + i] = ba_lin[i]; }
    }
    // from a window of ImuStream::preintegrate: the measurement, the model (1 / 2) and the linearisation point it was made with
    ImuFactorCPI(int model, const CpiResult &meas, const Vec3 &grav, const Vec3 &b_w_lin, const Vec3 &b_a_lin, const Vec4 &q_k_lin = Vec4{{0, 0, 0, 1}})
        : model_(model == CPI_MODEL_FORSTER ? CPI_MODEL_V1 : model), m_(meas), grav_(grav), qk_(q_k_lin) {
        for (int i = 0; i < 3; i++) { lin_[i] = b_w_lin[i]; lin_[3 + i] = b_a_lin[i]; }
    }
    void evaluateError(const Context &ctx, const double *state_i, const double *state_j, double *error, double *H1 = nullptr,
                       double *H2 = nullptr) {
        double states[32];
        for (int i = 0; i < 16; i++) { states[i] = state_i[i]; states[16 + i] = state_j[i]; }
        cpi_outputs o = CpiBase::outputs_of(m_);
        ctx.check(cpi_factor_eval_batch_host(ctx.get(), model_, grav_.data(), 1, &o, lin_, qk_.data(), states, 2, nullptr, nullptr,
                                             error, H1, H2));
    }
    // GTSAM's NoiseModelFactor::error(values) = 0.5 |R e|^2 at the two states, R = chol_upper(P_meas^-1) of the factor's own
    // covariance, factorised on the device (cpi_factor_cost_batch_host): what an optimiser accepts or rejects a step by.
    double error(const Context &ctx, const double *state_i, const double *state_j) {
        double states[32], chi2 = 0.0, total = 0.0;
        for (int i = 0; i < 16; i++) { states[i] = state_i[i]; states[16 + i] = state_j[i]; }
        cpi_outputs o = CpiBase::outputs_of(m_);
        ctx.check(cpi_factor_cost_batch_host(ctx.get(), model_, grav_.data(), 1, &o, lin_, qk_.data(), states, 2, nullptr, nullptr,
                                             &chi2, nullptr, &total));
        return total;
    }
private:
    int model_;
    CpiResult m_;
    Vec3 grav_;
    Vec4 qk_;
    double lin_[6];
};

}  // namespace cpi_host
