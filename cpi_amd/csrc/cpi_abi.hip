// cpi_abi.hip -- the C-ABI of include/cpi_amd.h: argument checks, launch heuristics, device sets (RCCL over xGMI) and the
// host-pointer pipelines.  Host code only; the kernels live in cpi_mean.hip / cpi_cov.hip / cpi_factor.hip and are reached
// through cpi::launch (cpi_args.hpp).
//
// Kernels behind the entries (one 64-lane wavefront per workgroup; all arithmetic f64 VALU, no MFMA -- the contractions
// are 3x3 / sparse 15x15):
//   cpi_mean_kernel<MODEL,JAC,AVG,L>   means (+ analytic bias Jacobians), L lanes per window.  CpiV1.h:67-259 / CpiV2.h:88-305.
//   cpi_mean_tiled_kernel              the same recursion on the tiled input layout (one lane per window, no staging).
//   cpi_cov_kernel<MODEL,AVG>          covariance (model 2: + compounded state transition -> Jacobians) and means;
//                                      column-lane RK4 recursion.  CpiV1.h:266-353 / CpiV2.h:314-464.
//   cpi_forster_kernel                 GTSAM's discrete comparator.  GraphSolver_IMU.cpp:141-232.
//   cpi_factor_kernel<MODEL,WHITEN,LPF,TRI> / cpi_factor_packed_kernel / cpi_factor_hessian_kernel<MODEL,TRI>
//                                      evaluateError residual + Jacobian blocks.  ImuFactorCPIv1.cpp:37-208 / v2.cpp:38-212.
//                                      TRI: the square-root information arrives as its packed upper triangle (ABI 3).
//   cpi_sqrt_info_kernel<PACKED>       R = chol_upper(P^-1) per factor (ImuFactorCPIv1.h:82); PACKED: triangles in and out.
//   cpi_predict_kernel<MODEL>          GraphSolver_IMU.cpp:263-307.
// The covariance / Forster kernels write cpi_outputs.P (dense) and / or P_sym (packed upper triangle, ABI 3).
//   cpi_tile_knots_kernel / cpi_assemble_tiles_kernel   producers of the tiled layout (GraphSolver_IMU.cpp:50-69).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // prototypes and enums only: the library is bound lazily with dlopen (never linked)
#include <dlfcn.h>
#include <stdlib.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cpi_amd.h"
#ifdef CPI_TEST_HOOKS
#include "../../include/cpi_amd_test.h"   // the two test hooks exist in libcpi_amd_test.so only (python -m cpi_amd.build --test-hooks)
#endif
#include "cpi_args.hpp"
#include "cpi_capture_overlap.hpp"

using namespace cpi;

constexpr int kOutFields = 13;   // fields of cpi_outputs (ABI 3: P_sym is the 13th)
static_assert(sizeof(cpi_outputs) == kOutFields * sizeof(double *), "cpi_outputs is a plain table of kOutFields pointers");
static const int OUT_N[kOutFields] = { 1, 3, 3, 4, 9, 9, 9, 9, 9, 9, 9, 225, CPI_TRI_DOUBLES };
static double **out_field(cpi_outputs *o, int k) {
    double **f[kOutFields] = { &o->DT, &o->alpha, &o->beta, &o->q, &o->J_q, &o->J_a, &o->J_b, &o->H_a, &o->H_b, &o->O_a, &o->O_b, &o->P, &o->P_sym };
    return f[k];
}
static double *out_field_c(const cpi_outputs *o, int k) { cpi_outputs t = *o; return *out_field(&t, k); }

// ============================================================================================
// contexts
// ============================================================================================
struct HostPipe;
static void host_pipe_destroy(HostPipe *);
struct cpi_ctx {
    int device;
    hipStream_t stream;
    std::string err;
    // side stream + fork / join events (created at the first use): the two INDEPENDENT kernels of a "model 1, everything"
    // request (covariance kernel; analytic-Jacobian kernel) run concurrently -- see cpi_preintegrate_batch
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    unsigned big_lds_set = 0;   // bit per kernel instantiation whose dynamic-LDS limit was raised on this device
    struct HostPipe *pipe = nullptr;   // staging of the host-pointer entries (created at their first use)
    // Captured single-kernel cpi_preintegrate_batch calls on provably disjoint memory are left unordered in the graph: on
    // overlap_n strands, or (the opt-in look-back shape) up to overlap_n of them at a time; 1 = the serial shape.  The window /
    // the strands are the bookkeeping of the current run of such calls (cpi_capture_overlap.hpp, capture_overlap_begin / _end
    // below); only the one overlap_shape names is ever open.  Parallel branches of a graph need >= 4 hardware queues.
    overlap::Shape overlap_shape = overlap::kShapeLookback;
    int overlap_n = 1;
    bool overlap_allowed = true;
    overlap::Window<hipGraphNode_t> window;
    overlap::Strands<hipGraphNode_t> strands;
    void close_window() { window.close(); strands.close(); }
    std::vector<hipGraphNode_t> ov_found, ov_preds;   // scratch of a call: the stream's dependencies as found; the planned predecessors
};
static thread_local std::string g_create_err;

static int fail(cpi_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg; else g_create_err = msg;
    return code;
}
// Selects the context's device for the duration of a call and restores the caller's current device afterwards.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t enter(int dev) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return e;
        if (prev == dev) return hipSuccess;
        e = hipSetDevice(dev);
        changed = (e == hipSuccess);
        return e;
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};
#define CPI_HIP(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, CPI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)

extern "C" int cpi_abi_version(void) { return CPI_ABI_VERSION; }
#ifndef CPI_BUILD_ID
#define CPI_BUILD_ID "unknown"
#endif
// "cpi-build-id:<id>" as ONE string in .rodata: cpi_amd/_lib.py finds the id of a library file by that tag without loading it
static const char kBuildIdTagged[] = "cpi-build-id:" CPI_BUILD_ID;
extern "C" const char *cpi_build_id(void) { return kBuildIdTagged + 13; }

extern "C" int cpi_ctx_create(int device, void *stream, cpi_ctx **out) {
    if (!out) return fail(nullptr, CPI_ERR_INVALID, "cpi_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, CPI_ERR_NO_DEVICE, "cpi_ctx_create: no HIP device available (this library has no CPU fallback)");
    if (device < 0) {
        e = hipGetDevice(&device);
        if (e != hipSuccess) return fail(nullptr, CPI_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    }
    if (device >= ndev) return fail(nullptr, CPI_ERR_INVALID, "cpi_ctx_create: device index out of range");
    cpi_ctx *c = new cpi_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;
    // the context's capture shape is settled once, here (cpi_capture_overlap.hpp: CapturePolicy); no launch path reads the environment
    const overlap::CapturePolicy pol = overlap::capture_policy_from_environment();
    c->overlap_allowed = pol.allowed;
    c->overlap_shape = pol.shape;
    c->overlap_n = pol.n;
    *out = c;
    return CPI_OK;
}
extern "C" void cpi_ctx_destroy(cpi_ctx *ctx) {
    if (!ctx) return;
    if (ctx->side || ctx->pipe) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(ctx->device);
        if (ctx->side) {
            (void)hipStreamDestroy(ctx->side);
            (void)hipEventDestroy(ctx->ev_fork);
            (void)hipEventDestroy(ctx->ev_join);
        }
        if (ctx->pipe) host_pipe_destroy(ctx->pipe);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    delete ctx;
}
extern "C" int cpi_ctx_set_stream(cpi_ctx *ctx, void *stream) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (ctx->stream != (hipStream_t)stream) ctx->close_window();   // the window describes one stream's capture
    ctx->stream = (hipStream_t)stream;
    return CPI_OK;
}
extern "C" int cpi_ctx_set_capture_overlap(cpi_ctx *ctx, int32_t depth) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    ctx->overlap_shape = overlap::kShapeLookback;
    ctx->overlap_n = ctx->overlap_allowed ? overlap::clamp_depth(depth) : 1;
    ctx->close_window();
    return CPI_OK;
}
extern "C" int cpi_ctx_set_capture_strands(cpi_ctx *ctx, int32_t n) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    ctx->overlap_shape = overlap::kShapeStrands;
    ctx->overlap_n = ctx->overlap_allowed ? overlap::clamp_strands(n) : 1;
    ctx->close_window();
    return CPI_OK;
}
extern "C" const char *cpi_last_error(const cpi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }
extern "C" int cpi_ctx_synchronize(cpi_ctx *ctx) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    CPI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPI_OK;
}

// hipLaunchKernelGGL takes 32-bit grid dimensions: a launch is refused rather than silently truncated
static bool grid_ok(long long nb) { return nb > 0 && nb <= 0x7fffffffLL; }

#ifdef CPI_EXPERIMENTS
// Measurement switches of tools/exp/ (A/B runs of kernel variants).  They exist ONLY in a -DCPI_EXPERIMENTS build
// (python -m cpi_amd.build --experiments -> libcpi_amd_exp.so, loaded through CPI_AMD_LIB); the default library reads no
// environment variable on any launch path.  Each is read once per process.
namespace expsw {
static launch::MeanDmaCfg mean_dma() {   // CPI_AMD_MEAN_DMA = "off" | "KC,S,A" (A = 1: 16-byte aligned pieces)
    static launch::MeanDmaCfg c = [] {
        launch::MeanDmaCfg d = {0, 0, 0};
        const char *e = getenv("CPI_AMD_MEAN_DMA");
        if (e && strcmp(e, "off") != 0) { int k = 0, s = 0, al = 1; if (sscanf(e, "%d,%d,%d", &k, &s, &al) >= 2) d = {k, s, al}; }
        return d;
    }();
    return c;
}
static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
static int mean_blk() { static int v = [] { const char *e = getenv("CPI_AMD_MEAN_BLK"); return e ? (strcmp(e, "off") == 0 ? -1 : atoi(e)) : 0; }(); return v; }
static bool mean_line() { static int v = env_int("CPI_AMD_MEAN_LINE", 0); return v != 0; }   // cpi_mean_line_kernel on the leading groups of a dense one-lane batch
static int blk_mode() { static int v = env_int("CPI_AMD_BLK_MODE", 0); return v; }
static int probe_lds() { static int v = env_int("CPI_AMD_PROBE_LDS", 0); return v; }
static bool no_overlap() { static int v = env_int("CPI_AMD_NO_OVERLAP", 0); return v != 0; }
static bool no_fused_cut() { static int v = env_int("CPI_AMD_NO_FUSED_CUT", 0); return v != 0; }   // A/B: the workspace route for mean-only streams
static int factor_lanes() { static int v = env_int("CPI_AMD_FACTOR_LANES", 0); return (v == 16 || v == 8 || v == 4) ? v : 0; }
static int cost_lanes() { static int v = env_int("CPI_AMD_COST_LANES", 0); return (v == 16 || v == 8 || v == 4) ? v : 0; }
static int packed_lpf() { static int v = env_int("CPI_AMD_PACKED_LPF", 0); return (v == 2 || v == 3 || v == 4 || v == 6 || v == 8) ? v : 0; }
}  // namespace expsw
#endif

// ============================================================================================
// preintegration
// ============================================================================================
static int pick_lanes(const cpi_params *prm, int64_t W, int N, bool jac) {
    // model 2 with analytic Jacobians: sequential per window (the O_a / O_b recursion is not composed); model 2
    // mean-only composes through the gravity response matrices at roughly twice the arithmetic per interval
    if (prm->model == CPI_MODEL_V2 && jac) return 1;
    // (model 2's level cost re-fitted in round 6 on windows of 10 and 20 intervals -- 10 k windows: 4 lanes 8.8 / 10.9 us, the 5 the old
    //  0.6 picked 9.3 / 11.5; the choices at N = 50 do not move.  Model 1's automatic choice is within 0-3 % of the best lane count for
    //  N = 10 / 20 at 5 k ... 50 k windows: profiles/r06_short_windows.md)
    const double t_int = (prm->model == CPI_MODEL_V2) ? 1.2 : 0.55, t_lvl = (prm->model == CPI_MODEL_V2) ? 1.3 : 0.3;
    int L = prm->lanes_per_window;
    if (L <= 0) {
        // Small batches are latency-bound: as long as every wavefront gets a SIMD of its own (<= 1024 wavefronts
        // on MI355X) the launch lasts as long as one wavefront -- intervals per lane plus composition levels
        // (measured: ~0.55 us per interval, ~0.3 us per level).  Splitting further makes wavefronts share SIMDs
        // and loses; batches with more than 1024 single-lane wavefronts are throughput-bound and want L = 1.
        // Measured optima: L = 12 at 5 k windows x 50, 6 at 10 k, 4 at 15 k, 3 at 20 k, 2 at 30 k, 1 from ~60 k.
        double best = 1e300;
        L = 1;
        const int *choices = nullptr;
        const int nc = launch::mean_lane_choices(&choices);
        for (int i = 0; i < nc; i++) {
            const int c = choices[i];
            if (c > 1 && 2 * c > N) break;
            const int64_t waves = (W + (64 / c) - 1) / (64 / c);
            if (c > 1 && waves > 1024) break;
            int levels = 0;
            while ((1 << levels) < c) levels++;
            const double cost = t_int * (double)((N + c - 1) / c) + t_lvl * levels;
            if (cost < best) { best = cost; L = c; }
        }
    }
    return L;
}

#ifdef CPI_EXPERIMENTS
static PreArgs shift_windows(const PreArgs &a, long long w0) {
    PreArgs t = a;
    t.W = a.W - w0;
    if (a.first) t.first = a.first + w0; else t.knots = a.knots + w0 * (long long)(a.N + 1) * 7;
    if (a.count) t.count = a.count + w0;
    t.lin = a.lin + w0 * 6;
    if (a.qk) t.qk = a.qk + w0 * 4;
    for (int k = 0; k < kOutFields; k++) { double **f = out_field(&t.out, k); if (*f) *f += w0 * OUT_N[k]; }
    return t;
}
#endif

// ---- what the preintegration entries share: the request, the kernel argument block, the refusals ---------------------------
// Which groups of fields a cpi_outputs asks for (O_a / O_b count as Jacobians for every model).
struct Request {
    bool mean, jac, cov;
    bool any() const { return mean || jac || cov; }
};
static Request request_of(const cpi_outputs *o) {
    return { o->DT || o->alpha || o->beta || o->q,
             o->J_q || o->J_a || o->J_b || o->H_a || o->H_b || o->O_a || o->O_b,
             o->P != nullptr || o->P_sym != nullptr };
}
static PreArgs pre_args(const cpi_params *prm, int64_t W, int32_t N, const double *knots, const int64_t *first, const int32_t *count,
                        const double *lin, const double *q_k_lin, const cpi_outputs *out) {
    PreArgs a;
    memset(&a, 0, sizeof a);
    a.W = W; a.N = N; a.knots = knots; a.first = (const long long *)first; a.count = count;
    a.lin = lin; a.qk = q_k_lin;
    for (int i = 0; i < 3; i++) a.grav[i] = prm->grav[i];
    a.q4[0] = prm->sigma_w * prm->sigma_w; a.q4[1] = prm->sigma_wb * prm->sigma_wb;
    a.q4[2] = prm->sigma_a * prm->sigma_a; a.q4[3] = prm->sigma_ab * prm->sigma_ab;
    a.out = *out;
    return a;
}

// A refusal is "<entry>: <what>".  The text is put together on the failing path only: a call that succeeds builds no string.
static int refuse(cpi_ctx *ctx, const char *who, const char *what, const char *more = "") {
    return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": " + what + more);
}
#define CPI_TRY(call)                          \
    do {                                       \
        const int rc_ = (call);                \
        if (rc_ != CPI_OK) return rc_;         \
    } while (0)

static bool model_is_cpi(const cpi_params *prm) { return prm->model == CPI_MODEL_V1 || prm->model == CPI_MODEL_V2; }
// what the Forster comparator lacks for an entry that serves models 1 and 2 only
enum { NO_RUNNING_FORM = 1, NOT_RESUMABLE = 2 };
static int refuse_forster(cpi_ctx *ctx, const char *who, int lacks) {
    const std::string why = std::string(lacks & NO_RUNNING_FORM ? "has no running form" : "") + (lacks == (NO_RUNNING_FORM | NOT_RESUMABLE) ? " and " : "") +
                            (lacks & NOT_RESUMABLE ? "cannot be resumed" : "");
    return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": model must be 1 or 2 (the Forster comparator " + why + ")");
}
// model 2 has no running Jacobian rows.  advice: what follows the reason inside its parentheses; NULL: no reason given
static int refuse_v2_jac(cpi_ctx *ctx, const char *who, const char *advice) {
    std::string msg = std::string(who) + ": the Jacobian fields (J_q ... O_b) are not available for model 2";
    if (advice) msg = msg + " (they are read out of the state transition matrix at the end of the recursion" + advice + ")";
    return fail(ctx, CPI_ERR_INVALID, msg);
}
static int check_qk(cpi_ctx *ctx, const char *who, const cpi_params *prm, const void *q_k_lin) {
    return (prm->model == CPI_MODEL_V2 && !q_k_lin) ? refuse(ctx, who, "model 2 needs q_k_lin") : CPI_OK;
}
static int check_N(cpi_ctx *ctx, const char *who, int32_t N) {
    return N > 65535 ? refuse(ctx, who, "N (intervals per window) must be <= 65535") : CPI_OK;
}
// dim: "W" or "U", the entry's name for its number of windows
static int check_grid(cpi_ctx *ctx, const char *who, const char *dim, int64_t n, const char *note = "") {
    return grid_ok(n) ? CPI_OK : fail(ctx, CPI_ERR_INVALID, std::string(who) + ": " + dim + " exceeds 2^31 - 1 windows per call" + note);
}
static int check_lanes(cpi_ctx *ctx, const cpi_params *prm) {
    const int L = prm->lanes_per_window;
    return (L != 0 && !launch::mean_lanes_supported(L)) ? fail(ctx, CPI_ERR_INVALID, "lanes_per_window must be 0 or one of 1,2,3,4,5,6,8,12,16,32,64") : CPI_OK;
}
// what the entries over W windows of <= N intervals refuse alike once their no-op returns are behind them
static int check_windows(cpi_ctx *ctx, const char *who, const cpi_params *prm, int64_t W, int32_t N, const double *knots,
                         const double *lin, const double *q_k_lin) {
    if (!knots || !lin) return refuse(ctx, who, "knots/lin is NULL");
    CPI_TRY(check_qk(ctx, who, prm, q_k_lin));
    CPI_TRY(check_grid(ctx, who, "W", W, " (32-bit grid)"));
    CPI_TRY(check_N(ctx, who, N));
    return check_lanes(ctx, prm);
}
// Carry records.  The kernels of a resume call all read carry_in while they write their parts of carry_out, so the two may
// not overlap; the header of a record's tag names what it was computed with (the records of the two resume entries are
// interchangeable).
static int check_carry_overlap(cpi_ctx *ctx, const char *who, const cpi_params *prm, int64_t W, const double *carry_in, const double *carry_out) {
    const int64_t n = W * (int64_t)carry::doubles(prm->model);
    return (carry_in && carry_in < carry_out + n && carry_out < carry_in + n) ? refuse(ctx, who, "carry_in and carry_out overlap") : CPI_OK;
}
static int carry_header(const cpi_params *prm) {
    const bool stj = prm->model == CPI_MODEL_V2 && prm->state_transition_jacobians != 0;
    return 1 | (prm->imu_avg != 0 ? 8 : 0) | (stj ? 16 : 0) | (32 * prm->model);
}

// Two INDEPENDENT kernels over the same knots (disjoint outputs) share the SIMDs when the second is issued on the context's side
// stream: fork / join by events, so everything later on the context's stream still waits for both, and a stream capture sees an
// ordinary fork.  side_fork returns with ctx->side ordered behind the context's stream; side_join orders the stream behind it.
static int side_fork(cpi_ctx *ctx) {
    if (!ctx->side) {
        CPI_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        CPI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        CPI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    }
    CPI_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    CPI_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    return CPI_OK;
}
static int side_join(cpi_ctx *ctx) {
    CPI_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->side));
    CPI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    return CPI_OK;
}

// cpi_preintegrate_stream: knots = ONE stream of K readings cut at update[W]; the workspace arrays are filled by
// cpi_cut_windows_kernel when a kernel that reads them runs (covariance / Forster / analytic-Jacobian kernels), and stay
// untouched -- except count -- when the mean kernel cuts its own windows (mean-only requests)
struct StreamCut {
    long long K;
    const double *update;
    long long *first;
    int *count;
    double *tstart, *tend;
    const RunArgs *runs;   // cpi_preintegrate_streams: the windows of many runs (NULL: one stream)
};
static int cut_launch(cpi_ctx *ctx, const StreamCut &sc, const double *stream, int64_t U, int32_t N) {
    if (sc.runs) launch::cut_runs(sc.K, stream, (long long)U, sc.update, *sc.runs, sc.first, sc.count, sc.tstart, sc.tend, ctx->stream);
    else launch::cut_windows(sc.K, stream, (long long)U, sc.update, (int)N, sc.first, sc.count, sc.tstart, sc.tend, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
// ---- captured batch calls: independent launches overlap in the graph ----------------------
// While the context's stream is capturing, a cpi_preintegrate_batch call that issues exactly one kernel and touches no
// context-owned memory need not wait for every such call captured before it: on the strand shape it follows the one strand its
// footprint conflicts with (or the least recently extended one), on the look-back shape it skips the up to overlap_n - 1 calls
// right before it whose footprints are disjoint from its own.  capture_overlap_begin replaces the stream's capture
// dependencies by the planned predecessors, the kernel is launched as always, capture_overlap_end reads the new node back and
// leaves the window's frontier on the stream.
// Nothing here can fail a call: any error or surprise of the capture queries puts the dependencies back as found (so the
// launch, and whatever follows, is ordered behind everything before it -- the serial shape) and closes the window.
static void overlap_give_up(cpi_ctx *ctx, bool restore) {
    (void)hipGetLastError();   // a failed query must not surface as the launch's error
    if (restore) {             // Add: whatever the stream depends on by now stays a dependency as well
        (void)hipStreamUpdateCaptureDependencies(ctx->stream, ctx->ov_found.empty() ? nullptr : ctx->ov_found.data(), ctx->ov_found.size(),
                                                 hipStreamAddCaptureDependencies);
        (void)hipGetLastError();
    }
    ctx->close_window();
}
// true: the launch that follows is part of the window and capture_overlap_end must be called after it
template <class Win>   // overlap::Window or overlap::Strands: the context's shape
static bool capture_overlap_begin(cpi_ctx *ctx, Win &win, const overlap::Footprint &fp) {
    if (ctx->overlap_n <= 1 || !ctx->stream) return false;   // the serial shape asks the runtime nothing
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    const hipGraphNode_t *deps = nullptr;
    size_t ndeps = 0;
    if (hipStreamGetCaptureInfo_v2(ctx->stream, &status, &id, nullptr, &deps, &ndeps) != hipSuccess) { overlap_give_up(ctx, false); return false; }
    if (status != hipStreamCaptureStatusActive || (ndeps && !deps)) { win.close(); return false; }
    // several contexts inside one capture: the caller spread the calls by hand, every context keeps the serial shape
    if (!overlap::capture_registry().sole(id, ctx)) { win.close(); return false; }
    ctx->ov_found.assign(deps, deps + ndeps);   // (the runtime's array is valid until the next call on the stream)
    if (!win.continues(id, ctx->ov_found.data(), ndeps)) win.open_at(id, ctx->overlap_n, ctx->ov_found.data(), ndeps);
    win.plan(fp, ctx->ov_preds);
    if (overlap::same_set(ctx->ov_preds, ctx->ov_found.data(), ndeps)) return true;   // (a window's first call; a chain) nothing to change
    if (hipStreamUpdateCaptureDependencies(ctx->stream, ctx->ov_preds.empty() ? nullptr : ctx->ov_preds.data(), ctx->ov_preds.size(),
                                           hipStreamSetCaptureDependencies) != hipSuccess) {
        overlap_give_up(ctx, true);
        return false;
    }
    return true;
}
template <class Win>
static void capture_overlap_end(cpi_ctx *ctx, Win &win, const overlap::Footprint &fp) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    const hipGraphNode_t *deps = nullptr;
    size_t ndeps = 0;
    if (hipStreamGetCaptureInfo_v2(ctx->stream, &status, &id, nullptr, &deps, &ndeps) != hipSuccess ||
        status != hipStreamCaptureStatusActive || ndeps != 1 || !deps) { overlap_give_up(ctx, true); return; }
    const hipGraphNode_t node = deps[0];
    for (hipGraphNode_t p : ctx->ov_preds) if (p == node) { overlap_give_up(ctx, true); return; }   // the launch captured nothing
    win.commit(node, fp);
    const std::vector<hipGraphNode_t> &fr = win.frontier();
    if (fr.size() == 1 && fr[0] == node) return;   // the new node alone: what the stream holds already
    if (hipStreamUpdateCaptureDependencies(ctx->stream, const_cast<hipGraphNode_t *>(fr.data()), fr.size(), hipStreamSetCaptureDependencies) != hipSuccess)
        overlap_give_up(ctx, true);
}

// who: the entry that is called (the batch entry, or a stream entry whose own checks are behind it).  Everything is refused
// before the cut kernel is enqueued: an invalid call must not leave a launch behind that writes the caller's workspace.
static int preintegrate_impl(cpi_ctx *ctx, const char *who, const cpi_params *prm, int64_t W, int32_t N, const double *knots,
                             const int64_t *first, const int32_t *count, const StreamCut *sc, const double *lin,
                             const double *q_k_lin, const cpi_outputs *out) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out) return refuse(ctx, who, "prm/out is NULL");
    if (!model_is_cpi(prm) && prm->model != CPI_MODEL_FORSTER) return refuse(ctx, who, "model must be 1, 2 or 3 (CPI_MODEL_FORSTER)");
    if (W < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (W == 0) return CPI_OK;
    CPI_TRY(check_windows(ctx, who, prm, W, N, knots, lin, q_k_lin));

    const Request rq = request_of(out);
    const bool forster = prm->model == CPI_MODEL_FORSTER;
    const bool avg = prm->imu_avg != 0;
    const bool v2 = prm->model == CPI_MODEL_V2;
    const bool stj = v2 && prm->state_transition_jacobians != 0;
    // Which kernel owns what:
    //   covariance kernel : P, and (model 2 + state_transition_jacobians) the Jacobians read out of
    //                       Discrete_J_b; it also carries the means, so it writes them when it runs.
    //   mean kernel       : means when no covariance kernel runs; the ANALYTIC Jacobians (model 1 always,
    //                       model 2 when state_transition_jacobians == 0).
    const bool run_cov = !forster && (rq.cov || (stj && rq.jac));
    const bool mean_jac = !forster && rq.jac && !stj;
    const bool run_mean = !forster && (mean_jac || (rq.mean && !run_cov));
    // A stream: the mean-only kernel cuts its own windows (fused; it still leaves the TRUE counts in the workspace); every
    // other kernel reads the cut that cpi_cut_windows_kernel leaves there.  Nothing asked for: the counts are still owed.
    // (many runs: the kernel handles runs of any length itself -- the host cannot see them)
    bool fused_cut = sc && rq.any() && run_mean && !mean_jac && !run_cov && (sc->runs != nullptr || sc->K >= 4);
#ifdef CPI_EXPERIMENTS
    if (expsw::no_fused_cut()) fused_cut = false;
#endif

    // One kernel, no context-owned memory: the batch entry's mean-only and mean + analytic-Jacobian requests.  Only those may
    // overlap with their neighbours in a capture; every other route launches as always and ends the window.
    bool overlap_ok = !sc && run_mean && !run_cov;
#ifdef CPI_EXPERIMENTS
    overlap_ok = overlap_ok && expsw::mean_blk() <= 0 && expsw::mean_dma().kc <= 0 && !expsw::mean_line();   // (may issue two kernels)
#endif

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    if (!overlap_ok) ctx->close_window();
    if (sc && !fused_cut) {
        CPI_TRY(cut_launch(ctx, *sc, knots, W, N));
        first = reinterpret_cast<const int64_t *>(sc->first); count = sc->count;
    }
    if (!rq.any()) return CPI_OK;
    PreArgs a = pre_args(prm, W, N, knots, first, count, lin, q_k_lin, out);
    if (sc) { a.K = sc->K; if (!fused_cut) { a.tstart = sc->tstart; a.tend = sc->tend; } }
    if (forster) {   // one kernel owns everything; imu_avg, q_k_lin, grav play no part
        launch::forster(a, ctx->stream);
        CPI_HIP(ctx, hipGetLastError());
        return CPI_OK;
    }

    // Model 1 with Jacobians AND covariance is two independent kernels (side_fork).  The covariance kernel waits on the LDS pipe
    // about as much as it issues VALU work and uses no more than two wavefronts per SIMD; the Jacobian kernel is pure FP64 VALU
    // with no LDS.
    bool forked = run_cov && run_mean && mean_jac;
#ifdef CPI_EXPERIMENTS
    forked = forked && !expsw::no_overlap();
#endif
    if (forked) CPI_TRY(side_fork(ctx));
    const hipStream_t mean_stream = forked ? ctx->side : ctx->stream;
    if (run_cov) {
        PreArgs c = a;
        c.write_means = rq.mean ? 1 : 0;
        c.write_jac = (stj && rq.jac) ? 1 : 0;
        launch::cov(prm->model, avg, c, ctx->stream);
    }
    if (run_mean) {
        PreArgs m = a;
        m.write_means = (rq.mean && !run_cov) ? 1 : 0;
        m.write_jac = mean_jac ? 1 : 0;
        if (fused_cut) { m.update = sc->update; m.count_out = sc->count; m.first = nullptr; m.count = nullptr; }
        const int LL = pick_lanes(prm, W, N, mean_jac);
        long long done = 0;
#ifdef CPI_EXPERIMENTS
        const int bl = expsw::mean_blk();
        m.dbg = expsw::blk_mode();
        // (both experimental kernels address `knots` as the dense [W][N + 1][7] layout: never on a stream call, whose outer
        //  first / count are NULL on the fused-cut route although the windows are anything but dense)
        if (!sc && !mean_jac && !first && bl > 0 && (size_t)(64 / bl) * (size_t)(N + 1) * 56 <= 65536 && N >= 1) {
            if (launch::mean_blk(prm->model, bl, avg, m, ctx->stream)) done = W;
        }
        const launch::MeanDmaCfg dc = expsw::mean_dma();
        if (!sc && !done && !mean_jac && LL == 1 && !first && !count && dc.kc > 0 && N >= 2 * dc.kc)
            done = launch::mean_dma(prm->model, dc, avg, m, ctx->stream);
        if (!sc && !done && !mean_jac && LL == 1 && !first && !count && expsw::mean_line()) done = launch::mean_line(prm->model, avg, m, ctx->stream);
        if (done && done < W) m = shift_windows(m, done);
#endif
        if (done < W) {
            if (fused_cut && sc->runs) launch::mean_runs(prm->model, avg, LL, m, *sc->runs, mean_stream);
            else if (overlap_ok && ctx->overlap_n > 1 && !overlap::launch_is_latency_bound((W + (64 / LL) - 1) / (64 / LL))) {
                ctx->close_window();   // a launch that fills the SIMDs several times over has no idle head and tail to hide
                launch::mean(prm->model, mean_jac, avg, LL, m, mean_stream);
            } else if (overlap_ok && ctx->overlap_n > 1) {
                const void *outs[kOutFields];
                for (int k = 0; k < kOutFields; k++) outs[k] = out_field_c(out, k);
                const overlap::Footprint fp = overlap::make_footprint(W, N, knots, first, count, lin, q_k_lin, outs, OUT_N, kOutFields);
                const bool strands = ctx->overlap_shape == overlap::kShapeStrands;
                const bool in_window = strands ? capture_overlap_begin(ctx, ctx->strands, fp) : capture_overlap_begin(ctx, ctx->window, fp);
                launch::mean(prm->model, mean_jac, avg, LL, m, mean_stream);
                const hipError_t launched = hipGetLastError();   // taken before the capture queries, which clear their own errors
                if (in_window) { if (strands) capture_overlap_end(ctx, ctx->strands, fp); else capture_overlap_end(ctx, ctx->window, fp); }
                CPI_HIP(ctx, launched);
            } else launch::mean(prm->model, mean_jac, avg, LL, m, mean_stream);
        }
    }
    if (forked) CPI_TRY(side_join(ctx));
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_preintegrate_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                      const double *knots, const int64_t *first, const int32_t *count,
                                      const double *lin, const double *q_k_lin, const cpi_outputs *out) {
    return preintegrate_impl(ctx, "cpi_preintegrate_batch", prm, W, N, knots, first, count, nullptr, lin, q_k_lin, out);
}

// Resumable preintegration: cpi_preintegrate_batch from and to carry records (include/cpi_amd.h).  The same ownership rules
// and lane choice as the batch entry, except that the means are always computed (into carry_out); the kernels are the
// CARRY instantiations of the batch kernels (cpi_mean_carry_kernel / cpi_cov_carry_kernel), so a NULL carry_in reproduces
// the batch call bit for bit.
extern "C" size_t cpi_carry_doubles(int32_t model) { return (model == CPI_MODEL_V1 || model == CPI_MODEL_V2) ? (size_t)carry::doubles(model) : 0; }
extern "C" int cpi_preintegrate_resume(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                       const double *knots, const int64_t *first, const int32_t *count,
                                       const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                                       const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_resume";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out) return refuse(ctx, who, "prm/out is NULL");
    if (!model_is_cpi(prm)) return refuse_forster(ctx, who, NOT_RESUMABLE);
    if (!carry_out) return refuse(ctx, who, "carry_out is NULL");
    if (W < 0 || N < 0) return refuse(ctx, who, "negative size");
    CPI_TRY(check_carry_overlap(ctx, who, prm, W, carry_in, carry_out));
    if (W == 0) return CPI_OK;
    CPI_TRY(check_windows(ctx, who, prm, W, N, knots, lin, q_k_lin));

    const Request rq = request_of(out);
    const bool avg = prm->imu_avg != 0;
    const bool stj = prm->model == CPI_MODEL_V2 && prm->state_transition_jacobians != 0;
    // ownership as in preintegrate_impl; the means always run (carry_out holds them even when out asks for none)
    const bool run_cov = rq.cov || (stj && rq.jac);
    const bool mean_jac = rq.jac && !stj;
    const bool run_mean = mean_jac || !run_cov;
    CarryArgs c;
    c.in = carry_in;
    c.out = carry_out;
    c.need = carry_header(prm) | (run_cov ? carry::TAG_P : 0) | (mean_jac ? carry::TAG_J : 0);
    c.tag_out = c.need;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    const PreArgs a = pre_args(prm, W, N, knots, first, count, lin, q_k_lin, out);
    // model 1 with Jacobians and covariance: the two kernels overlap on the side stream as in the batch entry.  They write
    // disjoint parts of carry_out and both only read carry_in (which is why the two may not overlap).
    const bool forked = run_cov && run_mean;
    if (forked) CPI_TRY(side_fork(ctx));
    if (run_cov) {
        PreArgs p = a;
        p.write_means = rq.mean ? 1 : 0;
        p.write_jac = (stj && rq.jac) ? 1 : 0;
        CarryArgs cc = c;
        cc.own_means = 1;
        launch::cov_carry(prm->model, avg, p, cc, ctx->stream);
    }
    if (run_mean) {
        PreArgs m = a;
        m.write_means = (rq.mean && !run_cov) ? 1 : 0;
        m.write_jac = mean_jac ? 1 : 0;
        CarryArgs cm = c;
        cm.own_means = run_cov ? 0 : 1;
        launch::mean_carry(prm->model, mean_jac, avg, pick_lanes(prm, W, N, mean_jac), m, cm, forked ? ctx->side : ctx->stream);
    }
    if (forked) CPI_TRY(side_join(ctx));
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// Running preintegration: the measurement after EVERY interval (include/cpi_amd.h).  rows holds W * N rows; the means and the
// model-1 analytic Jacobians come from cpi_mean_running_kernel (the batch entry's lane choice, pick_lanes), the covariance rows
// from cpi_cov_running_kernel.  The kernels run one after the other on the context's stream (no side stream: a capture of the
// call is a chain), and unlike the batch entry the covariance kernel leaves the means to the mean kernel -- its own means
// advance once per staged pass, not per interval.
// cpi_preintegrate_running and cpi_running_stj_batch (with_stj) are one body.  The latter serves the Jacobian fields of model 2
// with state_transition_jacobians != 0 as well: cpi_cov_running_stj_kernel takes the place of cpi_cov_running_kernel (it runs even when
// P / P_sym are not asked for: the transition columns ride on the covariance recursion) and the mean kernel is launched exactly as
// for the same request without the Jacobian fields, so the mean and P rows are bit for bit those of cpi_preintegrate_running.
static const char kNoAnalyticRunning[] = "the Jacobian fields (J_q ... O_b) of model 2 need state_transition_jacobians != 0 here: the analytic O_a / O_b "
                                         "recursion has no running form (the rows are read out of the state transition matrix)";
static int refuse_v2_jac_here(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, const char *advice) {
    if (with_stj) return prm->state_transition_jacobians != 0 ? CPI_OK : refuse(ctx, who, kNoAnalyticRunning);
    return refuse_v2_jac(ctx, who, advice);
}
static int running_device(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, int64_t W, int32_t N,
                          const double *knots, const int64_t *first, const int32_t *count,
                          const double *lin, const double *q_k_lin, const cpi_outputs *rows) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows) return refuse(ctx, who, "prm/rows is NULL");
    if (prm->model == CPI_MODEL_FORSTER) return refuse_forster(ctx, who, NO_RUNNING_FORM);
    if (!model_is_cpi(prm)) return refuse(ctx, who, "model must be 1 or 2");
    const Request rq = request_of(rows);
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;   // (past the refusal below: the rows of the transition columns)
    if (stj) CPI_TRY(refuse_v2_jac_here(ctx, who, with_stj, prm, ""));
    if (W < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (W == 0 || N == 0) return CPI_OK;
    CPI_TRY(check_windows(ctx, who, prm, W, N, knots, lin, q_k_lin));
    if (!rq.any()) return CPI_OK;
    const bool avg = prm->imu_avg != 0;
    const bool mean_jac = rq.jac && !stj;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    const PreArgs a = pre_args(prm, W, N, knots, first, count, lin, q_k_lin, rows);
    if (rq.mean || mean_jac) {
        PreArgs m = a;
        m.write_means = rq.mean ? 1 : 0;
        m.write_jac = mean_jac ? 1 : 0;
        launch::mean_running(prm->model, mean_jac, avg, pick_lanes(prm, W, N, mean_jac), m, ctx->stream);
    }
    if (stj) launch::cov_running_stj(avg, a, ctx->stream);
    else if (rq.cov) launch::cov_running(prm->model, avg, a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_preintegrate_running(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                        const double *knots, const int64_t *first, const int32_t *count,
                                        const double *lin, const double *q_k_lin, const cpi_outputs *rows) {
    return running_device(ctx, "cpi_preintegrate_running", false, prm, W, N, knots, first, count, lin, q_k_lin, rows);
}
extern "C" int cpi_running_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                     const double *knots, const int64_t *first, const int32_t *count,
                                     const double *lin, const double *q_k_lin, const cpi_outputs *rows) {
    return running_device(ctx, "cpi_running_stj_batch", true, prm, W, N, knots, first, count, lin, q_k_lin, rows);
}

// Running preintegration from and to carry records (include/cpi_amd.h): the argument rules of cpi_preintegrate_running and the
// record / tag rules of cpi_preintegrate_resume.  cpi_mean_running_carry_kernel ALWAYS runs -- it owns the tag, the means and
// the model-1 Jacobian block of carry_out, whatever rows asks for --, cpi_cov_running_carry_kernel adds the P / P_sym rows and
// the covariance block.  Both read carry_in and write disjoint parts of carry_out, one after the other on the context's
// stream: no side stream (a capture of the call is a chain), and still no in-place records.
// cpi_preintegrate_running_resume and cpi_running_resume_stj_batch (with_stj) are one body, as running_device is.  The latter serves
// the Jacobian fields of model 2 with state_transition_jacobians != 0: cpi_cov_running_stj_carry_kernel takes the place of
// cpi_cov_running_carry_kernel (it runs even when P / P_sym are not asked for, and the call then needs and leaves the covariance
// state), and the mean kernel is launched exactly as for the same request without the Jacobian fields.
static int running_resume_device(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, int64_t W, int32_t N,
                                 const double *knots, const int64_t *first, const int32_t *count,
                                 const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                                 const cpi_outputs *rows) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows) return refuse(ctx, who, "prm/rows is NULL");
    if (prm->model == CPI_MODEL_FORSTER) return refuse_forster(ctx, who, NO_RUNNING_FORM | NOT_RESUMABLE);
    if (!model_is_cpi(prm)) return refuse(ctx, who, "model must be 1 or 2");
    const Request rq = request_of(rows);
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;   // (past the refusal below: the rows of the transition columns)
    if (stj) CPI_TRY(refuse_v2_jac_here(ctx, who, with_stj, prm, ": finish the chain with cpi_preintegrate_resume"));
    const bool mean_jac = rq.jac && !stj;
    if (!carry_out) return refuse(ctx, who, "carry_out is NULL");
    if (W < 0 || N < 0) return refuse(ctx, who, "negative size");
    CPI_TRY(check_carry_overlap(ctx, who, prm, W, carry_in, carry_out));
    if (W == 0) return CPI_OK;
    CPI_TRY(check_windows(ctx, who, prm, W, N, knots, lin, q_k_lin));
    const bool avg = prm->imu_avg != 0;
    CarryArgs c;
    c.in = carry_in;
    c.out = carry_out;
    c.need = carry_header(prm) | ((rq.cov || stj) ? carry::TAG_P : 0) | (mean_jac ? carry::TAG_J : 0);
    c.tag_out = c.need;
    c.own_means = 0;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    const PreArgs a = pre_args(prm, W, N, knots, first, count, lin, q_k_lin, rows);
    {
        PreArgs m = a;
        m.write_means = rq.mean ? 1 : 0;
        m.write_jac = mean_jac ? 1 : 0;
        CarryArgs cm = c;
        cm.own_means = 1;
        launch::mean_running_carry(prm->model, mean_jac, avg, pick_lanes(prm, W, N, mean_jac), m, cm, ctx->stream);
    }
    if (stj) launch::cov_running_carry_stj(avg, a, c, ctx->stream);
    else if (rq.cov) launch::cov_running_carry(prm->model, avg, a, c, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_preintegrate_running_resume(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                               const double *knots, const int64_t *first, const int32_t *count,
                                               const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                                               const cpi_outputs *rows) {
    return running_resume_device(ctx, "cpi_preintegrate_running_resume", false, prm, W, N, knots, first, count, lin, q_k_lin, carry_in, carry_out, rows);
}
extern "C" int cpi_running_resume_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                            const double *knots, const int64_t *first, const int32_t *count,
                                            const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                                            const cpi_outputs *rows) {
    return running_resume_device(ctx, "cpi_running_resume_stj_batch", true, prm, W, N, knots, first, count, lin, q_k_lin, carry_in, carry_out, rows);
}

// The measurement at arbitrary times inside a window (include/cpi_amd.h): one kernel, one lane per query, over the rows
// cpi_preintegrate_running wrote for the same windows.  Nothing here looks at device memory, so the call can be captured.
// cpi_query_batch and cpi_query_cov_batch are one body: the latter also accepts P / P_sym in out (with_cov) and then enqueues
// cpi_query_cov_kernel behind the mean kernel, on the same stream.
static const char kQueryNoCov[] = "P / P_sym are not available at query times (they need the covariance kernel's lane-spread RK4 step)";
// what an entry of the query family serves beyond the means and the model-1 Jacobians
enum { QUERY_COV = 1, QUERY_STJ = 2 };
static int query_check(cpi_ctx *ctx, const char *who, const cpi_params *prm, const Request &rq, int with) {
    if (prm->model == CPI_MODEL_FORSTER) return refuse(ctx, who, "model must be 1 or 2 (the Forster comparator has no running form)");
    if (!model_is_cpi(prm)) return refuse(ctx, who, "model must be 1 or 2");
    if (rq.cov && !(with & QUERY_COV)) return refuse(ctx, who, kQueryNoCov);
    if (prm->model == CPI_MODEL_V2 && rq.jac) return refuse_v2_jac_here(ctx, who, (with & QUERY_STJ) != 0, prm, "");
    return CPI_OK;
}
static int query_trips(int32_t N) {
    int trips = 0;
    while ((1ll << trips) < (long long)N + 1) trips++;
    return trips;
}
// the checks the device and the host form share, up to the ones on rows (the host form computes its own rows); *done: a no-op call
static int query_check_args(cpi_ctx *ctx, const char *who, int with, const cpi_params *prm, int64_t W, int32_t N, const double *knots,
                            const double *lin, const double *q_k_lin, int64_t Q, const int32_t *qwin, const double *qtime,
                            const cpi_outputs *out, bool *done) {
    *done = true;
    CPI_TRY(query_check(ctx, who, prm, request_of(out), with));
    if (W < 0 || N < 0 || Q < 0) return refuse(ctx, who, "negative size");
    if (Q == 0) return CPI_OK;
    if (W == 0) return refuse(ctx, who, "W is 0: there is no window to query");
    if (!qwin || !qtime) return refuse(ctx, who, "qwin/qtime is NULL");
    CPI_TRY(check_windows(ctx, who, prm, W, N, knots, lin, q_k_lin));
    if (!grid_ok(Q)) return refuse(ctx, who, "Q exceeds 2^31 - 1 queries per call (32-bit grid)");
    *done = false;
    return CPI_OK;
}
// what rows must hold (N > 0) for the request of out: shared by the query entries
// (what: "rows", or "base" for the base row of cpi_query_open_batch, which must hold the same)
static int query_rows_check(cpi_ctx *ctx, const char *who, const cpi_params *prm, const cpi_outputs *rows, const cpi_outputs *out,
                            const char *what = "rows") {
    const std::string R = what;
    const Request rq = request_of(out);
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;
    const bool means = rq.mean || (rq.jac && !stj);
    if (stj) {   // the transition columns are rebuilt from ALL seven fields of a row, whatever subset out asks for
        std::string lacks;
        const struct { const char *name; const double *p; } need[] = { {"q", rows->q}, {"J_q", rows->J_q}, {"J_a", rows->J_a}, {"J_b", rows->J_b},
                                                                       {"H_a", rows->H_a}, {"H_b", rows->H_b}, {"O_a", rows->O_a}, {"O_b", rows->O_b} };
        for (const auto &f : need) if (!f.p) lacks += std::string(lacks.empty() ? "" : ", ") + f.name;
        if (!lacks.empty()) return refuse(ctx, who, (R + " needs q and all seven Jacobian fields for the model-2 Jacobians; missing: ").c_str(), lacks.c_str());
    }
    if (means || !(rq.cov || stj)) {
        if (!rows->DT || !rows->alpha || !rows->beta || !rows->q) return refuse(ctx, who, (R + " needs DT, alpha, beta and q").c_str());
        if (!stj && ((out->J_q && !rows->J_q) || (out->J_a && !rows->J_a) || (out->J_b && !rows->J_b) || (out->H_a && !rows->H_a) || (out->H_b && !rows->H_b)))
            return refuse(ctx, who, ("a Jacobian field of out needs the same field of " + R).c_str());
    }
    if (rq.cov) {
        if (!rows->q) return refuse(ctx, who, (R + " needs q (the rotation at the start of the partial interval)").c_str());
        if (!rows->P && !rows->P_sym) return refuse(ctx, who, (R + " needs P or P_sym when out asks for P / P_sym").c_str());
    }
    return CPI_OK;
}
static int query_device(cpi_ctx *ctx, const char *who, int with, const cpi_params *prm, int64_t W, int32_t N,
                        const double *knots, const int64_t *first, const int32_t *count,
                        const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                        int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out,
                        const cpi_outputs *base = nullptr, int32_t base_N = 0) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows || !out) return refuse(ctx, who, "prm/rows/out is NULL");
    if (base && base_N < 1) return refuse(ctx, who, "base_N must be >= 1 when base is given");
    const Request rq = request_of(out);
    bool done;
    CPI_TRY(query_check_args(ctx, who, with, prm, W, N, knots, lin, q_k_lin, Q, qwin, qtime, out, &done));
    if (done) return CPI_OK;
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;   // (cpi_query_stj_batch: query_check has refused it for the others)
    const bool mean_jac = rq.jac && !stj;
    const bool means = rq.mean || mean_jac;
    if (N > 0) CPI_TRY(query_rows_check(ctx, who, prm, rows, out));   // N == 0: every query is the zero state and rows is not read
    if (base) CPI_TRY(query_rows_check(ctx, who, prm, base, out, "base"));
    if (!rq.any()) return CPI_OK;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    QueryArgs a;
    memset(&a, 0, sizeof a);
    a.W = W; a.N = N; a.knots = knots; a.first = (const long long *)first; a.count = count; a.lin = lin; a.qk = q_k_lin;
    for (int i = 0; i < 3; i++) a.grav[i] = prm->grav[i];
    a.rows = *rows; a.Q = Q; a.qwin = qwin; a.qtime = qtime; a.trips = query_trips(N); a.out = *out;
    // the Jacobian instance carries all five matrices: the ones out does not ask for are read from a field that is there
    auto fill_jac = [](cpi_outputs &r) {
        const double *any = r.J_q ? r.J_q : r.J_a ? r.J_a : r.J_b ? r.J_b : r.H_a ? r.H_a : r.H_b;
        double **f[5] = { &r.J_q, &r.J_a, &r.J_b, &r.H_a, &r.H_b };
        for (double **x : f) if (!*x) *x = const_cast<double *>(any);
    };
    if (mean_jac) fill_jac(a.rows);
    const double q4[4] = { prm->sigma_w * prm->sigma_w, prm->sigma_wb * prm->sigma_wb, prm->sigma_a * prm->sigma_a, prm->sigma_ab * prm->sigma_ab };
    if (base) {   // cpi_query_open_batch: the same three kernels with the base row where the zero state stood, on the same stream
        QueryBase b;
        b.rows = *base;
        b.N = base_N;
        if (mean_jac) fill_jac(b.rows);
        if (means) launch::query_open(prm->model, mean_jac, prm->imu_avg != 0, a, b, ctx->stream);
        if (stj) launch::query_stj_open(prm->imu_avg != 0, a, b, ctx->stream);
        if (rq.cov) launch::query_cov_open(prm->model, prm->imu_avg != 0, a, q4, b, ctx->stream);
        CPI_HIP(ctx, hipGetLastError());
        return CPI_OK;
    }
    if (means) launch::query(prm->model, mean_jac, prm->imu_avg != 0, a, ctx->stream);
    if (stj) launch::query_stj(prm->imu_avg != 0, a, ctx->stream);
    if (rq.cov) launch::query_cov(prm->model, prm->imu_avg != 0, a, q4, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_query_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                               const double *knots, const int64_t *first, const int32_t *count,
                               const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                               int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    return query_device(ctx, "cpi_query_batch", 0, prm, W, N, knots, first, count, lin, q_k_lin, rows, Q, qwin, qtime, out);
}
extern "C" int cpi_query_cov_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                   const double *knots, const int64_t *first, const int32_t *count,
                                   const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                                   int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    return query_device(ctx, "cpi_query_cov_batch", QUERY_COV, prm, W, N, knots, first, count, lin, q_k_lin, rows, Q, qwin, qtime, out);
}
// cpi_query_cov_batch + the Jacobians of model 2 (state_transition_jacobians != 0): cpi_query_stj_kernel, on the same stream
extern "C" int cpi_query_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                   const double *knots, const int64_t *first, const int32_t *count,
                                   const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                                   int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    return query_device(ctx, "cpi_query_stj_batch", QUERY_COV | QUERY_STJ, prm, W, N, knots, first, count, lin, q_k_lin, rows, Q, qwin, qtime, out);
}
// cpi_query_stj_batch for windows that continue from a carried state: base (row w * base_N + base_N - 1) stands where the zero state
// stood.  base == NULL: cpi_query_stj_batch itself.
extern "C" int cpi_query_open_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                    const double *knots, const int64_t *first, const int32_t *count,
                                    const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                                    int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out,
                                    const cpi_outputs *base, int32_t base_N) {
    return query_device(ctx, "cpi_query_open_batch", QUERY_COV | QUERY_STJ, prm, W, N, knots, first, count, lin, q_k_lin, rows, Q, qwin, qtime, out,
                        base, base_N);
}

// cpi_merge_batch: consecutive preintegrated windows joined into one measurement (cpi_merge_kernel, cpi_merge.hip).  Everything
// the call can refuse is refused BEFORE the context is looked at, so the contract can be exercised where no device exists
// (cpi_last_error(NULL) holds the text then).
static int merge_check(cpi_ctx *ctx, const char *who, int32_t model, int64_t M, int32_t G, int64_t in_rows, const cpi_outputs *in,
                       const cpi_outputs *out, Request *rq) {
    if (!in || !out) return refuse(ctx, who, "in/out is NULL");
    if (model != CPI_MODEL_V1)
        return refuse(ctx, who, "model must be 1 (model 2 is not composable from its outputs: alpha and beta carry gravity through each "
                                "window's own q_k_lin; the Forster comparator's covariance does not come from this recursion)");
    if (G < 1) return refuse(ctx, who, "G (the largest group) must be >= 1");
    if (M < 0 || in_rows < 0) return refuse(ctx, who, "negative size");
    if (out->O_a || out->O_b) return refuse(ctx, who, "O_a / O_b are model-2 fields: not available");
    *rq = request_of(out);
    if (in_rows > 0 && rq->any()) {
        if (!in->DT || !in->alpha || !in->beta || !in->q) return refuse(ctx, who, "in must hold DT, alpha, beta and q");
        if ((rq->jac || rq->cov) && (!in->J_q || !in->J_a || !in->J_b || !in->H_a || !in->H_b))
            return refuse(ctx, who, "in must hold all five Jacobians (J_q J_a J_b H_a H_b) when out asks for a Jacobian or for P / P_sym");
        if (rq->cov && !in->P && !in->P_sym) return refuse(ctx, who, "in must hold P or P_sym when out asks for P / P_sym");
    }
    for (int a = 0; a < kOutFields; a++)
        for (int b = 0; b < kOutFields; b++) {
            const double *pi = out_field_c(in, a), *po = out_field_c(out, b);
            if (pi && po && pi < po + M * OUT_N[b] && po < pi + in_rows * OUT_N[a]) return refuse(ctx, who, "an array of out overlaps an array of in");
        }
    return CPI_OK;
}
extern "C" int cpi_merge_batch(cpi_ctx *ctx, int32_t model, int64_t M, int32_t G, int64_t in_rows, const cpi_outputs *in,
                               const int64_t *first, const int32_t *count, const cpi_outputs *out) {
    static const char who[] = "cpi_merge_batch";
    Request rq;
    CPI_TRY(merge_check(ctx, who, model, M, G, in_rows, in, out, &rq));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (M == 0 || !rq.any()) return CPI_OK;
    if (!grid_ok((M + 3) / 4)) return refuse(ctx, who, "M exceeds the 32-bit grid (4 output rows per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    MergeArgs a;
    memset(&a, 0, sizeof a);
    a.M = M; a.G = G; a.in_rows = in_rows; a.in = *in; a.first = (const long long *)first; a.count = count; a.out = *out;
    launch::merge(rq.jac, rq.cov, a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// Replaces the caller-side loop of GraphSolver::createimufactor_cpi_v1 / _v2 (GraphSolver_IMU.cpp:43-75, 97-130) for ALL the
// windows of a trajectory at once, with ZERO copies of the IMU data: cpi_cut_windows_kernel finds, per update time, where the
// reference's deque would stand (28 bytes per window into the caller's workspace), and the preintegration kernels read the
// stream in place, patching the first knot's stamp and building a partial tail interval from its predecessor in flight.
static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
extern "C" size_t cpi_stream_workspace_bytes(int64_t U) {
    if (U <= 0) return 16;
    return align16((size_t)U * 8) * 3 + align16((size_t)U * 4);
}
extern "C" const int32_t *cpi_stream_counts(const void *workspace, int64_t U) {
    if (!workspace || U <= 0) return nullptr;
    return reinterpret_cast<const int32_t *>(static_cast<const char *>(workspace) + align16((size_t)U * 8) * 3);
}
// the workspace layout shared by the stream entries: first[U] (8 B), tstart[U], tend[U], count[U] (4 B), each 16-byte aligned
static StreamCut stream_cut(int64_t K, const double *update_times, void *workspace, int64_t U, const RunArgs *runs) {
    StreamCut sc;
    char *ws = static_cast<char *>(workspace);
    sc.K = (long long)K; sc.update = update_times;
    sc.first = reinterpret_cast<long long *>(ws);
    sc.tstart = reinterpret_cast<double *>(ws + align16((size_t)U * 8));
    sc.tend = reinterpret_cast<double *>(ws + 2 * align16((size_t)U * 8));
    sc.count = reinterpret_cast<int *>(ws + 3 * align16((size_t)U * 8));
    sc.runs = runs;
    return sc;
}
static int check_workspace(cpi_ctx *ctx, const char *who, const void *workspace) {
    return ((uintptr_t)workspace & 15) != 0 ? refuse(ctx, who, "the workspace must be 16-byte aligned") : CPI_OK;
}
extern "C" int cpi_preintegrate_stream(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                       const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                       void *workspace, const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_stream";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (K < 0 || U < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (U == 0) return CPI_OK;
    if (K == 0) return refuse(ctx, who, "the stream is empty");
    if (!stream || !update_times || !workspace) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_workspace(ctx, who, workspace));
    CPI_TRY(check_grid(ctx, who, "U", U));
    if (!prm || !out || !lin) return refuse(ctx, who, "prm/out/lin is NULL");
    const StreamCut sc = stream_cut(K, update_times, workspace, U, nullptr);
    return preintegrate_impl(ctx, who, prm, U, N, stream, nullptr, nullptr, &sc, lin, q_k_lin, out);
}

// Many IMU streams in one call: run r owns the knots [stream_offsets[r], stream_offsets[r + 1]) and the windows
// [update_offsets[r], update_offsets[r + 1]).  The offsets are device data: the kernels clamp them (cpi_mean_kernels.hpp:
// run_of / run_window), the _host entry validates them.  The workspace is the single-stream entry's, so cpi_stream_counts
// reads the counts of a multi-run call too.
extern "C" size_t cpi_streams_workspace_bytes(int64_t R, int64_t U) {
    (void)R;   // the layout depends on U alone: the run lookup needs no per-window record (it is redone in every prologue)
    return cpi_stream_workspace_bytes(U);
}
extern "C" int cpi_preintegrate_streams(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                        const int64_t *stream_offsets, int64_t U, const double *update_times,
                                        const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                        void *workspace, const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_streams";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (R < 0 || K < 0 || U < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (U == 0) return CPI_OK;
    if (R == 0) return refuse(ctx, who, "U > 0 windows and no run");
    if (R > 0x7ffffffeLL) return refuse(ctx, who, "R exceeds 2^31 - 2 runs");
    if (K == 0) return refuse(ctx, who, "the streams hold no reading");
    if (!stream || !stream_offsets || !update_times || !update_offsets || !workspace) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_workspace(ctx, who, workspace));
    CPI_TRY(check_grid(ctx, who, "U", U));
    if (!prm || !out || !lin) return refuse(ctx, who, "prm/out/lin is NULL");
    RunArgs ra;
    ra.soff = reinterpret_cast<const long long *>(stream_offsets);
    ra.uoff = reinterpret_cast<const long long *>(update_offsets);
    ra.R = (int)R;
    const StreamCut sc = stream_cut(K, update_times, workspace, U, &ra);
    return preintegrate_impl(ctx, who, prm, U, N, stream, nullptr, nullptr, &sc, lin, q_k_lin, out);
}

// Running rows from the stream entries (include/cpi_amd.h: cpi_preintegrate_stream_running / cpi_preintegrate_streams_running): the
// cut kernel of cpi_preintegrate_stream[s] always runs, then cpi_mean_stream_running_kernel (means, model-1 Jacobians) and
// cpi_cov_running_kernel (whose phase A reads cut windows when PreArgs::tstart is set) read the stream in place -- one after the
// other on the context's stream, as in cpi_preintegrate_running.  The lane choice is pick_lanes(U, N, request), the function
// cpi_preintegrate_running uses: the rows are bit for bit those of that entry on the host-assembled windows.
// with_stj: cpi_stream_running_stj_batch, which serves model 2's Jacobian rows as cpi_running_stj_batch does (cpi_cov_running_stj_kernel
// sits on cov_body, whose phase A reads cut windows: the same launch with tstart / tend set).
static int stream_running_check(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, bool many, int64_t R, int64_t K, int64_t U,
                                int32_t N, const void *stream, const void *soff, const void *update_times, const void *uoff,
                                const void *lin, const void *q_k_lin, const cpi_outputs *rows, bool &noop) {
    noop = false;
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows) return refuse(ctx, who, "prm/rows is NULL");
    if (prm->model == CPI_MODEL_FORSTER) return refuse_forster(ctx, who, NO_RUNNING_FORM);
    if (!model_is_cpi(prm)) return refuse(ctx, who, "model must be 1 or 2");
    if (prm->model == CPI_MODEL_V2 && request_of(rows).jac) CPI_TRY(refuse_v2_jac_here(ctx, who, with_stj, prm, ""));
    if (R < 0 || K < 0 || U < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (U == 0 || N == 0) { noop = true; return CPI_OK; }
    if (many && R == 0) return refuse(ctx, who, "U > 0 windows and no run");
    if (many && R > 0x7ffffffeLL) return refuse(ctx, who, "R exceeds 2^31 - 2 runs");
    if (K == 0) return refuse(ctx, who, many ? "the streams hold no reading" : "the stream is empty");
    if (!stream || !update_times || !lin || (many && (!soff || !uoff))) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_grid(ctx, who, "U", U));
    CPI_TRY(check_qk(ctx, who, prm, q_k_lin));
    CPI_TRY(check_N(ctx, who, N));
    return check_lanes(ctx, prm);
}
// the running kernels on the windows [w0, w0 + wn) of a cut that is already in the workspace; rows: row 0 = window w0, interval 0.
// L: the lane choice of the WHOLE call (a chunked download must not change it)
static int stream_running_launch(cpi_ctx *ctx, const cpi_params *prm, const StreamCut &sc, const double *stream, int32_t N, int L,
                                 const double *lin, const double *q_k_lin, const cpi_outputs *rows, int64_t w0, int64_t wn) {
    const Request rq = request_of(rows);
    const bool avg = prm->imu_avg != 0;
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;   // (cpi_stream_running_stj_batch: the check has refused it for the others)
    const bool mean_jac = rq.jac && !stj;
    PreArgs a = pre_args(prm, wn, N, stream, reinterpret_cast<const int64_t *>(sc.first), sc.count, lin, q_k_lin, rows);
    a.K = sc.K; a.tstart = sc.tstart + w0; a.tend = sc.tend + w0;
    a.first += w0; a.count += w0; a.lin += w0 * 6;
    if (a.qk) a.qk += w0 * 4;
    if (rq.mean || mean_jac) {
        PreArgs m = a;
        m.write_means = rq.mean ? 1 : 0;
        m.write_jac = mean_jac ? 1 : 0;
        launch::mean_stream_running(prm->model, mean_jac, avg, L, m, ctx->stream);
    }
    if (stj) launch::cov_running_stj(avg, a, ctx->stream);
    else if (rq.cov) launch::cov_running(prm->model, avg, a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
static int stream_running_lanes(const cpi_params *prm, int64_t U, int32_t N, const cpi_outputs *rows) {
    return pick_lanes(prm, U, N, request_of(rows).jac && prm->model != CPI_MODEL_V2);   // as running_device: model 2's rows are not the mean kernel's
}
static int stream_running_impl(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, const RunArgs *runs, int64_t R, int64_t K,
                               const double *stream, int64_t U, const double *update_times, int32_t N, const double *lin,
                               const double *q_k_lin, void *workspace, const cpi_outputs *rows) {
    bool noop;
    const int rc = stream_running_check(ctx, who, with_stj, prm, runs != nullptr, R, K, U, N, stream, runs ? runs->soff : nullptr, update_times,
                                        runs ? runs->uoff : nullptr, lin, q_k_lin, rows, noop);
    if (rc != CPI_OK || noop) return rc;
    if (!workspace) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_workspace(ctx, who, workspace));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    RunArgs ra;
    if (runs) { ra = *runs; ra.R = (int)R; }
    const StreamCut sc = stream_cut(K, update_times, workspace, U, runs ? &ra : nullptr);
    CPI_TRY(cut_launch(ctx, sc, stream, U, N));
    return stream_running_launch(ctx, prm, sc, stream, N, stream_running_lanes(prm, U, N, rows), lin, q_k_lin, rows, 0, U);
}
extern "C" int cpi_preintegrate_stream_running(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                               const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                               void *workspace, const cpi_outputs *rows) {
    return stream_running_impl(ctx, "cpi_preintegrate_stream_running", false, prm, nullptr, 0, K, stream, U, update_times, N, lin, q_k_lin,
                               workspace, rows);
}
extern "C" int cpi_preintegrate_streams_running(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                                const int64_t *stream_offsets, int64_t U, const double *update_times,
                                                const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                                void *workspace, const cpi_outputs *rows) {
    RunArgs ra;
    ra.soff = reinterpret_cast<const long long *>(stream_offsets);
    ra.uoff = reinterpret_cast<const long long *>(update_offsets);
    ra.R = 0;
    return stream_running_impl(ctx, "cpi_preintegrate_streams_running", false, prm, &ra, R, K, stream, U, update_times, N, lin, q_k_lin,
                               workspace, rows);
}
// One entry for one stream (R == 1, both offsets NULL: cpi_preintegrate_stream_running) or many (cpi_preintegrate_streams_running).
static bool one_stream(int64_t R, const void *stream_offsets, const void *update_offsets) { return R == 1 && !stream_offsets && !update_offsets; }
extern "C" int cpi_stream_running_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                            const int64_t *stream_offsets, int64_t U, const double *update_times,
                                            const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                            void *workspace, const cpi_outputs *rows) {
    static const char who[] = "cpi_stream_running_stj_batch";
    RunArgs ra;
    ra.soff = reinterpret_cast<const long long *>(stream_offsets);
    ra.uoff = reinterpret_cast<const long long *>(update_offsets);
    ra.R = 0;
    const bool one = one_stream(R, stream_offsets, update_offsets);
    return stream_running_impl(ctx, who, true, prm, one ? nullptr : &ra, one ? 0 : R, K, stream, U, update_times, N, lin, q_k_lin, workspace, rows);
}

// The query family by ABSOLUTE time over IMU stream(s) (include/cpi_amd.h: cpi_query_stream_batch): the cut kernel into the workspace,
// then the kernels of cpi_query_stream.hip, which find the window among the run's update times and the interval among the patched
// stamps before they do what cpi_query_kernel / cpi_query_cov_kernel / cpi_query_stj_kernel do -- one after the other on the context's
// stream.  The first kernel that runs writes qwin_out (the mean kernel alone when out asks for nothing).
// *done: a no-op call.  The checks the device and the host form share, up to the ones on rows and the workspace.
static int query_stream_check(cpi_ctx *ctx, const char *who, const cpi_params *prm, bool one, int64_t R, int64_t K, int64_t U, int32_t N,
                              const void *stream, const void *soff, const void *update_times, const void *uoff, const void *lin,
                              const void *q_k_lin, int64_t Q, const void *qtime, const cpi_outputs *out, bool *done) {
    *done = true;
    CPI_TRY(query_check(ctx, who, prm, request_of(out), QUERY_COV | QUERY_STJ));
    if (R < 0 || K < 0 || U < 0 || N < 0 || Q < 0) return refuse(ctx, who, "negative size");
    if (Q == 0) return CPI_OK;
    if (U == 0) return refuse(ctx, who, "U is 0: there is no window to query");
    if (R == 0) return refuse(ctx, who, "U > 0 windows and no run");
    if (R > 0x7ffffffeLL) return refuse(ctx, who, "R exceeds 2^31 - 2 runs");
    if (K == 0) return refuse(ctx, who, one ? "the stream is empty" : "the streams hold no reading");
    if (!stream || !update_times || !lin || !qtime || (!one && (!soff || !uoff))) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_grid(ctx, who, "U", U));
    CPI_TRY(check_qk(ctx, who, prm, q_k_lin));
    CPI_TRY(check_N(ctx, who, N));
    CPI_TRY(check_lanes(ctx, prm));
    if (!grid_ok(Q)) return refuse(ctx, who, "Q exceeds 2^31 - 1 queries per call (32-bit grid)");
    *done = false;
    return CPI_OK;
}
extern "C" int cpi_query_stream_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                      const int64_t *stream_offsets, int64_t U, const double *update_times,
                                      const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                      void *workspace, const cpi_outputs *rows, int64_t Q, const int32_t *qrun, const double *qtime,
                                      int32_t *qwin_out, const cpi_outputs *out) {
    static const char who[] = "cpi_query_stream_batch";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows || !out) return refuse(ctx, who, "prm/rows/out is NULL");
    const bool one = one_stream(R, stream_offsets, update_offsets);
    bool done;
    CPI_TRY(query_stream_check(ctx, who, prm, one, R, K, U, N, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin, Q, qtime, out, &done));
    if (done) return CPI_OK;
    if (!workspace) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_workspace(ctx, who, workspace));
    const Request rq = request_of(out);
    if (N > 0 && rq.any()) CPI_TRY(query_rows_check(ctx, who, prm, rows, out));   // N == 0: every query is the zero state and rows is not read
    if (!rq.any() && !qwin_out) return CPI_OK;
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;
    const bool mean_jac = rq.jac && !stj;
    const bool means = rq.mean || mean_jac || !rq.any();
    const bool avg = prm->imu_avg != 0;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    RunArgs ra;
    ra.soff = reinterpret_cast<const long long *>(stream_offsets);
    ra.uoff = reinterpret_cast<const long long *>(update_offsets);
    ra.R = (int)R;
    const StreamCut sc = stream_cut(K, update_times, workspace, U, one ? nullptr : &ra);
    CPI_TRY(cut_launch(ctx, sc, stream, U, N));
    StreamQueryArgs a;
    memset(&a, 0, sizeof a);
    a.U = U; a.N = N; a.stream = stream; a.K = K; a.update = update_times; a.uoff = one ? nullptr : ra.uoff; a.R = (int)R;
    a.first = sc.first; a.count = sc.count; a.tstart = sc.tstart; a.tend = sc.tend; a.lin = lin; a.qk = q_k_lin;
    for (int i = 0; i < 3; i++) a.grav[i] = prm->grav[i];
    if (rq.any()) a.rows = *rows;   // (a call for qwin_out alone reads no row)
    a.Q = Q; a.qrun = qrun; a.qtime = qtime; a.qwin_out = qwin_out;
    a.wtrips = 0;
    while ((1ll << a.wtrips) < (long long)U + 1) a.wtrips++;
    a.trips = query_trips(N); a.out = *out;
    if (mean_jac) {
        // the Jacobian instance carries all five matrices: the ones out does not ask for are read from a field that is there
        const double *any = rows->J_q ? rows->J_q : rows->J_a ? rows->J_a : rows->J_b ? rows->J_b : rows->H_a ? rows->H_a : rows->H_b;
        double **f[5] = { &a.rows.J_q, &a.rows.J_a, &a.rows.J_b, &a.rows.H_a, &a.rows.H_b };
        for (double **x : f) if (!*x) *x = const_cast<double *>(any);
    }
    if (means) { launch::squery_mean(prm->model, mean_jac, avg, a, ctx->stream); a.qwin_out = nullptr; }
    if (stj) { launch::squery_jac2(avg, a, ctx->stream); a.qwin_out = nullptr; }
    if (rq.cov) {
        const double q4[4] = { prm->sigma_w * prm->sigma_w, prm->sigma_wb * prm->sigma_wb, prm->sigma_a * prm->sigma_a, prm->sigma_ab * prm->sigma_ab };
        launch::squery_cov(prm->model, avg, a, q4, ctx->stream);
    }
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// re-linearisation sweeps
// ============================================================================================
// Lanes per factor of the dense sweep: 16 gives the most wavefronts (small sweeps), fewer lanes do less redundant
// arithmetic.  Measured on MI355X, 1 M factors: plain 0.82 ms with 8 lanes vs 1.09 ms with 16; whitened (37 KB vs 19 KB of
// LDS per wavefront) 1.45 ms with 8 vs 1.37 ms with 16.
static int factor_lanes(int64_t F, bool whiten) {
#ifdef CPI_EXPERIMENTS
    if (expsw::factor_lanes()) return expsw::factor_lanes();
#endif
    if (whiten) return 16;
    return F >= 32768 ? 8 : 16;
}

// argument checks shared by the four sweeps; fills the kernel argument block
static int factor_args(cpi_ctx *ctx, const char *who, int32_t model, const double grav[3], int64_t F, const cpi_outputs *meas,
                       const double *lin, const double *q_k_lin, const double *states, int64_t S, const int32_t *idx_i,
                       const int32_t *idx_j, FactorArgs &a) {
    const std::string w(who);
    if (model != CPI_MODEL_V1 && model != CPI_MODEL_V2) return fail(ctx, CPI_ERR_INVALID, w + ": model must be 1 or 2");
    if (F < 0) return fail(ctx, CPI_ERR_INVALID, w + ": negative size");
    if (!grav || !meas || !lin || !states) return fail(ctx, CPI_ERR_INVALID, w + ": NULL argument");
    if (!meas->DT || !meas->alpha || !meas->beta || !meas->q || !meas->J_q || !meas->J_a || !meas->J_b || !meas->H_a || !meas->H_b)
        return fail(ctx, CPI_ERR_INVALID, w + ": measurement fields DT/alpha/beta/q/J_q/J_a/J_b/H_a/H_b are required");
    if (model == CPI_MODEL_V2 && (!q_k_lin || !meas->O_a || !meas->O_b))
        return fail(ctx, CPI_ERR_INVALID, w + ": model 2 needs q_k_lin, O_a, O_b");
    if (!grid_ok(F)) return fail(ctx, CPI_ERR_INVALID, w + ": F exceeds 2^31 - 1 factors per call");
    if (S <= 0 || (!idx_i && S < F) || (!idx_j && S < F + 1))
        return fail(ctx, CPI_ERR_INVALID, w + ": S (number of states) must be >= 1, and >= F + 1 when idx_i / idx_j are NULL (chained states f, f + 1)");
    memset(&a, 0, sizeof a);
    a.F = F;
    for (int i = 0; i < 3; i++) a.grav[i] = grav[i];
    a.meas = *meas; a.lin = lin; a.qk = q_k_lin; a.states = states; a.S = S; a.idx_i = idx_i; a.idx_j = idx_j;
    return CPI_OK;
}

static int factor_eval_impl(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F, const cpi_outputs *meas,
                            const double *lin, const double *q_k_lin, const double *states, int64_t S, const int32_t *idx_i,
                            const int32_t *idx_j, const double *sqrt_info, bool tri, double *err, double *H1, double *H2) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0) return CPI_OK;
    if (!err) return fail(ctx, CPI_ERR_INVALID, "cpi_factor_eval_batch: NULL argument");
    FactorArgs a;
    const int rc = factor_args(ctx, "cpi_factor_eval_batch", model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, a);
    if (rc != CPI_OK) return rc;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    a.err = err; a.H1 = H1; a.H2 = H2; a.sqrt_info = sqrt_info; a.r_tri = tri ? 1 : 0;
    launch::factor(model, sqrt_info != nullptr, factor_lanes(F, sqrt_info != nullptr), a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

extern "C" int cpi_factor_eval_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                     const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                     const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                     double *err, double *H1, double *H2) {
    return factor_eval_impl(ctx, model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, nullptr, false, err, H1, H2);
}

extern "C" int cpi_factor_eval_whitened_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                              const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                              const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                              const double *sqrt_info, double *err, double *H1, double *H2) {
    if (ctx && !sqrt_info) return fail(ctx, CPI_ERR_INVALID, "cpi_factor_eval_whitened_batch: sqrt_info is NULL");
    return factor_eval_impl(ctx, model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, sqrt_info, false, err, H1, H2);
}
extern "C" int cpi_factor_eval_whitened_tri_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                                  const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                                  const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                                  const double *R_tri, double *err, double *H1, double *H2) {
    if (ctx && !R_tri) return fail(ctx, CPI_ERR_INVALID, "cpi_factor_eval_whitened_tri_batch: R_tri is NULL");
    return factor_eval_impl(ctx, model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, R_tri, true, err, H1, H2);
}

extern "C" int cpi_factor_eval_packed_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                            const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                            const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                            double *packed) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0) return CPI_OK;
    if (!packed) return fail(ctx, CPI_ERR_INVALID, "cpi_factor_eval_packed_batch: NULL argument");
    FactorArgs a;
    const int rc = factor_args(ctx, "cpi_factor_eval_packed_batch", model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, a);
    if (rc != CPI_OK) return rc;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    // lanes per factor.  Every lane of a factor repeats the shared quaternion algebra, so fewer lanes = less VALU per factor
    // but more LDS per wavefront (a factor's staged record + packed output = 1.5 KB).  Measured (MI355X, 1 M factors, model 1 /
    // model 2, us): 8 lanes 383 / 435 (VALU 53 % busy at 2 wavefronts per SIMD), 6: 335 / 389, 4: 290 / 324, 3: 281 / 314,
    // 2: 328 / 361 (48 KB of LDS: one wavefront per SIMD); 100 k factors: 4 lanes 31.5, 3 lanes 32.5.
    // Round 6 (the result overlays the record: 928 B of LDS per factor, 8 wavefronts per CU at 3 lanes): 2 / 3 / 4 / 6 lanes
    // 252-254 / 249-255 / 256-258 / 315-317 (model 2: 276-282 / 269-272 / 282-283 / 334-337); 100 k factors 31.7 / 27.3 / 26.9-27.4 /
    // 31.0; 20 k 8.7 / 7.9-8.0 / 8.5 / 8.4: three at every size.
    int lpf = 3;
    (void)F;
#ifdef CPI_EXPERIMENTS
    if (expsw::packed_lpf()) lpf = expsw::packed_lpf();
#endif
    launch::factor_packed(model, lpf, a, packed, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

static bool bytes_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa && pb && na && nb && pa < pb + nb && pb < pa + na;
}
static int sqrt_information_impl(cpi_ctx *ctx, int64_t F, const double *P, double *R, bool packed) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F < 0) return fail(ctx, CPI_ERR_INVALID, "cpi_sqrt_information_batch: negative size");
    if (F == 0) return CPI_OK;
    if (!P || !R) return fail(ctx, CPI_ERR_INVALID, "cpi_sqrt_information_batch: NULL argument");
    if (!grid_ok(F)) return fail(ctx, CPI_ERR_INVALID, "cpi_sqrt_information_batch: F exceeds 2^31 - 1 factors per call");
    // The kernel stages a wavefront's four factors before it stores any of them: R == P is safe, a shifted R is not.
    const size_t bytes = (size_t)F * (packed ? 120 : 225) * sizeof(double);
    if (R != P && bytes_overlap(R, bytes, P, bytes))
        return packed ? refuse(ctx, "cpi_sqrt_information_packed_batch", "R_tri overlaps P_sym (R_tri == P_sym exactly is the in-place form)")
                      : refuse(ctx, "cpi_sqrt_information_batch", "sqrt_info overlaps P (sqrt_info == P exactly is the in-place form)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    launch::sqrt_info((long long)F, P, R, packed, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_sqrt_information_batch(cpi_ctx *ctx, int64_t F, const double *P, double *sqrt_info) {
    return sqrt_information_impl(ctx, F, P, sqrt_info, false);
}
extern "C" int cpi_sqrt_information_packed_batch(cpi_ctx *ctx, int64_t F, const double *P_sym, double *R_tri) {
    return sqrt_information_impl(ctx, F, P_sym, R_tri, true);
}

static int factor_hessian_impl(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                               const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                               const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                               const double *sqrt_info, bool tri, double *hess) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0) return CPI_OK;
    if (!sqrt_info || !hess) return fail(ctx, CPI_ERR_INVALID, "cpi_factor_hessian_batch: NULL argument");
    FactorArgs a;
    const int rc = factor_args(ctx, "cpi_factor_hessian_batch", model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, a);
    if (rc != CPI_OK) return rc;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    a.sqrt_info = sqrt_info; a.r_tri = tri ? 1 : 0;
    launch::factor_hessian(model, a, hess, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_factor_hessian_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                        const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                        const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                        const double *sqrt_info, double *hess) {
    return factor_hessian_impl(ctx, model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, sqrt_info, false, hess);
}
extern "C" int cpi_factor_hessian_tri_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                            const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                            const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                            const double *R_tri, double *hess) {
    return factor_hessian_impl(ctx, model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, R_tri, true, hess);
}

extern "C" int cpi_predict_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                 const cpi_outputs *meas, const double *states_i, int64_t S, const int32_t *idx_i,
                                 double *states_j) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (model != CPI_MODEL_V1 && model != CPI_MODEL_V2) return fail(ctx, CPI_ERR_INVALID, "cpi_predict_batch: model must be 1 or 2");
    if (F < 0) return fail(ctx, CPI_ERR_INVALID, "cpi_predict_batch: negative size");
    if (F == 0) return CPI_OK;
    if (!grav || !meas || !states_i || !states_j || !meas->DT || !meas->alpha || !meas->beta || !meas->q)
        return fail(ctx, CPI_ERR_INVALID, "cpi_predict_batch: NULL argument");
    if (!grid_ok(F)) return fail(ctx, CPI_ERR_INVALID, "cpi_predict_batch: F exceeds 2^31 - 1 factors per call");
    if (S <= 0 || (!idx_i && S < F)) return fail(ctx, CPI_ERR_INVALID, "cpi_predict_batch: S (number of states) must be >= 1, and >= F when idx_i is NULL");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    PredictArgs a;
    memset(&a, 0, sizeof a);
    a.F = F;
    for (int i = 0; i < 3; i++) a.grav[i] = grav[i];
    a.meas = *meas; a.states_i = states_i; a.S = S; a.idx_i = idx_i; a.states_j = states_j;
    launch::predict(model, a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}


// ============================================================================================
// the optimiser's trial step: retract / localCoordinates of the states, the whitened cost at the trial states (cpi_trial.hip)
// ============================================================================================
// Everything these entries can refuse is refused BEFORE the context is looked at (cpi_last_error(NULL) holds the text then), as
// cpi_merge_batch does.
// "No output may overlap an input or another output": the first output, in order, that does is named in the refusal.  A NULL or
// empty span overlaps nothing.
struct Span {
    const void *p;
    size_t bytes;
    const char *name;
};
static int refuse_overlaps(cpi_ctx *ctx, const char *who, const Span *outs, int n_out, const Span *ins, int n_in) {
    for (int o = 0; o < n_out; o++) {
        bool bad = false;
        for (int k = 0; k < n_in; k++) bad = bad || bytes_overlap(outs[o].p, outs[o].bytes, ins[k].p, ins[k].bytes);
        for (int q = o + 1; q < n_out; q++) bad = bad || bytes_overlap(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes);
        if (bad) return refuse(ctx, who, outs[o].name, " overlaps an input or another output");
    }
    return CPI_OK;
}
// what the device and the host forms of retract / local refuse alike, before the context is looked at
static int retract_check(cpi_ctx *ctx, const char *who, int64_t S, const double *states_in, const double *delta, const double *states_out) {
    if (S < 0) return refuse(ctx, who, "negative size");
    if (S > 0 && (!states_in || !delta || !states_out)) return refuse(ctx, who, "NULL argument");
    const size_t ns = (size_t)S * 16 * sizeof(double), nd = (size_t)S * 15 * sizeof(double);
    if ((states_out != states_in && bytes_overlap(states_out, ns, states_in, ns)) || bytes_overlap(states_out, ns, delta, nd) ||
        bytes_overlap(states_in, ns, delta, nd))
        return refuse(ctx, who, "states_out overlaps states_in or delta (states_out == states_in exactly is the in-place form), or delta overlaps states_in");
    return CPI_OK;
}
static int local_check(cpi_ctx *ctx, const char *who, int64_t S, const double *x, const double *other, const double *xi) {
    if (S < 0) return refuse(ctx, who, "negative size");
    if (S > 0 && (!x || !other || !xi)) return refuse(ctx, who, "NULL argument");
    const size_t ns = (size_t)S * 16 * sizeof(double), nx = (size_t)S * 15 * sizeof(double);
    if (bytes_overlap(xi, nx, x, ns) || bytes_overlap(xi, nx, other, ns)) return refuse(ctx, who, "xi overlaps x or other");
    return CPI_OK;
}
extern "C" int cpi_retract_batch(cpi_ctx *ctx, int64_t S, const double *states_in, const double *delta, double *states_out) {
    static const char who[] = "cpi_retract_batch";
    CPI_TRY(retract_check(ctx, who, S, states_in, delta, states_out));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (S == 0) return CPI_OK;
    if (!grid_ok((S + 63) / 64)) return refuse(ctx, who, "S exceeds the 32-bit grid (64 states per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    launch::retract((long long)S, states_in, delta, states_out, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_local_batch(cpi_ctx *ctx, int64_t S, const double *x, const double *other, double *xi) {
    static const char who[] = "cpi_local_batch";
    CPI_TRY(local_check(ctx, who, S, x, other, xi));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (S == 0) return CPI_OK;
    if (!grid_ok((S + 63) / 64)) return refuse(ctx, who, "S exceeds the 32-bit grid (64 states per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    launch::local_coordinates((long long)S, x, other, xi, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

extern "C" size_t cpi_factor_cost_total_doubles(int64_t F) { return launch::cost_total_doubles(F > 0 ? (long long)F : 0); }

// Lanes per factor of the cost kernel (cpi_trial_kernels.hpp).  Measured on an MI355X (tools/trial_step_bench.py, 1 M factors, R packed,
// model 1 / 2, ms): 16 lanes 0.39-0.40 / 0.42-0.43, 8 lanes 0.38 / 0.41, 4 lanes 0.43 / 0.46 -- sixteen idle fifteen lanes of sixteen through the
// core, four need 32 KB of LDS per wavefront.  Eight at every size (profiles/trial_step.md).
static int cost_lanes(int64_t F) {
#ifdef CPI_EXPERIMENTS
    if (expsw::cost_lanes()) return expsw::cost_lanes();
#endif
    (void)F;
    return 8;
}
static int factor_cost_impl(cpi_ctx *ctx, const char *who, int32_t model, const double grav[3], int64_t F, const cpi_outputs *meas,
                            const double *lin, const double *q_k_lin, const double *states, int64_t S, const int32_t *idx_i,
                            const int32_t *idx_j, const double *R, bool tri, double *chi2, double *werr, double *total) {
    if (model != CPI_MODEL_V1 && model != CPI_MODEL_V2) return refuse(ctx, who, "model must be 1 or 2");
    if (F < 0) return refuse(ctx, who, "negative size");
    FactorArgs a;
    if (F > 0) {
        if (!chi2) return refuse(ctx, who, "chi2 is NULL");
        if (!R) return refuse(ctx, who, tri ? "R_tri is NULL" : "sqrt_info is NULL");
        CPI_TRY(factor_args(ctx, who, model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, a));
        const size_t d = sizeof(double);
        const Span outs[3] = { { chi2, (size_t)F * d, "chi2" }, { werr, (size_t)F * 15 * d, "werr" },
                               { total, cpi_factor_cost_total_doubles(F) * d, "total (the workspace)" } };
        Span ins[17] = { { lin, (size_t)F * 6 * d, "" }, { q_k_lin, (size_t)F * 4 * d, "" }, { states, (size_t)S * 16 * d, "" },
                         { idx_i, (size_t)F * sizeof(int32_t), "" }, { idx_j, (size_t)F * sizeof(int32_t), "" },
                         { R, (size_t)F * (tri ? CPI_TRI_DOUBLES : 225) * d, "" } };
        for (int k = 0; k < 11; k++) ins[6 + k] = { out_field_c(meas, k), (size_t)F * OUT_N[k] * d, "" };   // the measurement: every field but P / P_sym
        CPI_TRY(refuse_overlaps(ctx, who, outs, 3, ins, 17));
    }
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0 && !total) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    if (F > 0) {
        a.sqrt_info = R; a.r_tri = tri ? 1 : 0;
        launch::factor_cost(model, cost_lanes(F), a, chi2, werr, ctx->stream);
    }
    if (total) launch::cost_total((long long)F, chi2, total, ctx->stream);   // F == 0: the empty sum, 0
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_factor_cost_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                     const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                     const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                     const double *sqrt_info, double *chi2, double *werr, double *total) {
    return factor_cost_impl(ctx, "cpi_factor_cost_batch", model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, sqrt_info, false, chi2, werr, total);
}
extern "C" int cpi_factor_cost_tri_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                         const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                         const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                         const double *R_tri, double *chi2, double *werr, double *total) {
    return factor_cost_impl(ctx, "cpi_factor_cost_tri_batch", model, grav, F, meas, lin, q_k_lin, states, S, idx_i, idx_j, R_tri, true, chi2, werr, total);
}

// ============================================================================================
// cpi_chain_solve_batch: the damped block-tridiagonal solve of chains of IMU factors (cpi_chain_solve_kernel, cpi_chain.hip)
// ============================================================================================
extern "C" size_t cpi_chain_solve_workspace_doubles(int64_t S) { return launch::chain_workspace_doubles(S > 0 ? (long long)S : 0); }

// what both forms refuse alike, before the context is looked at; host: the arrays are the caller's host arrays (no workspace)
static int chain_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                       const int64_t *ffirst, const double *hess, const double *prior, const double *lambda, int32_t damping,
                       double *delta, int32_t *status, double *workspace, bool host) {
    if (C < 0 || S < 0 || F < 0) return refuse(ctx, who, "negative size");
    if (G < 1) return refuse(ctx, who, "G (the longest chain in states) must be >= 1");
    if (G > 0x7fffffffLL) return refuse(ctx, who, "G exceeds 2^31 - 1 states per chain");
    if (damping != CPI_DAMP_IDENTITY && damping != CPI_DAMP_DIAGONAL) return refuse(ctx, who, "damping must be CPI_DAMP_IDENTITY or CPI_DAMP_DIAGONAL");
    if (C == 0) return CPI_OK;
    if (!hess && G > 1) return refuse(ctx, who, "hess is NULL (only chains of one state, G == 1, need none)");
    if (!delta) return refuse(ctx, who, "delta is NULL");
    if (!host && !workspace) return refuse(ctx, who, "workspace is NULL");
    const size_t d = sizeof(double);
    const Span outs[3] = { { delta, (size_t)S * 15 * d, "delta" }, { status, (size_t)C * sizeof(int32_t), "status" },
                           { workspace, workspace ? cpi_chain_solve_workspace_doubles(S) * d : 0, "workspace" } };
    const Span ins[6] = { { first, (size_t)C * sizeof(int64_t), "" }, { count, (size_t)C * sizeof(int32_t), "" }, { ffirst, (size_t)C * sizeof(int64_t), "" },
                          { hess, (size_t)F * 496 * d, "" }, { prior, (size_t)S * 136 * d, "" }, { lambda, (size_t)C * d, "" } };
    return refuse_overlaps(ctx, who, outs, 3, ins, 6);
}

extern "C" int cpi_chain_solve_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                     const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                     const double *hess, const double *prior, const double *lambda, int32_t damping,
                                     double *delta, int32_t *status, double *workspace) {
    static const char who[] = "cpi_chain_solve_batch";
    CPI_TRY(chain_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, lambda, damping, delta, status, workspace, false));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    if (!grid_ok((C + 3) / 4)) return refuse(ctx, who, "C exceeds the 32-bit grid (4 chains per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    ChainArgs a;
    memset(&a, 0, sizeof a);
    a.C = C; a.G = (int)G; a.S = S; a.F = F;
    a.first = (const long long *)first; a.count = count; a.ffirst = (const long long *)ffirst;
    a.hess = hess; a.prior = prior; a.lambda = lambda; a.diagonal = damping == CPI_DAMP_DIAGONAL;
    a.delta = delta; a.status = status; a.workspace = workspace;
    launch::chain_solve(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// cpi_chain_marginals_batch: the state covariances of solved chains (cpi_marginals_kernel, cpi_marginals.hip)
// ============================================================================================
// what both forms refuse alike, before the context is looked at; host: no workspace, status is an output, and the inputs of the solve
// (F, ffirst, hess, prior: the device form has none) are checked after everything the forms share
static int marginals_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                           const int64_t *ffirst, const double *hess, const double *prior, const int32_t *status, const double *workspace,
                           double *cov, double *cross, bool host) {
    if (C < 0 || S < 0 || F < 0) return refuse(ctx, who, "negative size");
    if (G < 1) return refuse(ctx, who, "G (the longest chain in states) must be >= 1");
    if (G > 0x7fffffffLL) return refuse(ctx, who, "G exceeds 2^31 - 1 states per chain");
    if (S > 0 && !host && !workspace) return refuse(ctx, who, "workspace is NULL");
    if (S > 0 && !cov) return refuse(ctx, who, "cov is NULL");
    const size_t d = sizeof(double);
    const Span outs[3] = { { cov, (size_t)S * 120 * d, "cov" }, { cross, (size_t)S * 225 * d, "cross" },
                           { host ? status : nullptr, (size_t)C * sizeof(int32_t), "status" } };
    const Span ins[4] = { { workspace, workspace ? cpi_chain_solve_workspace_doubles(S) * d : 0, "" }, { first, (size_t)C * sizeof(int64_t), "" },
                          { count, (size_t)C * sizeof(int32_t), "" }, { host ? nullptr : status, (size_t)C * sizeof(int32_t), "" } };
    CPI_TRY(refuse_overlaps(ctx, who, outs, 3, ins, 4));
    if (!host) return CPI_OK;
    if (C > 0 && !hess && G > 1) return refuse(ctx, who, "hess is NULL (only chains of one state, G == 1, need none)");
    const Span solve_ins[3] = { { ffirst, (size_t)C * sizeof(int64_t), "" }, { hess, (size_t)F * 496 * d, "" }, { prior, (size_t)S * 136 * d, "" } };
    return refuse_overlaps(ctx, who, outs, 3, solve_ins, 3);
}

extern "C" int cpi_chain_marginals_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S,
                                         const int64_t *first, const int32_t *count, const int32_t *status,
                                         const double *workspace, double *cov, double *cross) {
    static const char who[] = "cpi_chain_marginals_batch";
    CPI_TRY(marginals_check(ctx, who, C, G, S, 0, first, count, nullptr, nullptr, nullptr, status, workspace, cov, cross, false));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0 || S == 0) return CPI_OK;               // no chain has a state
    if (!grid_ok((C + 3) / 4)) return refuse(ctx, who, "C exceeds the 32-bit grid (4 chains per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    MarginalsArgs a;
    memset(&a, 0, sizeof a);
    a.C = C; a.G = (int)G; a.S = S;
    a.first = (const long long *)first; a.count = count; a.status = status;
    a.workspace = workspace; a.cov = cov; a.cross = cross;
    launch::chain_marginals(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// cpi_chain_marginalize_batch: the oldest states of chains eliminated into a prior (cpi_marginalize_kernel, cpi_marginalize.hip)
// ============================================================================================
// what both forms refuse alike, before the context is looked at
static int marginalize_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                             const int64_t *ffirst, const double *hess, const double *prior, const int32_t *drop, double *out, int32_t *status) {
    if (C < 0 || S < 0 || F < 0) return refuse(ctx, who, "negative size");
    if (G < 1) return refuse(ctx, who, "G (the longest chain in states) must be >= 1");
    if (G > 0x7fffffffLL) return refuse(ctx, who, "G exceeds 2^31 - 1 states per chain");
    if (C == 0) return CPI_OK;
    if (!hess && G > 1) return refuse(ctx, who, "hess is NULL (only chains of one state, G == 1, need none)");
    if (!out) return refuse(ctx, who, "out is NULL");
    const size_t d = sizeof(double);
    const Span outs[2] = { { out, (size_t)C * 136 * d, "out" }, { status, (size_t)C * sizeof(int32_t), "status" } };
    const Span ins[6] = { { first, (size_t)C * sizeof(int64_t), "" }, { count, (size_t)C * sizeof(int32_t), "" }, { ffirst, (size_t)C * sizeof(int64_t), "" },
                          { hess, (size_t)F * 496 * d, "" }, { prior, (size_t)S * 136 * d, "" }, { drop, (size_t)C * sizeof(int32_t), "" } };
    return refuse_overlaps(ctx, who, outs, 2, ins, 6);
}

extern "C" int cpi_chain_marginalize_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                           const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                           const double *hess, const double *prior,
                                           int32_t M, const int32_t *drop,
                                           double *out, int32_t *status) {
    static const char who[] = "cpi_chain_marginalize_batch";
    CPI_TRY(marginalize_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, drop, out, status));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    if (!grid_ok((C + 3) / 4)) return refuse(ctx, who, "C exceeds the 32-bit grid (4 chains per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    MarginalizeArgs a;
    memset(&a, 0, sizeof a);
    a.C = C; a.G = (int)G; a.S = S; a.F = F;
    a.first = (const long long *)first; a.count = count; a.ffirst = (const long long *)ffirst;
    a.hess = hess; a.prior = prior; a.M = M; a.drop = drop;
    a.out = out; a.status = status;
    launch::chain_marginalize(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// cpi_chain_condense_batch / cpi_chain_expand_batch: segments of chains condensed in parallel (cpi_condense_kernel / cpi_expand_kernel,
// cpi_condense.hip)
// ============================================================================================
extern "C" int64_t cpi_chain_condense_states(int64_t G, int64_t K) {
    if (G < 2 || K < 1) return G < 0 ? 0 : (G < 2 ? G : 0);   // K < 1 is refused by the entries: no layout
    return (G - 2) / K + 2;
}
extern "C" size_t cpi_chain_condense_workspace_doubles(int64_t S) { return launch::condense_workspace_doubles(S > 0 ? (long long)S : 0); }

// what the device and the host forms refuse alike, before the context is looked at; host: no workspace
static int condense_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                          const int64_t *ffirst, const double *hess, const double *prior, const double *lambda, int32_t damping, int64_t K,
                          double *rhess, double *rprior, int32_t *rcount, int32_t *status, double *workspace, bool host) {
    if (C < 0 || S < 0 || F < 0) return refuse(ctx, who, "negative size");
    if (G < 1) return refuse(ctx, who, "G (the longest chain in states) must be >= 1");
    if (G > 0x7fffffffLL) return refuse(ctx, who, "G exceeds 2^31 - 1 states per chain");
    if (K < 1) return refuse(ctx, who, "K (the factors of a segment) must be >= 1");
    if (damping != CPI_DAMP_IDENTITY && damping != CPI_DAMP_DIAGONAL) return refuse(ctx, who, "damping must be CPI_DAMP_IDENTITY or CPI_DAMP_DIAGONAL");
    if (C == 0) return CPI_OK;
    const int64_t Gr = cpi_chain_condense_states(G, K);
    if (!hess && G > 1) return refuse(ctx, who, "hess is NULL (only chains of one state, G == 1, need none)");
    if (!rhess && G > 1) return refuse(ctx, who, "rhess is NULL (only chains of one state, G == 1, need none)");
    if (!rprior) return refuse(ctx, who, "rprior is NULL");
    if (!rcount) return refuse(ctx, who, "rcount is NULL");
    if (!host && !workspace) return refuse(ctx, who, "workspace is NULL");
    const size_t d = sizeof(double);
    const Span outs[5] = { { rhess, (size_t)C * (size_t)(Gr - 1) * 496 * d, "rhess" }, { rprior, (size_t)C * (size_t)Gr * 136 * d, "rprior" },
                           { rcount, (size_t)C * sizeof(int32_t), "rcount" }, { status, (size_t)C * (size_t)(Gr - 1) * sizeof(int32_t), "status" },
                           { workspace, workspace ? cpi_chain_condense_workspace_doubles(S) * d : 0, "workspace" } };
    const Span ins[6] = { { first, (size_t)C * sizeof(int64_t), "" }, { count, (size_t)C * sizeof(int32_t), "" }, { ffirst, (size_t)C * sizeof(int64_t), "" },
                          { hess, (size_t)F * 496 * d, "" }, { prior, (size_t)S * 136 * d, "" }, { lambda, (size_t)C * d, "" } };
    return refuse_overlaps(ctx, who, outs, 5, ins, 6);
}
// K as the kernels take it: a K beyond the longest chain's factors cuts nothing, and max(G - 1, 1) cuts the same
static int condense_k(int64_t G, int64_t K) { return (int)(K < (G > 2 ? G - 1 : 1) ? K : (G > 2 ? G - 1 : 1)); }

extern "C" int cpi_chain_condense_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                        const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                        const double *hess, const double *prior, const double *lambda, int32_t damping, int64_t K,
                                        double *rhess, double *rprior, int32_t *rcount,
                                        int32_t *status, double *workspace) {
    static const char who[] = "cpi_chain_condense_batch";
    CPI_TRY(condense_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, lambda, damping, K, rhess, rprior, rcount, status, workspace, false));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    const int64_t Gr = cpi_chain_condense_states(G, K);
    if (C > 0x7fffffffffffffffLL / Gr || !grid_ok((launch::condense_groups(C, (int)Gr) + 3) / 4))
        return refuse(ctx, who, "C x segments exceeds the 32-bit grid (4 segments per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    CondenseArgs a;
    memset(&a, 0, sizeof a);
    a.C = C; a.G = (int)G; a.S = S; a.F = F;
    a.first = (const long long *)first; a.count = count; a.ffirst = (const long long *)ffirst;
    a.hess = hess; a.prior = prior; a.lambda = lambda; a.diagonal = damping == CPI_DAMP_DIAGONAL;
    a.K = condense_k(G, K); a.Gr = (int)Gr;
    a.rhess = rhess; a.rprior = rprior; a.rcount = rcount; a.status = status; a.workspace = workspace;
    launch::chain_condense(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

static int expand_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, const int64_t *first, const int32_t *count, int64_t K,
                        const double *rdelta, const double *workspace, double *delta) {
    if (C < 0 || S < 0) return refuse(ctx, who, "negative size");
    if (G < 1) return refuse(ctx, who, "G (the longest chain in states) must be >= 1");
    if (G > 0x7fffffffLL) return refuse(ctx, who, "G exceeds 2^31 - 1 states per chain");
    if (K < 1) return refuse(ctx, who, "K (the factors of a segment) must be >= 1");
    if (C == 0) return CPI_OK;
    if (!rdelta) return refuse(ctx, who, "rdelta is NULL");
    if (!workspace) return refuse(ctx, who, "workspace is NULL");
    if (!delta) return refuse(ctx, who, "delta is NULL");
    const size_t d = sizeof(double);
    const Span outs[1] = { { delta, (size_t)S * 15 * d, "delta" } };
    const Span ins[4] = { { first, (size_t)C * sizeof(int64_t), "" }, { count, (size_t)C * sizeof(int32_t), "" },
                          { rdelta, (size_t)C * (size_t)cpi_chain_condense_states(G, K) * 15 * d, "" },
                          { workspace, cpi_chain_condense_workspace_doubles(S) * d, "" } };
    return refuse_overlaps(ctx, who, outs, 1, ins, 4);
}

extern "C" int cpi_chain_expand_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S,
                                      const int64_t *first, const int32_t *count, int64_t K,
                                      const double *rdelta, const double *workspace, double *delta) {
    static const char who[] = "cpi_chain_expand_batch";
    CPI_TRY(expand_check(ctx, who, C, G, S, first, count, K, rdelta, workspace, delta));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    const int64_t Gr = cpi_chain_condense_states(G, K);
    if (C > 0x7fffffffffffffffLL / Gr || !grid_ok((launch::condense_groups(C, (int)Gr) + 3) / 4))
        return refuse(ctx, who, "C x segments exceeds the 32-bit grid (4 segments per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    ExpandArgs a;
    memset(&a, 0, sizeof a);
    a.C = C; a.G = (int)G; a.S = S;
    a.first = (const long long *)first; a.count = count; a.K = condense_k(G, K); a.Gr = (int)Gr;
    a.rdelta = rdelta; a.workspace = workspace; a.delta = delta;
    launch::chain_expand(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// The Levenberg-Marquardt step per chain: cpi_prior_relinearize_batch, cpi_chain_cost_batch, cpi_chain_accept_batch (cpi_lm.hip)
// ============================================================================================
// what the device and the host forms refuse alike, before the context is looked at
static int lm_prior_check(cpi_ctx *ctx, const char *who, int64_t S, int64_t P, const int32_t *idx, const double *states, const double *anchor,
                          const double *prior0, double *prior, double *pcost) {
    if (S < 0 || P < 0) return refuse(ctx, who, "negative size");
    if (!idx && P > S) return refuse(ctx, who, "P > S with idx NULL (record p belongs to state p)");
    if (P == 0) return CPI_OK;
    if ((S > 0 && !states) || !anchor || !prior0) return refuse(ctx, who, "NULL argument");   // S == 0: every record is skipped
    if (!prior && !pcost) return refuse(ctx, who, "prior and pcost are both NULL");
    const size_t d = sizeof(double);
    const Span outs[2] = { { prior, (size_t)S * 136 * d, "prior" }, { pcost, (size_t)S * d, "pcost" } };
    const Span ins[4] = { { idx, (size_t)P * sizeof(int32_t), "" }, { states, (size_t)S * 16 * d, "" }, { anchor, (size_t)P * 16 * d, "" },
                          { prior0, (size_t)P * 136 * d, "" } };
    return refuse_overlaps(ctx, who, outs, 2, ins, 4);
}
extern "C" int cpi_prior_relinearize_batch(cpi_ctx *ctx, int64_t S, int64_t P, const int32_t *idx,
                                           const double *states, const double *anchor, const double *prior0,
                                           double *prior, double *pcost) {
    static const char who[] = "cpi_prior_relinearize_batch";
    CPI_TRY(lm_prior_check(ctx, who, S, P, idx, states, anchor, prior0, prior, pcost));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (P == 0) return CPI_OK;
    if (!grid_ok((P + 3) / 4)) return refuse(ctx, who, "P exceeds the 32-bit grid (4 records per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    LmPriorArgs a;
    memset(&a, 0, sizeof a);
    a.S = S; a.P = P; a.idx = idx; a.states = states; a.anchor = anchor; a.prior0 = prior0; a.prior = prior; a.pcost = pcost;
    launch::lm_prior(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

static int lm_sizes_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F) {
    if (C < 0 || S < 0 || F < 0) return refuse(ctx, who, "negative size");
    if (G < 1) return refuse(ctx, who, "G (the longest chain in states) must be >= 1");
    if (G > 0x7fffffffLL) return refuse(ctx, who, "G exceeds 2^31 - 1 states per chain");
    return CPI_OK;
}
static int lm_cost_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                         const int64_t *ffirst, const double *chi2, const double *pcost, double *cost) {
    CPI_TRY(lm_sizes_check(ctx, who, C, G, S, F));
    if (C == 0) return CPI_OK;
    if (!chi2 && G > 1) return refuse(ctx, who, "chi2 is NULL (only chains of one state, G == 1, need none)");
    if (!cost) return refuse(ctx, who, "cost is NULL");
    const size_t d = sizeof(double);
    const Span outs[1] = { { cost, (size_t)C * d, "cost" } };
    const Span ins[5] = { { first, (size_t)C * sizeof(int64_t), "" }, { count, (size_t)C * sizeof(int32_t), "" }, { ffirst, (size_t)C * sizeof(int64_t), "" },
                          { chi2, (size_t)F * d, "" }, { pcost, (size_t)S * d, "" } };
    return refuse_overlaps(ctx, who, outs, 1, ins, 5);
}
static void lm_cost_args(LmCostArgs &a, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                         const int64_t *ffirst, const double *chi2, const double *pcost, double *cost) {
    memset(&a, 0, sizeof a);
    a.C = C; a.G = (int)G; a.S = S; a.F = F;
    a.first = (const long long *)first; a.count = count; a.ffirst = (const long long *)ffirst;
    a.chi2 = chi2; a.pcost = pcost; a.cost = cost;
}
extern "C" int cpi_chain_cost_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                    const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                    const double *chi2, const double *pcost, double *cost) {
    static const char who[] = "cpi_chain_cost_batch";
    CPI_TRY(lm_cost_check(ctx, who, C, G, S, F, first, count, ffirst, chi2, pcost, cost));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    if (!grid_ok((C + 3) / 4)) return refuse(ctx, who, "C exceeds the 32-bit grid (4 chains per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    LmCostArgs a;
    lm_cost_args(a, C, G, S, F, first, count, ffirst, chi2, pcost, cost);
    launch::lm_cost(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// NULL: the defaults of GTSAM's LevenbergMarquardtParams (lambdaFactor 10, lambdaLowerBound 0, lambdaUpperBound 1e5,
// absoluteErrorTol / relativeErrorTol 1e-5)
static const cpi_lm_params kLmDefaults = { 0.1, 10.0, 0.0, 1e5, 1e-5, 1e-5 };
static int lm_accept_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count,
                           const int64_t *ffirst, const cpi_lm_params *params, const double *chi2_new, const double *pcost_new,
                           const double *trial, double *cost, double *states, double *chi2, double *lambda, int32_t *phase,
                           int32_t *accepted) {
    CPI_TRY(lm_sizes_check(ctx, who, C, G, S, F));
    const cpi_lm_params &p = params ? *params : kLmDefaults;
    // every test is written so that a NaN fails it
    if (!(p.lam_down > 0.0 && p.lam_down <= 1.0 && p.lam_up >= 1.0)) return refuse(ctx, who, "params: 0 < lam_down <= 1 <= lam_up is required");
    if (!(p.lam_min >= 0.0 && p.lam_min <= p.lam_max)) return refuse(ctx, who, "params: 0 <= lam_min <= lam_max is required");
    if (!(p.abs_tol >= 0.0 && p.rel_tol >= 0.0)) return refuse(ctx, who, "params: a tolerance is negative or NaN");
    if (C == 0) return CPI_OK;
    if (!cost || !lambda || !phase) return refuse(ctx, who, "cost, lambda or phase is NULL");
    if (S > 0 && (!states || !trial)) return refuse(ctx, who, "states or trial is NULL");
    if (!chi2_new && G > 1) return refuse(ctx, who, "chi2_new is NULL (only chains of one state, G == 1, need none)");
    const size_t d = sizeof(double);
    const Span outs[6] = { { cost, (size_t)C * d, "cost" }, { states, (size_t)S * 16 * d, "states" }, { chi2, (size_t)F * d, "chi2" },
                           { lambda, (size_t)C * d, "lambda" }, { phase, (size_t)C * sizeof(int32_t), "phase" },
                           { accepted, (size_t)C * sizeof(int32_t), "accepted" } };
    const Span ins[6] = { { first, (size_t)C * sizeof(int64_t), "" }, { count, (size_t)C * sizeof(int32_t), "" }, { ffirst, (size_t)C * sizeof(int64_t), "" },
                          { chi2_new, (size_t)F * d, "" }, { pcost_new, (size_t)S * d, "" }, { trial, (size_t)S * 16 * d, "" } };
    return refuse_overlaps(ctx, who, outs, 6, ins, 6);
}
extern "C" int cpi_chain_accept_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                      const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                      const cpi_lm_params *params,
                                      const double *chi2_new, const double *pcost_new, const double *trial,
                                      double *cost, double *states, double *chi2, double *lambda,
                                      int32_t *phase, int32_t *accepted) {
    static const char who[] = "cpi_chain_accept_batch";
    CPI_TRY(lm_accept_check(ctx, who, C, G, S, F, first, count, ffirst, params, chi2_new, pcost_new, trial, cost, states, chi2, lambda, phase, accepted));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    if (!grid_ok((C + 3) / 4)) return refuse(ctx, who, "C exceeds the 32-bit grid (4 chains per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    LmCostArgs a;
    lm_cost_args(a, C, G, S, F, first, count, ffirst, chi2_new, pcost_new, cost);
    LmAcceptArgs b;
    memset(&b, 0, sizeof b);
    b.p = params ? *params : kLmDefaults;
    b.trial = trial; b.states = states; b.chi2 = chi2; b.lambda = lambda; b.phase = phase; b.accepted = accepted;
    launch::lm_accept(a, b, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// cpi_state_fix_batch: absolute measurements of states added to their rows and to their cost (cpi_fix.hip)
// ============================================================================================
static const int kFixZ[4] = { 3, 3, 4, 7 }, kFixR[4] = { 6, 6, 6, 21 };
// what the device and the host forms refuse alike, before the context is looked at
static int fix_check(cpi_ctx *ctx, const char *who, int64_t S, int64_t M, int32_t kind, const int64_t *mfirst, const double *states, const double *z,
                     const double *R, const double *weight, const double *base, const double *pcost_base, double *out, double *pcost, double *chi2) {
    if (S < 0 || M < 0) return refuse(ctx, who, "negative size");
    if (kind < CPI_FIX_POSITION || kind > CPI_FIX_POSE) return refuse(ctx, who, "unknown kind (CPI_FIX_POSITION .. CPI_FIX_POSE)");
    if (!mfirst || !states) return refuse(ctx, who, "mfirst or states is NULL");
    if (M > 0 && (!z || !R)) return refuse(ctx, who, "z or R is NULL with M > 0");
    if (!out && !pcost && !chi2) return refuse(ctx, who, "out, pcost and chi2 are all NULL");
    const size_t d = sizeof(double);
    const Span outs[3] = { { out, (size_t)S * 136 * d, "out" }, { pcost, (size_t)S * d, "pcost" }, { chi2, (size_t)M * d, "chi2" } };
    const Span ins[7] = { { mfirst, (size_t)(S + 1) * sizeof(int64_t), "" }, { states, (size_t)S * 16 * d, "" }, { z, (size_t)M * kFixZ[kind] * d, "" },
                          { R, (size_t)M * kFixR[kind] * d, "" }, { weight, (size_t)M * d, "" }, { base, (size_t)S * 136 * d, "" },
                          { pcost_base, (size_t)S * d, "" } };
    return refuse_overlaps(ctx, who, outs, 3, ins, 7);
}
extern "C" int cpi_state_fix_batch(cpi_ctx *ctx, int64_t S, int64_t M, int32_t kind, const int64_t *mfirst,
                                   const double *states, const double *z, const double *R,
                                   const double *weight, const double *base,
                                   const double *pcost_base, double *out,
                                   double *pcost, double *chi2) {
    static const char who[] = "cpi_state_fix_batch";
    CPI_TRY(fix_check(ctx, who, S, M, kind, mfirst, states, z, R, weight, base, pcost_base, out, pcost, chi2));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (S == 0) return CPI_OK;
    if (!grid_ok((S + 3) / 4)) return refuse(ctx, who, "S exceeds the 32-bit grid (4 states per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    FixArgs a;
    memset(&a, 0, sizeof a);
    a.S = S; a.M = M; a.mfirst = (const long long *)mfirst; a.states = states; a.z = z; a.R = R; a.weight = weight; a.base = base;
    a.pcost_base = pcost_base; a.out = out; a.pcost = pcost; a.chi2 = chi2;
    launch::state_fix(kind, a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// cpi_state_between_batch: measurements between the two states of an IMU factor added to its 31 x 31 row and to its chi2 (cpi_between.hip)
// ============================================================================================
static const int kBetweenZ[3] = { 3, 4, 7 }, kBetweenR[3] = { 6, 6, 21 };
// what the device and the host forms refuse alike, before the context is looked at
static int between_check(cpi_ctx *ctx, const char *who, int64_t F, int64_t M, int32_t kind, const int64_t *mfirst, const double *states, int64_t S,
                         const int32_t *idx_i, const int32_t *idx_j, const double *z, const double *R, const double *weight, const double *hess_base,
                         const double *chi2_base, double *hess, double *chi2, double *chi2_m) {
    if (F < 0 || M < 0 || S < 0) return refuse(ctx, who, "negative size");
    if (kind < CPI_BETWEEN_POSITION || kind > CPI_BETWEEN_POSE) return refuse(ctx, who, "unknown kind (CPI_BETWEEN_POSITION .. CPI_BETWEEN_POSE)");
    if (!mfirst || !states) return refuse(ctx, who, "mfirst or states is NULL");
    if (M > 0 && (!z || !R)) return refuse(ctx, who, "z or R is NULL with M > 0");
    if (!hess && !chi2 && !chi2_m) return refuse(ctx, who, "hess, chi2 and chi2_m are all NULL");
    if (F > 0 && (S < 1 || (!idx_i && S < F) || (!idx_j && S < F + 1)))
        return refuse(ctx, who, "too few states: S >= 1, and >= F + 1 when idx_i / idx_j are NULL (chained states f, f + 1)");
    const size_t d = sizeof(double);
    // hess == hess_base and chi2 == chi2_base exactly are the in-place forms: the base then is no input of its own
    const Span outs[3] = { { hess, (size_t)F * 496 * d, "hess" }, { chi2, (size_t)F * d, "chi2" }, { chi2_m, (size_t)M * d, "chi2_m" } };
    const Span ins[9] = { { mfirst, (size_t)(F + 1) * sizeof(int64_t), "" }, { states, (size_t)S * 16 * d, "" },
                          { idx_i, (size_t)F * sizeof(int32_t), "" }, { idx_j, (size_t)F * sizeof(int32_t), "" },
                          { z, (size_t)M * kBetweenZ[kind] * d, "" }, { R, (size_t)M * kBetweenR[kind] * d, "" }, { weight, (size_t)M * d, "" },
                          { hess_base == hess ? nullptr : hess_base, (size_t)F * 496 * d, "" }, { chi2_base == chi2 ? nullptr : chi2_base, (size_t)F * d, "" } };
    return refuse_overlaps(ctx, who, outs, 3, ins, 9);
}
extern "C" int cpi_state_between_batch(cpi_ctx *ctx, int64_t F, int64_t M, int32_t kind, const int64_t *mfirst,
                                       const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                       const double *z, const double *R, const double *weight,
                                       const double *hess_base, const double *chi2_base,
                                       double *hess, double *chi2, double *chi2_m) {
    static const char who[] = "cpi_state_between_batch";
    CPI_TRY(between_check(ctx, who, F, M, kind, mfirst, states, S, idx_i, idx_j, z, R, weight, hess_base, chi2_base, hess, chi2, chi2_m));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0) return CPI_OK;
    if (!grid_ok((F + 3) / 4)) return refuse(ctx, who, "F exceeds the 32-bit grid (4 factors per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    BetweenArgs a;
    memset(&a, 0, sizeof a);
    a.F = F; a.M = M; a.S = S; a.mfirst = (const long long *)mfirst; a.states = states; a.idx_i = idx_i; a.idx_j = idx_j; a.z = z; a.R = R;
    a.weight = weight; a.hess_base = hess_base; a.chi2_base = chi2_base; a.hess = hess; a.chi2 = chi2; a.chi2_m = chi2_m;
    launch::state_between(kind, a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

extern "C" size_t cpi_outputs_slab_doubles(const cpi_outputs *mask, int64_t Wb) {
    if (!mask || Wb <= 0) return 0;
    size_t n = 0;
    for (int k = 0; k < kOutFields; k++) if (out_field_c(mask, k)) n += (size_t)OUT_N[k] * (size_t)Wb;
    return n;
}
extern "C" int cpi_outputs_bind_slab(const cpi_outputs *mask, int64_t Wb, double *slab, cpi_outputs *bound) {
    if (!mask || !bound || Wb < 0 || (!slab && Wb > 0)) return CPI_ERR_INVALID;
    cpi_outputs b;
    memset(&b, 0, sizeof b);
    size_t off = 0;
    for (int k = 0; k < kOutFields; k++)
        if (out_field_c(mask, k)) { *out_field(&b, k) = slab + off; off += (size_t)OUT_N[k] * (size_t)Wb; }
    *bound = b;
    return CPI_OK;
}

// ============================================================================================
// tiled layout: producers and the mean-only entry
// ============================================================================================
extern "C" int cpi_tile_windows(cpi_ctx *ctx, int64_t W, int32_t N, const double *knots, const int64_t *first,
                                const int32_t *count, double *tiles) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (W < 0 || N < 0) return fail(ctx, CPI_ERR_INVALID, "cpi_tile_windows: negative size");
    if (W == 0) return CPI_OK;
    if (!knots || !tiles) return fail(ctx, CPI_ERR_INVALID, "cpi_tile_windows: NULL argument");
    if (!grid_ok(W)) return fail(ctx, CPI_ERR_INVALID, "cpi_tile_windows: W exceeds 2^31 - 1 windows per call");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    launch::tile_knots((long long)W, (int)N, knots, (const long long *)first, count, tiles, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
extern "C" int cpi_tile_knots(cpi_ctx *ctx, int64_t W, int32_t N, const double *knots, double *tiles) {
    return cpi_tile_windows(ctx, W, N, knots, nullptr, nullptr, tiles);
}
extern "C" int cpi_assemble_tiles(cpi_ctx *ctx, int64_t K, const double *stream, int64_t U, const double *update_times,
                                  int32_t N, double *tiles, int32_t *count) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (K < 0 || U < 0 || N < 0) return fail(ctx, CPI_ERR_INVALID, "cpi_assemble_tiles: negative size");
    if (U == 0) return CPI_OK;
    if (K == 0) return fail(ctx, CPI_ERR_INVALID, "cpi_assemble_tiles: the stream is empty");
    if (!stream || !update_times || !tiles || !count) return fail(ctx, CPI_ERR_INVALID, "cpi_assemble_tiles: NULL argument");
    if (!grid_ok(U)) return fail(ctx, CPI_ERR_INVALID, "cpi_assemble_tiles: U exceeds 2^31 - 1 windows per call");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    AssembleArgs a;
    memset(&a, 0, sizeof a);
    a.K = K; a.stream = stream; a.U = U; a.update = update_times; a.N = N; a.tiles = tiles; a.count = count;
    a.ts = (long long)(N + 1) * 448; a.ss = 448;
    launch::assemble_tiles(a, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
static const char kTiledMeansOnly[] = "the tiled layout serves the mean outputs (DT, alpha, beta, q) only";
extern "C" int cpi_preintegrate_tiled_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *tiles,
                                            const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_tiled_batch";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out) return refuse(ctx, who, "prm/out is NULL");
    if (!model_is_cpi(prm)) return refuse(ctx, who, "model must be 1 or 2");
    if (W < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (W == 0) return CPI_OK;
    if (!tiles || !lin) return refuse(ctx, who, "tiles/lin is NULL");
    CPI_TRY(check_qk(ctx, who, prm, q_k_lin));
    CPI_TRY(check_grid(ctx, who, "W", W));
    const Request rq = request_of(out);
    if (rq.jac || rq.cov) return refuse(ctx, who, kTiledMeansOnly, "; Jacobians and covariance are FP64-bound, not HBM-bound: use cpi_preintegrate_batch");
    if (prm->lanes_per_window < 0 || prm->lanes_per_window > 8)
        return refuse(ctx, who, "lanes_per_window (here: wavefronts per tile) must be 0 (auto) or 1..8");
    if (!rq.mean) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    TiledArgs a;
    memset(&a, 0, sizeof a);
    a.W = W; a.N = N; a.tiles = tiles; a.count = count; a.lin = lin; a.qk = q_k_lin; a.out = *out;
    for (int i = 0; i < 3; i++) a.grav[i] = prm->grav[i];
    a.ts = (long long)(N + 1) * 448; a.ss = 448;
    const long long nb = (W + 63) / 64;
#ifdef CPI_EXPERIMENTS
    a.dbg = expsw::blk_mode();
    if (a.dbg == 1) {   // CPI_AMD_PROBE_LDS = dynamic LDS bytes per wavefront, to pin the probe's occupancy (13312 -> 12 waves / CU)
        launch::tiled_fetch_probe(a, (size_t)expsw::probe_lds(), ctx->stream);
        CPI_HIP(ctx, hipGetLastError());
        return CPI_OK;
    }
#endif
    // wavefronts per tile.  Measured (MI355X, N = 50, us per launch, S = 1 / 2 / 3 / 4 / 8): 5 k windows 24.9 / 15.0 / 11.5 /
    // 10.3 / -, 10 k 25.2 / 15.4 / 11.9 / 10.8 / 12.4, 20 k 27.0 / 23.6 / 19.6 / 18.7 / 22.8, 30 k 28.6 / 25.1 / 22.2 / 21.3,
    // 50 k 33.0 / 34.4 / 34.8 / 34.9, 100 k 61.3 / 64.3 / 65.8 / 65.2: four (one per SIMD of the CU that owns the tile) while
    // the tiles do not fill the chip, one beyond.  prm->lanes_per_window (1..8) overrides the choice.
    int S = (nb < 640) ? std::max(1, std::min(4, (int)N / 4)) : 1;
    if (prm->lanes_per_window > 0) S = prm->lanes_per_window;
    CPI_HIP(ctx, launch::mean_tiled(prm->model, prm->imu_avg != 0, count != nullptr, S, a, ctx->stream, &ctx->big_lds_set));
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}

// ============================================================================================
// device sets
// ============================================================================================
// Windows shard embarrassingly: rank r of n owns the contiguous block cpi_shard_bounds(W, r, n) and runs the ordinary
// entries on its own context; the ONE exchange step is the final gather of the output slabs to a root device.  RCCL is
// bound lazily (dlopen of librccl.so.1 at the first cpi_group_create with n > 1): single-GPU users never load it, and a
// process that already carries an RCCL (PyTorch) shares that copy.  One process drives all devices (ncclCommInitAll,
// rccl/rccl.h:236) -- the reference is a single process too; multi-process hosts (one rank per GPU, torch.distributed)
// use cpi_amd/dist.py, which issues the same send / recv pattern through ProcessGroupNCCL.
// The function-pointer types are decltype's of the prototypes in <rccl/rccl.h> and the datatype is its ncclFloat64, so a
// signature or enum drift is a compile error here, not a silent mismatch behind dlsym.
namespace {
struct Rccl {
    void *h = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string err;
    std::mutex mu;
    bool load() {   // serialised: two host threads may create their first groups at the same time
        std::lock_guard<std::mutex> lock(mu);
        if (h) return true;
        // CPI_AMD_RCCL_LIB: an explicit library path (deployments with several ROCm installs; the test-suite points it at
        // tests/fake_rccl).  Read here, once, at the first n > 1 group -- never on a launch path.
        const char *forced = getenv("CPI_AMD_RCCL_LIB");
        std::string tried;
        if (forced && *forced) {
            h = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
            tried = forced;
        } else {
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (h) break;
            }
            tried = "librccl.so.1";
        }
        if (!h) {
            const char *de = dlerror();   // dlerror() clears its state: call it ONCE
            err = "dlopen(" + tried + "): " + (de ? de : "not found");
            return false;
        }
#define CPI_SYM(field, name) field = reinterpret_cast<decltype(field)>(dlsym(h, name)); \
        if (!field) { err = std::string("dlsym(") + name + "): symbol missing in " + tried; dlclose(h); h = nullptr; return false; }
        CPI_SYM(CommInitAll, "ncclCommInitAll") CPI_SYM(CommDestroy, "ncclCommDestroy") CPI_SYM(GroupStart, "ncclGroupStart")
        CPI_SYM(GroupEnd, "ncclGroupEnd") CPI_SYM(Send, "ncclSend") CPI_SYM(Recv, "ncclRecv") CPI_SYM(GetErrorString, "ncclGetErrorString")
#undef CPI_SYM
        return true;
    }
};
Rccl g_rccl;
constexpr int kMaxGroup = 16;   // ranks of one device set (a node has 8 GPUs)
}  // namespace

struct cpi_group {
    int n = 0;
    std::vector<cpi_ctx *> ctx;
    std::vector<hipStream_t> streams;   // owned
    std::vector<ncclComm_t> comms;      // empty when n == 1
    std::string err;
    // slab path of cpi_group_gather: the peers' slabs land here on the root's device before the unpack kernel places them
    double *staging = nullptr;
    size_t staging_cap = 0;             // doubles
    int staging_dev = -1;
    int last_gather_sends = 0;          // messages per peer of the last gather (1 = slab path); cpi_group_last_gather_messages
    // cpi_group_gather_chunk: a second non-blocking stream per device for the exchange (made at the first use), and one event per
    // device to order it behind / ahead of the compute stream
    std::vector<hipStream_t> xstreams;  // owned; empty until the first chunked gather
    std::vector<hipEvent_t> xev;
};
static thread_local std::string g_group_err;
static int gfail(cpi_group *g, int code, const std::string &msg) { if (g) g->err = msg; else g_group_err = msg; return code; }

extern "C" void cpi_shard_bounds(int64_t W, int rank, int n, int64_t *lo, int64_t *hi) {
    const int64_t per = n > 0 ? (W + n - 1) / n : W;
    const int64_t a = std::min<int64_t>(W, (int64_t)rank * per);
    if (lo) *lo = a;
    if (hi) *hi = std::min<int64_t>(W, a + per);
}
// sub-block `chunk` of `chunks` of rank's block: equal sub-block size on every rank (cper = ceil(ceil(W / n) / chunks))
extern "C" void cpi_shard_chunk_bounds(int64_t W, int rank, int n, int chunk, int chunks, int64_t *lo, int64_t *hi) {
    int64_t a, b;
    cpi_shard_bounds(W, rank, n, &a, &b);
    if (chunks > 1) {
        const int64_t per = n > 0 ? (W + n - 1) / n : W, cper = (per + chunks - 1) / chunks;
        const int64_t ca = std::min<int64_t>(b, a + (int64_t)chunk * cper);
        b = std::min<int64_t>(b, ca + cper);
        a = ca;
    }
    if (lo) *lo = a;
    if (hi) *hi = b;
}
extern "C" const char *cpi_group_last_error(const cpi_group *g) { return g ? g->err.c_str() : g_group_err.c_str(); }
extern "C" int cpi_group_size(const cpi_group *g) { return g ? g->n : 0; }
extern "C" cpi_ctx *cpi_group_ctx(cpi_group *g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->ctx[rank] : nullptr; }
extern "C" int cpi_group_last_gather_messages(const cpi_group *g) { return g ? g->last_gather_sends : 0; }
extern "C" void cpi_group_destroy(cpi_group *g) {
    if (!g) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (int r = 0; r < g->n; r++) {
        if (r < (int)g->comms.size() && g->comms[r] && g_rccl.CommDestroy) g_rccl.CommDestroy(g->comms[r]);
        if (r < (int)g->ctx.size() && g->ctx[r]) {
            (void)hipSetDevice(g->ctx[r]->device);
            if (r < (int)g->xstreams.size() && g->xstreams[r]) (void)hipStreamDestroy(g->xstreams[r]);
            if (r < (int)g->xev.size() && g->xev[r]) (void)hipEventDestroy(g->xev[r]);
            if (r < (int)g->streams.size() && g->streams[r]) (void)hipStreamDestroy(g->streams[r]);
            cpi_ctx_destroy(g->ctx[r]);
        }
    }
    if (g->staging) { (void)hipSetDevice(g->staging_dev); (void)hipFree(g->staging); }
    if (prev >= 0) (void)hipSetDevice(prev);
    delete g;
}
static int group_create(int n, const int *devices, bool shared_device_for_tests, cpi_group **out) {
    if (!out) return gfail(nullptr, CPI_ERR_INVALID, "cpi_group_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return gfail(nullptr, CPI_ERR_NO_DEVICE, "cpi_group_create: no HIP device available (this library has no CPU fallback)");
    if (n <= 0 || n > kMaxGroup || (!shared_device_for_tests && n > ndev))
        return gfail(nullptr, CPI_ERR_INVALID, "cpi_group_create: n must be between 1 and the number of devices");
    std::vector<int> devs(n);
    for (int r = 0; r < n; r++) {
        devs[r] = devices ? devices[r] : r;
        if (devs[r] < 0 || devs[r] >= ndev) return gfail(nullptr, CPI_ERR_INVALID, "cpi_group_create: device index out of range");
        if (!shared_device_for_tests)
            for (int q = 0; q < r; q++) if (devs[q] == devs[r]) return gfail(nullptr, CPI_ERR_INVALID, "cpi_group_create: duplicate device");
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    cpi_group *g = new cpi_group();
    g->n = n;
    g->ctx.assign(n, nullptr); g->streams.assign(n, nullptr);
    for (int r = 0; r < n; r++) {
        hipError_t e = hipSetDevice(devs[r]);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->streams[r], hipStreamNonBlocking);
        if (e != hipSuccess || cpi_ctx_create(devs[r], g->streams[r], &g->ctx[r]) != CPI_OK) {
            const std::string msg = std::string("cpi_group_create: device ") + std::to_string(devs[r]) + ": " + (e != hipSuccess ? hipGetErrorString(e) : cpi_last_error(nullptr));
            cpi_group_destroy(g);
            if (prev >= 0) (void)hipSetDevice(prev);
            return gfail(nullptr, CPI_ERR_HIP, msg);
        }
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    if (n > 1) {
        if (!g_rccl.load()) { const std::string m = "cpi_group_create: " + g_rccl.err; cpi_group_destroy(g); return gfail(nullptr, CPI_ERR_RCCL, m); }
        g->comms.assign(n, nullptr);
        const ncclResult_t rc = g_rccl.CommInitAll(g->comms.data(), n, devs.data());
        if (rc != ncclSuccess) { const std::string m = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(rc); cpi_group_destroy(g); return gfail(nullptr, CPI_ERR_RCCL, m); }
    }
    *out = g;
    return CPI_OK;
}
extern "C" int cpi_group_create(int n, const int *devices, cpi_group **out) { return group_create(n, devices, false, out); }
#ifdef CPI_TEST_HOOKS
// include/cpi_amd_test.h: n ranks that all live on ONE device -- the n > 1 code paths of the device set on a 1-GPU box.
// Real RCCL refuses duplicate devices in ncclCommInitAll; the test-suite binds tests/fake_rccl through CPI_AMD_RCCL_LIB.
// Not in the product library: the entry switches the duplicate-device guard of cpi_group_create off.
extern "C" int cpi_test_group_create_shared(int n, int device, cpi_group **out) {
    if (n <= 0 || n > kMaxGroup) return gfail(nullptr, CPI_ERR_INVALID, "cpi_test_group_create_shared: n out of range");
    std::vector<int> devs(n, device);
    return group_create(n, devs.data(), true, out);
}
#endif
extern "C" int cpi_group_synchronize(cpi_group *g) {
    if (!g) return gfail(nullptr, CPI_ERR_INVALID, "group is NULL");
    for (int r = 0; r < g->n; r++) {
        const int rc = cpi_ctx_synchronize(g->ctx[r]);
        if (rc != CPI_OK) return gfail(g, rc, cpi_last_error(g->ctx[r]));
    }
    if (!g->xstreams.empty()) {   // a chunked exchange that was not joined yet (cpi_group_gather_chunk)
        int prev = -1;
        (void)hipGetDevice(&prev);
        hipError_t e = hipSuccess;
        for (int r = 0; r < g->n && e == hipSuccess; r++) {
            e = hipSetDevice(g->ctx[r]->device);
            if (e == hipSuccess) e = hipStreamSynchronize(g->xstreams[r]);
        }
        if (prev >= 0) (void)hipSetDevice(prev);
        if (e != hipSuccess) return gfail(g, CPI_ERR_HIP, std::string("cpi_group_synchronize (exchange streams): ") + hipGetErrorString(e));
    }
    return CPI_OK;
}

// Is rank r's local output set ONE slab -- the wanted fields back to back, field-major over wb >= cnt windows
// (cpi_outputs_bind_slab)?  Returns its base, wb and the doubles to send (the last field only up to cnt windows).
static bool slab_of(const cpi_outputs &loc, const cpi_outputs &want, long long cnt, const double *&base, long long &wb, size_t &len) {
    int ks[kOutFields], nk = 0;
    for (int k = 0; k < kOutFields; k++) if (out_field_c(&want, k)) ks[nk++] = k;
    if (nk == 0) return false;
    const double *p0 = out_field_c(&loc, ks[0]);
    if (!p0) return false;
    wb = cnt;
    if (nk > 1) {
        const double *p1 = out_field_c(&loc, ks[1]);
        if (!p1 || p1 <= p0) return false;
        const long long d = (long long)(p1 - p0);
        if (d % OUT_N[ks[0]] != 0) return false;
        wb = d / OUT_N[ks[0]];
        if (wb < cnt) return false;
    }
    size_t off = 0;
    for (int i = 0; i < nk; i++) {
        if (out_field_c(&loc, ks[i]) != p0 + off) return false;
        if (i + 1 < nk) off += (size_t)OUT_N[ks[i]] * (size_t)wb;
    }
    base = p0;
    len = off + (size_t)OUT_N[ks[nk - 1]] * (size_t)cnt;
    return true;
}

// chunk < 0: the whole blocks, on the ranks' compute streams (cpi_group_gather).  chunk >= 0: sub-block `chunk` of `chunks` of every
// block, on the exchange streams, ordered behind the compute streams' position at this call; the last chunk joins
// (cpi_group_gather_chunk).
static int gather_impl(cpi_group *g, int root, int64_t W, int chunk, int chunks, const cpi_outputs *local, const cpi_outputs *root_out) {
    if (!g) return gfail(nullptr, CPI_ERR_INVALID, "group is NULL");
    if (root < 0 || root >= g->n || W < 0 || !local || !root_out) return gfail(g, CPI_ERR_INVALID, "cpi_group_gather: invalid argument");
    const bool chunked = chunk >= 0;
    if (chunked && (chunks < 1 || chunk >= chunks)) return gfail(g, CPI_ERR_INVALID, "cpi_group_gather_chunk: chunk must lie in [0, chunks)");
    int prev = -1;
    (void)hipGetDevice(&prev);
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore_{prev};
    const int n = g->n;
    if (chunked && g->xstreams.empty()) {
        g->xstreams.assign(n, nullptr); g->xev.assign(n, nullptr);
        for (int r = 0; r < n; r++)
            if (hipSetDevice(g->ctx[r]->device) != hipSuccess || hipStreamCreateWithFlags(&g->xstreams[r], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&g->xev[r], hipEventDisableTiming) != hipSuccess)
                return gfail(g, CPI_ERR_HIP, "cpi_group_gather_chunk: creating the exchange streams failed");
    }
    auto stream_of = [&](int r) { return chunked ? g->xstreams[r] : g->ctx[r]->stream; };
    if (chunked) {   // the exchange of this sub-block starts where the compute streams stand NOW
        for (int r = 0; r < n; r++)
            if (hipSetDevice(g->ctx[r]->device) != hipSuccess || hipEventRecord(g->xev[r], g->ctx[r]->stream) != hipSuccess ||
                hipStreamWaitEvent(g->xstreams[r], g->xev[r], 0) != hipSuccess)
                return gfail(g, CPI_ERR_HIP, "cpi_group_gather_chunk: ordering the exchange stream behind the compute stream failed");
    }
    long long lo[kMaxGroup], cnt[kMaxGroup], wb[kMaxGroup];
    const double *base[kMaxGroup];
    size_t len[kMaxGroup], stride = 0;
    bool any_field = false;
    for (int k = 0; k < kOutFields; k++) any_field = any_field || out_field_c(root_out, k);
    if (!any_field) return CPI_OK;
    // every wanted field must exist in every non-empty block
    bool slabs = n > 1;
    for (int r = 0; r < n; r++) {
        int64_t a, b;
        if (chunked) cpi_shard_chunk_bounds(W, r, n, chunk, chunks, &a, &b); else cpi_shard_bounds(W, r, n, &a, &b);
        lo[r] = a; cnt[r] = b - a; wb[r] = 0; base[r] = nullptr; len[r] = 0;
        if (cnt[r] == 0) continue;
        for (int k = 0; k < kOutFields; k++)
            if (out_field_c(root_out, k) && !out_field_c(&local[r], k))
                return gfail(g, CPI_ERR_INVALID, "cpi_group_gather: a field wanted at the root is NULL in a rank's local outputs");
        if (r == root) continue;
        if (slabs && slab_of(local[r], *root_out, cnt[r], base[r], wb[r], len[r])) stride = std::max(stride, len[r]);
        else slabs = false;
    }
    hipStream_t rs = stream_of(root);
    // the slab path needs staging for n slabs on the root's device (grow-only; a re-allocation waits for the root's stream)
    if (slabs && stride > 0) {
        stride = (stride + 1) & ~(size_t)1;   // 16-byte aligned slabs
        if (g->staging_cap < stride * (size_t)n || g->staging_dev != g->ctx[root]->device) {
            if (g->staging) {
                if (hipSetDevice(g->staging_dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipFree(g->staging) != hipSuccess)
                    return gfail(g, CPI_ERR_HIP, "cpi_group_gather: releasing the staging buffer failed");
                g->staging = nullptr; g->staging_cap = 0;
            }
            if (hipSetDevice(g->ctx[root]->device) != hipSuccess || hipMalloc((void **)&g->staging, stride * (size_t)n * sizeof(double)) != hipSuccess)
                return gfail(g, CPI_ERR_HIP, "cpi_group_gather: allocating the root's staging buffer failed");
            g->staging_cap = stride * (size_t)n; g->staging_dev = g->ctx[root]->device;
        }
    }
    ncclResult_t rc = ncclSuccess;
    int hip_bad = 0, msgs = 0;
    if (n > 1) { rc = g_rccl.GroupStart(); if (rc != ncclSuccess) return gfail(g, CPI_ERR_RCCL, std::string("ncclGroupStart: ") + g_rccl.GetErrorString(rc)); }
    // the root's own block: device-to-device copies on its stream (unless it was computed in place)
    if (cnt[root] > 0) {
        for (int k = 0; k < kOutFields && !hip_bad; k++) {
            double *dst = out_field_c(root_out, k);
            if (!dst) continue;
            const double *src = out_field_c(&local[root], k);
            if (src != dst + (size_t)lo[root] * OUT_N[k]) {
                if (hipSetDevice(g->ctx[root]->device) != hipSuccess ||
                    hipMemcpyAsync(dst + (size_t)lo[root] * OUT_N[k], src, (size_t)cnt[root] * OUT_N[k] * sizeof(double), hipMemcpyDeviceToDevice, rs) != hipSuccess) hip_bad = 1;
            }
        }
    }
    // every peer sends straight to the root: one xGMI link per peer, no ring
    for (int r = 0; r < n && rc == ncclSuccess && !hip_bad; r++) {
        if (r == root || cnt[r] == 0) continue;
        if (slabs) {   // ONE message per peer: its whole slab into the root's staging area
            rc = g_rccl.Recv(g->staging + (size_t)r * stride, len[r], ncclFloat64, r, g->comms[root], rs);
            if (rc == ncclSuccess) rc = g_rccl.Send(base[r], len[r], ncclFloat64, root, g->comms[r], stream_of(r));
            msgs = 1;
        } else {       // separately allocated fields: one message per (peer, field), received in place
            int m = 0;
            for (int k = 0; k < kOutFields && rc == ncclSuccess; k++) {
                double *dst = out_field_c(root_out, k);
                if (!dst) continue;
                const size_t c = (size_t)cnt[r] * (size_t)OUT_N[k];
                rc = g_rccl.Recv(dst + (size_t)lo[r] * OUT_N[k], c, ncclFloat64, r, g->comms[root], rs);
                if (rc == ncclSuccess) rc = g_rccl.Send(out_field_c(&local[r], k), c, ncclFloat64, root, g->comms[r], stream_of(r));
                m++;
            }
            msgs = std::max(msgs, m);
        }
    }
    ncclResult_t rce = ncclSuccess;
    if (n > 1) rce = g_rccl.GroupEnd();
    if (hip_bad) return gfail(g, CPI_ERR_HIP, "cpi_group_gather: device-to-device copy of the root's own block failed");
    if (rc != ncclSuccess) return gfail(g, CPI_ERR_RCCL, std::string("ncclSend/ncclRecv: ") + g_rccl.GetErrorString(rc));
    if (rce != ncclSuccess) return gfail(g, CPI_ERR_RCCL, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(rce));
    if (slabs && msgs) {   // place the staged slabs: one launch on the root's stream, behind the receives
        long long c2[kMaxGroup];
        for (int r = 0; r < n; r++) c2[r] = (r == root) ? 0 : cnt[r];
        if (hipSetDevice(g->ctx[root]->device) != hipSuccess) return gfail(g, CPI_ERR_HIP, "cpi_group_gather: hipSetDevice(root) failed");
        launch::unpack_slabs(n, lo, c2, wb, g->staging, (long long)stride, *root_out, rs);
        if (hipGetLastError() != hipSuccess) return gfail(g, CPI_ERR_HIP, "cpi_group_gather: the unpack launch failed");
    }
    g->last_gather_sends = msgs;
    if (chunked && chunk == chunks - 1) {   // join: whatever is enqueued on the contexts from here on waits for the whole exchange
        for (int r = 0; r < n; r++)
            if (hipSetDevice(g->ctx[r]->device) != hipSuccess || hipEventRecord(g->xev[r], g->xstreams[r]) != hipSuccess ||
                hipStreamWaitEvent(g->ctx[r]->stream, g->xev[r], 0) != hipSuccess)
                return gfail(g, CPI_ERR_HIP, "cpi_group_gather_chunk: joining the exchange streams failed");
    }
    return CPI_OK;
}
extern "C" int cpi_group_gather(cpi_group *g, int root, int64_t W, const cpi_outputs *local, const cpi_outputs *root_out) {
    return gather_impl(g, root, W, -1, 1, local, root_out);
}
extern "C" int cpi_group_gather_chunk(cpi_group *g, int root, int64_t W, int chunk, int chunks, const cpi_outputs *local_chunk,
                                      const cpi_outputs *root_out) {
    return gather_impl(g, root, W, chunk, chunks, local_chunk, root_out);
}

// -------------------------------------------------------------------------------- test hook (include/cpi_amd_test.h)
#ifdef CPI_TEST_HOOKS
extern "C" int cpi_test_quat_ops(cpi_ctx *ctx, int32_t op, int64_t n, const double *in, double *out) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (op < 0 || op > 5 || n < 0) return fail(ctx, CPI_ERR_INVALID, "cpi_test_quat_ops: unknown op / negative size");
    if (n == 0) return CPI_OK;
    if (!in || !out) return fail(ctx, CPI_ERR_INVALID, "cpi_test_quat_ops: NULL argument");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    launch::test_quat_ops((int)op, (long long)n, in, out, ctx->stream);
    CPI_HIP(ctx, hipGetLastError());
    return CPI_OK;
}
#endif

// ============================================================================================
// host-pointer variants
// ============================================================================================
// Whole-batch staging, shared by every host-pointer entry that stages its arrays whole (one-off calls): device copies of the
// caller's arrays and a device mirror of its cpi_outputs, all on the context's stream, all released when the entry returns.
// Nothing returns while a copy is in flight: every way out of an entry -- a failed allocation, a refused device call, a
// failed copy -- runs the destructor, which drains the stream before the buffers go and the caller sees its memory again.
namespace {
class Staging {
public:
    explicit Staging(cpi_ctx *c) : ctx(c) {}
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() {
        if (in_flight) (void)hipStreamSynchronize(ctx->stream);
        for (int i = 0; i < n; i++) (void)hipFree(buf[i]);
    }
    int alloc(size_t bytes, void **dev) {
        if (n == kMax) return fail(ctx, CPI_ERR_INVALID, "host staging: too many arrays");
        CPI_HIP(ctx, hipMalloc(dev, bytes));
        buf[n++] = *dev;
        return CPI_OK;
    }
    template <class T> int alloc(size_t count, T **dev) { return alloc(count * sizeof(T), reinterpret_cast<void **>(dev)); }
    // device copy of host[count]; a NULL host array stays NULL
    template <class T> int upload(const T *host, size_t count, const T **dev) {
        *dev = nullptr;
        if (!host) return CPI_OK;
        T *d;
        CPI_TRY(alloc(count, &d));
        in_flight = true;
        CPI_HIP(ctx, hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        *dev = d;
        return CPI_OK;
    }
    // dev: the fields of mask, each with room for `rows` rows.  rows == 0: the mask itself -- the device entry classifies the
    // request by which fields are set and dereferences none of them
    int mirror(const cpi_outputs *mask, size_t rows, cpi_outputs *dev) {
        *dev = *mask;
        for (int k = 0; k < kOutFields && rows; k++)
            if (*out_field(dev, k)) CPI_TRY(alloc(rows * OUT_N[k], out_field(dev, k)));
        return CPI_OK;
    }
    template <class T> int download(T *host, const T *dev, size_t count) {
        in_flight = true;
        CPI_HIP(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return CPI_OK;
    }
    // rows [row0, row0 + rows) of the caller's fields from the first `rows` rows of the mirror
    int download(const cpi_outputs *host, const cpi_outputs &dev, size_t rows, size_t row0 = 0) {
        for (int k = 0; k < kOutFields && rows; k++)
            if (double *h = out_field_c(host, k)) CPI_TRY(download(h + row0 * OUT_N[k], (const double *)out_field_c(&dev, k), rows * OUT_N[k]));
        return CPI_OK;
    }
    // the end of a call that succeeded so far: the caller's memory holds the results when this returns CPI_OK
    int finish() {
        in_flight = false;
        CPI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CPI_OK;
    }

private:
    // the most any entry stages is cpi_query_open_batch_host's: the 5 window arrays, qwin and qtime, carry_in, carry_out and the
    // record the base-row call leaves, its all-zero counts, and mirrors of the running rows, of the base rows and of the outputs,
    // each of at most kOutFields arrays (cpi_query_stream_batch_host: 10 arrays and two mirrors)
    static constexpr int kMax = 11 + 3 * kOutFields;
    cpi_ctx *ctx;
    void *buf[kMax];
    int n = 0;
    bool in_flight = false;
};

// the window arrays of a batch, staged whole
struct WindowsDev {
    const double *knots, *lin, *qk;
    const int64_t *first;
    const int32_t *count;
};
int stage_windows(Staging &st, int64_t W, int64_t n_knots, const double *knots, const int64_t *first, const int32_t *count,
                  const double *lin, const double *q_k_lin, WindowsDev *d) {
    CPI_TRY(st.upload(knots, (size_t)n_knots * 7, &d->knots));
    CPI_TRY(st.upload(first, (size_t)W, &d->first));
    CPI_TRY(st.upload(count, (size_t)W, &d->count));
    CPI_TRY(st.upload(lin, (size_t)W * 6, &d->lin));
    return st.upload(q_k_lin, (size_t)W * 4, &d->qk);
}

// the operands of a factor sweep, staged whole: the measurement (every field but P / P_sym), the linearisation points, the states and
// the state indices
struct FactorsDev {
    cpi_outputs meas;
    const double *lin, *qk, *states;
    const int32_t *idx_i, *idx_j;
};
int stage_factors(Staging &st, int64_t F, int64_t S, const cpi_outputs *meas, const double *lin, const double *q_k_lin, const double *states,
                  const int32_t *idx_i, const int32_t *idx_j, FactorsDev *d) {
    memset(&d->meas, 0, sizeof d->meas);
    for (int k = 0; k < 11; k++) {
        const double *dm;
        CPI_TRY(st.upload((const double *)out_field_c(meas, k), (size_t)F * OUT_N[k], &dm));
        *out_field(&d->meas, k) = const_cast<double *>(dm);
    }
    CPI_TRY(st.upload(lin, (size_t)F * 6, &d->lin));
    CPI_TRY(st.upload(q_k_lin, (size_t)F * 4, &d->qk));
    CPI_TRY(st.upload(states, (size_t)S * 16, &d->states));
    CPI_TRY(st.upload(idx_i, (size_t)F, &d->idx_i));
    return st.upload(idx_j, (size_t)F, &d->idx_j);
}

// the chains of a solve, staged whole, and the workspace the solve leaves its factorisation in
struct ChainsDev {
    const int64_t *first, *ffirst;
    const int32_t *count;
    const double *hess, *prior;
    double *workspace;
};
int stage_chains(Staging &st, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count, const int64_t *ffirst,
                 const double *hess, const double *prior, ChainsDev *d, bool workspace = true) {
    CPI_TRY(st.upload(first, (size_t)C, &d->first));
    CPI_TRY(st.upload(count, (size_t)C, &d->count));
    CPI_TRY(st.upload(ffirst, (size_t)C, &d->ffirst));
    CPI_TRY(st.upload(F > 0 ? hess : nullptr, (size_t)F * 496, &d->hess));
    CPI_TRY(st.upload(S > 0 ? prior : nullptr, (size_t)S * 136, &d->prior));
    d->workspace = nullptr;
    if (workspace) CPI_TRY(st.alloc(cpi_chain_solve_workspace_doubles(S), &d->workspace));   // cpi_chain_marginalize_batch has none
    if (!d->hess && G > 1) {   // F == 0: no chain has a factor (the ranges are validated), and the device form wants a pointer it never reads
        double *none;
        CPI_TRY(st.alloc((size_t)1, &none));
        d->hess = none;
    }
    return CPI_OK;
}
}  // namespace

// Host pointers: the state indices of a factor sweep and the state and factor ranges of every chain can be (and are) validated; the
// device-pointer entries clamp them, or refuse them per chain, instead.
static int check_state_indices(cpi_ctx *ctx, const char *who, int64_t F, int64_t S, const int32_t *idx_i, const int32_t *idx_j) {
    if (S <= 0 || (!idx_i && S < F) || (!idx_j && S < F + 1)) return refuse(ctx, who, "too few states");
    for (int64_t f = 0; f < F; f++)
        if ((idx_i && (idx_i[f] < 0 || idx_i[f] >= S)) || (idx_j && (idx_j[f] < 0 || idx_j[f] >= S)))
            return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": state index out of range at factor " + std::to_string(f));
    return CPI_OK;
}
static int chain_ranges_check(cpi_ctx *ctx, const char *who, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first,
                              const int32_t *count, const int64_t *ffirst) {
    for (int64_t c = 0; c < C; c++) {
        const int64_t f = first ? first[c] : c * G;
        int64_t n = count ? count[c] : G;
        n = n < 0 ? 0 : (n > G ? G : n);
        if (f < 0 || f > S || n > S - f)
            return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": the states of chain " + std::to_string(c) + " leave [0, S)");
        const int64_t ff = ffirst ? ffirst[c] : f - c;
        if (n > 1 && (ff < 0 || ff > F - (n - 1)))
            return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": the factor rows of chain " + std::to_string(c) + " leave [0, F)");
    }
    return CPI_OK;
}

// Dense (and tiled) batches from host memory run as a three-stage pipeline over chunks of <= 65536 windows: upload of
// chunk i + 1 (copy stream), kernels of chunk i (the context's stream), download of chunk i - 1 (second copy stream) -- PCIe
// is full duplex, so with PINNED host buffers (cpi_host_alloc, hipHostMalloc, torch pin_memory) a call costs about
// max(upload, download, kernels) instead of their sum; with pageable memory the copies serialise in the runtime's own
// staging and the pipeline degenerates to the sum, minus the per-call hipMalloc / hipFree of the device staging, which
// the context now keeps (two slots, grow-only, released by cpi_ctx_destroy).  Measured (MI355X box, 1 M x 50, everything
// out = "V1 full", 2.9 GB up + 2.3 GB down): pinned 56 ms (92 GB/s both directions summed), pageable 112 ms; mean only
// 52 / 56 ms.  Page-locked bounce buffers + copy threads for pageable destinations were built and measured: no faster
// than the runtime's own path (112 ms) -- what costs is FRESH pageable output memory (first-touch page faults: 375-450 ms
// for the same call), so callers should re-use their output buffers.
constexpr int kPipeArrays = 11;   // per-window arrays of a chunk: knots, count, lin, q_k_lin and two of the caller's (the carry records);
                                  // cpi_merge_batch_host: the ten operand fields a request can read and count
// One per-window array that travels with a chunk: `stride` bytes per window, uploaded from `up` before the chunk's kernels or
// downloaded to `down` after them (both NULL: absent); whole groups of `group` windows are copied (64: tiles).
struct PipeArray {
    const char *name;
    const void *up;
    void *down;
    size_t stride;
    int group;
};
struct PipeArrays { PipeArray a[kPipeArrays]; };
// knots[W][N+1][7] (group 1) or tiles[ceil(W/64)][N+1][7][64] (group 64: chunks are whole tiles) with count, lin and q_k_lin
static PipeArrays pipe_windows(const double *knots, int32_t N, int group, const int32_t *count, const double *lin, const double *q_k_lin) {
    PipeArrays p = {};
    p.a[0] = {"knots", knots, nullptr, (size_t)(N + 1) * 7 * sizeof(double), group};
    p.a[1] = {"count", count, nullptr, sizeof(int32_t), 1};
    p.a[2] = {"lin", lin, nullptr, 6 * sizeof(double), 1};
    p.a[3] = {"q_k_lin", q_k_lin, nullptr, 4 * sizeof(double), 1};
    return p;
}
struct HostPipe {
    hipStream_t up = nullptr, down = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    void *arr[2][kPipeArrays] = {};
    size_t arr_cap[2][kPipeArrays] = {};
    void *out[2][kOutFields] = {};
    size_t out_cap[2][kOutFields] = {};
};
static void host_pipe_destroy(HostPipe *hp) {
    if (!hp) return;
    for (int s = 0; s < 2; s++) {
        for (int k = 0; k < kPipeArrays; k++) if (hp->arr[s][k]) (void)hipFree(hp->arr[s][k]);
        for (int k = 0; k < kOutFields; k++) if (hp->out[s][k]) (void)hipFree(hp->out[s][k]);
        if (hp->ev_in[s]) (void)hipEventDestroy(hp->ev_in[s]);
        if (hp->ev_done[s]) (void)hipEventDestroy(hp->ev_done[s]);
        if (hp->ev_out[s]) (void)hipEventDestroy(hp->ev_out[s]);
    }
    if (hp->up) (void)hipStreamDestroy(hp->up);
    if (hp->down) (void)hipStreamDestroy(hp->down);
    delete hp;
}
static int host_pipe_get(cpi_ctx *ctx) {
    if (ctx->pipe) return CPI_OK;
    HostPipe *hp = new HostPipe();
    ctx->pipe = hp;   // owned by the context from here on: a partial set-up is released by cpi_ctx_destroy
    CPI_HIP(ctx, hipStreamCreateWithFlags(&hp->up, hipStreamNonBlocking));
    CPI_HIP(ctx, hipStreamCreateWithFlags(&hp->down, hipStreamNonBlocking));
    for (int s = 0; s < 2; s++) {
        CPI_HIP(ctx, hipEventCreateWithFlags(&hp->ev_in[s], hipEventDisableTiming));
        CPI_HIP(ctx, hipEventCreateWithFlags(&hp->ev_done[s], hipEventDisableTiming));
        CPI_HIP(ctx, hipEventCreateWithFlags(&hp->ev_out[s], hipEventDisableTiming));
    }
    return CPI_OK;
}
static int host_pipe_reserve(cpi_ctx *ctx, void *&p, size_t &cap, size_t bytes) {
    if (bytes <= cap) return CPI_OK;
    if (p) { CPI_HIP(ctx, hipFree(p)); p = nullptr; cap = 0; }
    CPI_HIP(ctx, hipMalloc(&p, bytes));
    cap = bytes;
    return CPI_OK;
}
extern "C" void *cpi_host_alloc(size_t bytes) {
    void *p = nullptr;
    return (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess) ? p : nullptr;
}
extern "C" void cpi_host_free(void *p) { if (p) (void)hipHostFree(p); }

// who: the _host entry that is called.  rows: output rows per window (the running entries: N >= 1 rows, chunks of <= 65536 ROWS).
// launch(wn, dev, d): the device-pointer entry on the wn windows of one chunk -- dev[k] the device copy of arr.a[k] (NULL:
// absent), d the device mirror of out -- enqueued on the context's stream.
template <class Launch>
static int preintegrate_host_pipeline(cpi_ctx *ctx, const char *who, int64_t W, size_t rows, const PipeArrays &arr, const cpi_outputs *out,
                                      Launch launch) {
    int rc = host_pipe_get(ctx);
    if (rc != CPI_OK) return rc;
    HostPipe *hp = ctx->pipe;
    const int64_t cw = std::max<int64_t>(64, 65536 / (int64_t)rows / 64 * 64);
    const int64_t nch = (W + cw - 1) / cw;
    const int64_t Wc = std::min<int64_t>(W, (((W + nch - 1) / nch) + 63) / 64 * 64);   // balanced chunks, whole wavefronts / tiles
    const int nslots = nch > 1 ? 2 : 1;
    auto bytes_of = [](const PipeArray &p, int64_t wn) { return (size_t)((wn + p.group - 1) / p.group * p.group) * p.stride; };
    for (int s = 0; s < nslots; s++) {
        for (int k = 0; k < kPipeArrays; k++)
            if ((arr.a[k].up || arr.a[k].down) && (rc = host_pipe_reserve(ctx, hp->arr[s][k], hp->arr_cap[s][k], bytes_of(arr.a[k], Wc))) != CPI_OK) return rc;
        for (int k = 0; k < kOutFields; k++)
            if (out_field_c(out, k) && (rc = host_pipe_reserve(ctx, hp->out[s][k], hp->out_cap[s][k], (size_t)Wc * rows * OUT_N[k] * sizeof(double))) != CPI_OK) return rc;
    }
    // after the first enqueue nothing may return before the three streams are idle: copies into the caller's memory are in flight
    std::string err;
    auto hip_ok = [&](hipError_t e, const char *what, const char *name = "") { if (e != hipSuccess && err.empty()) err = std::string(what) + name + ": " + hipGetErrorString(e); return e == hipSuccess; };
    for (int64_t i = 0; i < nch && err.empty() && rc == CPI_OK; i++) {
        const int s = (int)(i & 1);
        const int64_t w0 = i * Wc, wn = std::min<int64_t>(Wc, W - w0);
        if (i >= 2 && !hip_ok(hipStreamWaitEvent(hp->up, hp->ev_done[s], 0), "hipStreamWaitEvent")) break;   // slot's inputs consumed
        void *dev[kPipeArrays];
        for (int k = 0; k < kPipeArrays; k++) {
            const PipeArray &p = arr.a[k];
            dev[k] = (p.up || p.down) ? hp->arr[s][k] : nullptr;
            if (p.up && !hip_ok(hipMemcpyAsync(dev[k], (const char *)p.up + (size_t)w0 * p.stride, bytes_of(p, wn), hipMemcpyHostToDevice, hp->up), "upload ", p.name)) break;
        }
        if (!err.empty()) break;
        if (!hip_ok(hipEventRecord(hp->ev_in[s], hp->up), "hipEventRecord")) break;
        if (!hip_ok(hipStreamWaitEvent(ctx->stream, hp->ev_in[s], 0), "hipStreamWaitEvent")) break;
        if (i >= 2 && !hip_ok(hipStreamWaitEvent(ctx->stream, hp->ev_out[s], 0), "hipStreamWaitEvent")) break;   // slot's outputs downloaded
        cpi_outputs d;
        memset(&d, 0, sizeof d);
        for (int k = 0; k < kOutFields; k++) if (out_field_c(out, k)) *out_field(&d, k) = (double *)hp->out[s][k];
        rc = launch(wn, dev, &d);
        if (rc != CPI_OK) break;
        if (!hip_ok(hipEventRecord(hp->ev_done[s], ctx->stream), "hipEventRecord")) break;
        if (!hip_ok(hipStreamWaitEvent(hp->down, hp->ev_done[s], 0), "hipStreamWaitEvent")) break;
        for (int k = 0; k < kOutFields; k++)
            if (out_field_c(out, k) && !hip_ok(hipMemcpyAsync(out_field_c(out, k) + (size_t)w0 * rows * OUT_N[k], hp->out[s][k], (size_t)wn * rows * OUT_N[k] * sizeof(double),
                                                              hipMemcpyDeviceToHost, hp->down), "download")) break;
        for (int k = 0; k < kPipeArrays && err.empty(); k++)
            if (arr.a[k].down) hip_ok(hipMemcpyAsync((char *)arr.a[k].down + (size_t)w0 * arr.a[k].stride, dev[k], bytes_of(arr.a[k], wn), hipMemcpyDeviceToHost, hp->down), "download ", arr.a[k].name);
        if (!err.empty()) break;
        if (!hip_ok(hipEventRecord(hp->ev_out[s], hp->down), "hipEventRecord")) break;
    }
    const hipError_t e1 = hipStreamSynchronize(hp->up), e2 = hipStreamSynchronize(ctx->stream), e3 = hipStreamSynchronize(hp->down);
    if (rc != CPI_OK) return rc;   // message already set by the device-pointer entry
    hip_ok(e1, "hipStreamSynchronize(upload)"); hip_ok(e2, "hipStreamSynchronize"); hip_ok(e3, "hipStreamSynchronize(download)");
    if (!err.empty()) return fail(ctx, CPI_ERR_HIP, std::string(who) + ": " + err);
    return CPI_OK;
}

extern "C" int cpi_preintegrate_tiled_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *tiles,
                                                 const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_tiled_batch_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out || !tiles || !lin) return refuse(ctx, who, "NULL argument");
    if (W <= 0) return W == 0 ? CPI_OK : fail(ctx, CPI_ERR_INVALID, "negative size");
    if (N < 0) return fail(ctx, CPI_ERR_INVALID, "negative size");
    if (request_of(out).jac || request_of(out).cov) return refuse(ctx, who, kTiledMeansOnly);
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    return preintegrate_host_pipeline(ctx, who, W, 1, pipe_windows(tiles, N, 64, count, lin, q_k_lin), out,
                                      [&](int64_t wn, void *const *dev, const cpi_outputs *d) {
                                          return cpi_preintegrate_tiled_batch(ctx, prm, wn, N, (const double *)dev[0], (const int32_t *)dev[1],
                                                                              (const double *)dev[2], (const double *)dev[3], d);
                                      });
}

extern "C" int cpi_preintegrate_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                           const double *knots, const int64_t *first, const int32_t *count,
                                           int64_t n_knots, const double *lin, const double *q_k_lin,
                                           const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_batch_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out || !knots || !lin) return refuse(ctx, who, "NULL argument");
    if (W <= 0) return W == 0 ? CPI_OK : fail(ctx, CPI_ERR_INVALID, "negative size");
    if (N < 0) return fail(ctx, CPI_ERR_INVALID, "negative size");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    if (!first)
        return preintegrate_host_pipeline(ctx, who, W, 1, pipe_windows(knots, N, 1, count, lin, q_k_lin), out,
                                          [&](int64_t wn, void *const *dev, const cpi_outputs *d) {
                                              return cpi_preintegrate_batch(ctx, prm, wn, N, (const double *)dev[0], nullptr, (const int32_t *)dev[1],
                                                                            (const double *)dev[2], (const double *)dev[3], d);
                                          });
    // ragged windows share one knot stream: staged whole (one-off calls; the stream is usually small)
    Staging st(ctx);
    WindowsDev in;
    cpi_outputs d;
    CPI_TRY(stage_windows(st, W, n_knots, knots, first, count, lin, q_k_lin, &in));
    CPI_TRY(st.mirror(out, (size_t)W, &d));
    CPI_TRY(cpi_preintegrate_batch(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, &d));
    CPI_TRY(st.download(out, d, (size_t)W));
    return st.finish();
}

// cpi_preintegrate_running_host / cpi_running_stj_batch_host: one body over the device entry of the same family
typedef int (*RunningEntry)(cpi_ctx *, const cpi_params *, int64_t, int32_t, const double *, const int64_t *, const int32_t *, const double *,
                            const double *, const cpi_outputs *);
static int running_host(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, int64_t W, int32_t N,
                        const double *knots, const int64_t *first, const int32_t *count,
                        int64_t n_knots, const double *lin, const double *q_k_lin,
                        const cpi_outputs *rows) {
    const RunningEntry entry = with_stj ? cpi_running_stj_batch : cpi_preintegrate_running;
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows || !knots || !lin) return refuse(ctx, who, "NULL argument");
    if (W < 0 || N < 0) return fail(ctx, CPI_ERR_INVALID, "negative size");
    if (!model_is_cpi(prm)) return refuse_forster(ctx, who, NO_RUNNING_FORM);
    if (prm->model == CPI_MODEL_V2 && request_of(rows).jac) CPI_TRY(refuse_v2_jac_here(ctx, who, with_stj, prm, nullptr));
    if (W == 0 || N == 0) return CPI_OK;
    CPI_TRY(check_N(ctx, who, N));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    if (!first)
        return preintegrate_host_pipeline(ctx, who, W, (size_t)N, pipe_windows(knots, N, 1, count, lin, q_k_lin), rows,
                                          [&](int64_t wn, void *const *dev, const cpi_outputs *d) {
                                              return entry(ctx, prm, wn, N, (const double *)dev[0], nullptr, (const int32_t *)dev[1],
                                                                              (const double *)dev[2], (const double *)dev[3], d);
                                          });
    // ragged windows share one knot stream: staged whole, as in cpi_preintegrate_batch_host
    if (n_knots <= 0) return refuse(ctx, who, "n_knots must be > 0");
    Staging st(ctx);
    WindowsDev in;
    cpi_outputs d;
    CPI_TRY(stage_windows(st, W, n_knots, knots, first, count, lin, q_k_lin, &in));
    CPI_TRY(st.mirror(rows, (size_t)W * (size_t)N, &d));
    CPI_TRY(entry(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, &d));
    CPI_TRY(st.download(rows, d, (size_t)W * (size_t)N));
    return st.finish();
}
extern "C" int cpi_preintegrate_running_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                             const double *knots, const int64_t *first, const int32_t *count,
                                             int64_t n_knots, const double *lin, const double *q_k_lin,
                                             const cpi_outputs *rows) {
    return running_host(ctx, "cpi_preintegrate_running_host", false, prm, W, N, knots, first, count, n_knots, lin, q_k_lin, rows);
}
extern "C" int cpi_running_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                          const double *knots, const int64_t *first, const int32_t *count,
                                          int64_t n_knots, const double *lin, const double *q_k_lin,
                                          const cpi_outputs *rows) {
    return running_host(ctx, "cpi_running_stj_batch_host", true, prm, W, N, knots, first, count, n_knots, lin, q_k_lin, rows);
}

// the staged-whole form of the two resume entries: the records go up and come down with the windows.  rows_per_window: 1
// (cpi_preintegrate_resume), N (the running rows; 0 rows: only the record is computed)
template <class Entry>
static int resume_staged(cpi_ctx *ctx, Entry entry, const cpi_params *prm, int64_t W, int32_t N, size_t rows_per_window, const double *knots,
                         const int64_t *first, const int32_t *count, int64_t n_knots, const double *lin, const double *q_k_lin,
                         const double *carry_in, double *carry_out, const cpi_outputs *out) {
    const size_t cd = (size_t)W * (size_t)carry::doubles(prm->model);
    Staging st(ctx);
    WindowsDev in;
    const double *dci;
    double *dco;
    cpi_outputs d;
    CPI_TRY(stage_windows(st, W, n_knots, knots, first, count, lin, q_k_lin, &in));
    CPI_TRY(st.upload(carry_in, cd, &dci));
    CPI_TRY(st.alloc(cd, &dco));
    CPI_TRY(st.mirror(out, (size_t)W * rows_per_window, &d));
    CPI_TRY(entry(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, dci, dco, &d));
    CPI_TRY(st.download(out, d, (size_t)W * rows_per_window));
    CPI_TRY(st.download(carry_out, (const double *)dco, cd));
    return st.finish();
}

extern "C" int cpi_preintegrate_resume_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                            const double *knots, const int64_t *first, const int32_t *count,
                                            int64_t n_knots, const double *lin, const double *q_k_lin,
                                            const double *carry_in, double *carry_out, const cpi_outputs *out) {
    static const char who[] = "cpi_preintegrate_resume_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out || !knots || !lin || !carry_out) return refuse(ctx, who, "NULL argument");
    if (W <= 0) return W == 0 ? CPI_OK : fail(ctx, CPI_ERR_INVALID, "negative size");
    if (N < 0) return fail(ctx, CPI_ERR_INVALID, "negative size");
    if (!model_is_cpi(prm)) return refuse_forster(ctx, who, NOT_RESUMABLE);
    CPI_TRY(check_carry_overlap(ctx, who, prm, W, carry_in, carry_out));
    if (!first) n_knots = W * (int64_t)(N + 1);
    if (n_knots <= 0) return refuse(ctx, who, "n_knots must be > 0");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    return resume_staged(ctx, cpi_preintegrate_resume, prm, W, N, 1, knots, first, count, n_knots, lin, q_k_lin, carry_in, carry_out, out);
}

// cpi_preintegrate_running_resume from host memory: dense batches through the chunked pipeline (the records of a chunk travel with
// it), ragged ones -- and N = 0, which has no rows to chunk by -- staged whole as in cpi_preintegrate_resume_host.
// cpi_running_resume_stj_batch_host (with_stj) is the same body over its own device entry.
typedef int (*RunningResumeEntry)(cpi_ctx *, const cpi_params *, int64_t, int32_t, const double *, const int64_t *, const int32_t *, const double *,
                                  const double *, const double *, double *, const cpi_outputs *);
static int running_resume_host(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, int64_t W, int32_t N,
                               const double *knots, const int64_t *first, const int32_t *count,
                               int64_t n_knots, const double *lin, const double *q_k_lin,
                               const double *carry_in, double *carry_out, const cpi_outputs *rows) {
    const RunningResumeEntry entry = with_stj ? cpi_running_resume_stj_batch : cpi_preintegrate_running_resume;
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !rows || !knots || !lin || !carry_out) return refuse(ctx, who, "NULL argument");
    if (W < 0 || N < 0) return fail(ctx, CPI_ERR_INVALID, "negative size");
    if (!model_is_cpi(prm)) return refuse_forster(ctx, who, NO_RUNNING_FORM | NOT_RESUMABLE);
    if (prm->model == CPI_MODEL_V2 && request_of(rows).jac) CPI_TRY(refuse_v2_jac_here(ctx, who, with_stj, prm, nullptr));
    CPI_TRY(check_carry_overlap(ctx, who, prm, W, carry_in, carry_out));
    if (W == 0) return CPI_OK;
    CPI_TRY(check_N(ctx, who, N));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    if (!first && N > 0) {
        const size_t cd_bytes = (size_t)carry::doubles(prm->model) * sizeof(double);
        PipeArrays arr = pipe_windows(knots, N, 1, count, lin, q_k_lin);
        arr.a[4] = {"carry_in", carry_in, nullptr, cd_bytes, 1};
        arr.a[5] = {"carry_out", nullptr, carry_out, cd_bytes, 1};
        return preintegrate_host_pipeline(ctx, who, W, (size_t)N, arr, rows, [&](int64_t wn, void *const *dev, const cpi_outputs *d) {
            return entry(ctx, prm, wn, N, (const double *)dev[0], nullptr, (const int32_t *)dev[1], (const double *)dev[2],
                         (const double *)dev[3], (const double *)dev[4], (double *)dev[5], d);
        });
    }
    if (!first) n_knots = W * (int64_t)(N + 1);
    if (n_knots <= 0) return refuse(ctx, who, "n_knots must be > 0");
    return resume_staged(ctx, entry, prm, W, N, (size_t)N, knots, first, count, n_knots, lin, q_k_lin, carry_in, carry_out, rows);
}
extern "C" int cpi_preintegrate_running_resume_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                                    const double *knots, const int64_t *first, const int32_t *count,
                                                    int64_t n_knots, const double *lin, const double *q_k_lin,
                                                    const double *carry_in, double *carry_out, const cpi_outputs *rows) {
    return running_resume_host(ctx, "cpi_preintegrate_running_resume_host", false, prm, W, N, knots, first, count, n_knots, lin, q_k_lin,
                               carry_in, carry_out, rows);
}
extern "C" int cpi_running_resume_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                                 const double *knots, const int64_t *first, const int32_t *count,
                                                 int64_t n_knots, const double *lin, const double *q_k_lin,
                                                 const double *carry_in, double *carry_out, const cpi_outputs *rows) {
    return running_resume_host(ctx, "cpi_running_resume_stj_batch_host", true, prm, W, N, knots, first, count, n_knots, lin, q_k_lin,
                               carry_in, carry_out, rows);
}

// cpi_query_batch / cpi_query_cov_batch from host memory.  The windows are staged whole, the running rows are computed into device
// staging and never leave it (the covariance rows as P_sym: 960 B per row instead of 1 800): Q rows come down.  What the device form
// cannot check is checked here, before anything is enqueued: qwin in range, and finite non-decreasing stamps (the bisection's
// precondition) in every window that is queried.
static int query_host_check_windows(cpi_ctx *ctx, const char *who, int64_t W, int32_t N, const double *knots, const int64_t *first,
                                    const int32_t *count, int64_t n_knots, int64_t Q, const int32_t *qwin) {
    std::vector<char> seen((size_t)W, 0);
    for (int64_t k = 0; k < Q; k++) {
        const int64_t w = qwin[k];
        if (w < 0 || w >= W) return refuse(ctx, who, ("qwin[" + std::to_string(k) + "] = " + std::to_string(w) + " is not a window of [0, W)").c_str());
        if (seen[w]) continue;
        seen[w] = 1;
        const int64_t k0 = first ? first[w] : w * (int64_t)(N + 1);
        const int64_t n = count ? std::min<int64_t>(std::max<int64_t>(count[w], 0), N) : N;
        if (k0 < 0 || k0 + n >= n_knots) return refuse(ctx, who, ("window " + std::to_string(w) + " does not lie inside the knots").c_str());
        for (int64_t i = 0; i <= n; i++) {
            const double t = knots[(k0 + i) * 7];
            if (!std::isfinite(t) || (i > 0 && t < knots[(k0 + i - 1) * 7]))
                return refuse(ctx, who, ("window " + std::to_string(w) + " has a NaN, infinite or decreasing stamp at knot " + std::to_string(i) +
                                         " (a queried window needs finite non-decreasing stamps)").c_str());
        }
    }
    return CPI_OK;
}
// the rows a query entry's host form computes for the request of out (mirror() allocates the fields that are set)
static cpi_outputs query_host_rows_mask(const cpi_outputs *out, bool stj, bool cov, double *dummy) {
    cpi_outputs rmask = {};
    rmask.DT = rmask.alpha = rmask.beta = rmask.q = dummy;
    rmask.J_q = out->J_q; rmask.J_a = out->J_a; rmask.J_b = out->J_b; rmask.H_a = out->H_a; rmask.H_b = out->H_b;
    if (stj) rmask.J_q = rmask.J_a = rmask.J_b = rmask.H_a = rmask.H_b = rmask.O_a = rmask.O_b = dummy;
    if (cov) rmask.P_sym = dummy;
    return rmask;
}
static int query_host(cpi_ctx *ctx, const char *who, int with, const cpi_params *prm, int64_t W, int32_t N,
                      const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                      const double *lin, const double *q_k_lin,
                      int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out) return refuse(ctx, who, "prm/out is NULL");
    const Request rq = request_of(out);
    bool done;
    CPI_TRY(query_check_args(ctx, who, with, prm, W, N, knots, lin, q_k_lin, Q, qwin, qtime, out, &done));
    if (done) return CPI_OK;
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;   // (cpi_query_stj_batch_host only: all seven Jacobian rows are computed)
    if (!first) n_knots = W * (int64_t)(N + 1);
    if (n_knots <= 0) return refuse(ctx, who, "n_knots must be > 0");
    CPI_TRY(query_host_check_windows(ctx, who, W, N, knots, first, count, n_knots, Q, qwin));
    if (!rq.any()) return CPI_OK;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    WindowsDev in;
    const int32_t *dqwin;
    const double *dqtime;
    cpi_outputs drows, d;
    double dummy;
    const cpi_outputs rmask = query_host_rows_mask(out, stj, rq.cov, &dummy);
    CPI_TRY(stage_windows(st, W, n_knots, knots, first, count, lin, q_k_lin, &in));
    CPI_TRY(st.upload(qwin, (size_t)Q, &dqwin));
    CPI_TRY(st.upload(qtime, (size_t)Q, &dqtime));
    CPI_TRY(st.mirror(&rmask, (size_t)W * (size_t)N, &drows));
    CPI_TRY(st.mirror(out, (size_t)Q, &d));
    if (N > 0) CPI_TRY((stj ? cpi_running_stj_batch : cpi_preintegrate_running)(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, &drows));
    CPI_TRY(((with & QUERY_STJ) ? cpi_query_stj_batch : (with & QUERY_COV) ? cpi_query_cov_batch : cpi_query_batch)(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, &drows, Q, dqwin, dqtime, &d));
    CPI_TRY(st.download(out, d, (size_t)Q));
    return st.finish();
}
extern "C" int cpi_query_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                    const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                                    const double *lin, const double *q_k_lin,
                                    int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    return query_host(ctx, "cpi_query_batch_host", 0, prm, W, N, knots, first, count, n_knots, lin, q_k_lin, Q, qwin, qtime, out);
}
extern "C" int cpi_query_cov_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                        const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                                        const double *lin, const double *q_k_lin,
                                        int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    return query_host(ctx, "cpi_query_cov_batch_host", QUERY_COV, prm, W, N, knots, first, count, n_knots, lin, q_k_lin, Q, qwin, qtime, out);
}
extern "C" int cpi_query_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                        const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                                        const double *lin, const double *q_k_lin,
                                        int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    return query_host(ctx, "cpi_query_stj_batch_host", QUERY_COV | QUERY_STJ, prm, W, N, knots, first, count, n_knots, lin, q_k_lin, Q, qwin, qtime, out);
}

// cpi_query_open_batch from host memory: the chunk's windows are staged whole; the base rows (cpi_running_resume_stj_batch with N = 1
// and every count 0: the carried state read out), the chunk's running rows and carry_out are computed in device staging, Q rows and
// the records come down.  The checks on qwin and the stamps are cpi_query_batch_host's.
extern "C" int cpi_query_open_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                         const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                                         const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                                         int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out) {
    static const char who[] = "cpi_query_open_batch_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out) return refuse(ctx, who, "prm/out is NULL");
    if (!carry_out) return refuse(ctx, who, "carry_out is NULL");
    const Request rq = request_of(out);
    CPI_TRY(query_check(ctx, who, prm, rq, QUERY_COV | QUERY_STJ));
    if (W < 0 || N < 0 || Q < 0) return refuse(ctx, who, "negative size");
    CPI_TRY(check_carry_overlap(ctx, who, prm, W, carry_in, carry_out));
    if (W == 0) return Q == 0 ? CPI_OK : refuse(ctx, who, "W is 0: there is no window to query");
    if (Q > 0 && (!qwin || !qtime)) return refuse(ctx, who, "qwin/qtime is NULL");
    CPI_TRY(check_windows(ctx, who, prm, W, N, knots, lin, q_k_lin));
    if (Q > 0 && !grid_ok(Q)) return refuse(ctx, who, "Q exceeds 2^31 - 1 queries per call (32-bit grid)");
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;
    if (!first) n_knots = W * (int64_t)(N + 1);
    if (n_knots <= 0) return refuse(ctx, who, "n_knots must be > 0");
    CPI_TRY(query_host_check_windows(ctx, who, W, N, knots, first, count, n_knots, Q, qwin));

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    const size_t cd = (size_t)W * (size_t)carry::doubles(prm->model);
    // the base-row call is N = 1 with every count 0: it touches knot first[w] alone, so a dense chunk gets its own first (a dense
    // N = 1 call would look for window w at knot 2 w)
    std::vector<int64_t> first0;
    if (!first) { first0.resize((size_t)W); for (int64_t w = 0; w < W; w++) first0[w] = w * (int64_t)(N + 1); }
    Staging st(ctx);
    WindowsDev in;
    const int64_t *dfirst0 = nullptr;
    const int32_t *dqwin;
    const double *dqtime, *dci;
    double *dco, *dcb;
    int32_t *zero;
    cpi_outputs dbase, drows, d;
    double dummy;
    const cpi_outputs rmask = query_host_rows_mask(out, stj, rq.cov, &dummy);
    CPI_TRY(stage_windows(st, W, n_knots, knots, first, count, lin, q_k_lin, &in));
    CPI_TRY(st.upload(qwin, (size_t)Q, &dqwin));
    CPI_TRY(st.upload(qtime, (size_t)Q, &dqtime));
    CPI_TRY(st.upload(carry_in, cd, &dci));
    CPI_TRY(st.alloc(cd, &dco));
    CPI_TRY(st.alloc(cd, &dcb));
    CPI_TRY(st.alloc((size_t)W, &zero));
    if (!first) CPI_TRY(st.upload(first0.data(), (size_t)W, &dfirst0));
    CPI_HIP(ctx, hipMemsetAsync(zero, 0, (size_t)W * sizeof(int32_t), ctx->stream));
    CPI_TRY(st.mirror(&rmask, (size_t)W, &dbase));
    CPI_TRY(st.mirror(&rmask, (size_t)W * (size_t)N, &drows));
    CPI_TRY(st.mirror(out, (size_t)Q, &d));
    CPI_TRY(cpi_running_resume_stj_batch(ctx, prm, W, 1, in.knots, first ? in.first : dfirst0, zero, in.lin, in.qk, dci, dcb, &dbase));
    CPI_TRY(cpi_running_resume_stj_batch(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, dci, dco, &drows));
    if (Q > 0) CPI_TRY(cpi_query_open_batch(ctx, prm, W, N, in.knots, in.first, in.count, in.lin, in.qk, &drows, Q, dqwin, dqtime, &d, &dbase, 1));
    CPI_TRY(st.download(out, d, (size_t)Q));
    CPI_TRY(st.download(carry_out, (const double *)dco, cd));
    return st.finish();
}

// cpi_merge_batch from host memory.  The dense layout (first == NULL) with every group inside in_rows runs through the chunked
// pipeline: the G operand rows of a group travel with it, field by field, and one output row comes down.  A ragged layout (or a
// last group clipped by in_rows) is staged whole.
static cpi_outputs merge_in_mask(const cpi_outputs *in, const Request &rq) {
    cpi_outputs m = {};
    m.DT = in->DT; m.alpha = in->alpha; m.beta = in->beta; m.q = in->q;
    if (rq.jac || rq.cov) { m.J_q = in->J_q; m.J_a = in->J_a; m.J_b = in->J_b; m.H_a = in->H_a; m.H_b = in->H_b; }
    if (rq.cov) { if (in->P) m.P = in->P; else m.P_sym = in->P_sym; }
    return m;
}
extern "C" int cpi_merge_batch_host(cpi_ctx *ctx, int32_t model, int64_t M, int32_t G, int64_t in_rows, const cpi_outputs *in,
                                    const int64_t *first, const int32_t *count, const cpi_outputs *out) {
    static const char who[] = "cpi_merge_batch_host";
    Request rq;
    CPI_TRY(merge_check(ctx, who, model, M, G, in_rows, in, out, &rq));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (M == 0 || !rq.any()) return CPI_OK;
    if (!grid_ok((M + 3) / 4)) return refuse(ctx, who, "M exceeds the 32-bit grid (4 output rows per workgroup)");
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    const cpi_outputs need = merge_in_mask(in, rq);   // what the request reads: nothing else crosses PCIe
    if (!first && in_rows > 0 && M <= in_rows / G) {
        PipeArrays arr = {};
        static const char *const names[kOutFields] = { "DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b", "P", "P_sym" };
        int slot[kOutFields], na = 0;
        for (int k = 0; k < kOutFields; k++) {
            slot[k] = -1;
            if (const double *h = out_field_c(&need, k)) { slot[k] = na; arr.a[na++] = {names[k], h, nullptr, (size_t)G * OUT_N[k] * sizeof(double), 1}; }
        }
        const int cslot = count ? na : -1;
        if (count) arr.a[na++] = {"count", count, nullptr, sizeof(int32_t), 1};
        return preintegrate_host_pipeline(ctx, who, M, 1, arr, out, [&](int64_t mn, void *const *dev, const cpi_outputs *d) {
            cpi_outputs din = {};
            for (int k = 0; k < kOutFields; k++) if (slot[k] >= 0) *out_field(&din, k) = (double *)dev[slot[k]];
            return cpi_merge_batch(ctx, model, mn, G, mn * G, &din, nullptr, cslot >= 0 ? (const int32_t *)dev[cslot] : nullptr, d);
        });
    }
    Staging st(ctx);
    cpi_outputs din = {}, d;
    const int64_t *dfirst;
    const int32_t *dcount;
    for (int k = 0; k < kOutFields; k++) {
        const double *dk;
        CPI_TRY(st.upload(in_rows > 0 ? (const double *)out_field_c(&need, k) : nullptr, (size_t)in_rows * OUT_N[k], &dk));
        *out_field(&din, k) = const_cast<double *>(dk);
    }
    CPI_TRY(st.upload(first, (size_t)M, &dfirst));
    CPI_TRY(st.upload(count, (size_t)M, &dcount));
    CPI_TRY(st.mirror(out, (size_t)M, &d));
    CPI_TRY(cpi_merge_batch(ctx, model, M, G, in_rows, &din, dfirst, dcount, &d));
    CPI_TRY(st.download(out, d, (size_t)M));
    return st.finish();
}

// The offsets of a multi-run call as the _host entries can (and do) validate them before anything is enqueued: each array
// starts at 0, never decreases and ends at K (stream_offsets) / U (update_offsets).
static int check_offsets(cpi_ctx *ctx, const char *who, int64_t R, const int64_t *stream_offsets, int64_t K, const int64_t *update_offsets, int64_t U) {
    for (int pass = 0; pass < 2; pass++) {
        const int64_t *o = pass ? update_offsets : stream_offsets;
        const int64_t end = pass ? U : K;
        const char *what = pass ? "update_offsets" : "stream_offsets";
        if (o[0] != 0) return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": " + what + "[0] is not 0");
        for (int64_t r = 0; r < R; r++)
            if (o[r + 1] < o[r]) return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": " + what + " decrease at run " + std::to_string(r));
        if (o[R] != end) return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": " + what + "[R] is not " + (pass ? "U" : "K"));
    }
    return CPI_OK;
}
// the arrays of the stream entries, staged whole (stream_offsets == NULL: one stream), and a workspace for U windows
struct StreamsDev {
    const double *stream, *update, *lin, *qk;
    const int64_t *soff, *uoff;
    void *ws;
};
static int stage_streams(Staging &st, int64_t R, int64_t K, const double *stream, const int64_t *stream_offsets, int64_t U,
                         const double *update_times, const int64_t *update_offsets, const double *lin, const double *q_k_lin, StreamsDev *d) {
    CPI_TRY(st.upload(stream, (size_t)K * 7, &d->stream));
    CPI_TRY(st.upload(stream_offsets, (size_t)(R + 1), &d->soff));
    CPI_TRY(st.upload(update_times, (size_t)U, &d->update));
    CPI_TRY(st.upload(update_offsets, (size_t)(R + 1), &d->uoff));
    CPI_TRY(st.upload(lin, (size_t)U * 6, &d->lin));
    CPI_TRY(st.upload(q_k_lin, (size_t)U * 4, &d->qk));
    return st.alloc(cpi_streams_workspace_bytes(R, U), &d->ws);
}

// The stream entry from HOST memory: what a GraphSolver-shaped caller holds (its IMU deque as one array, the update times of the
// states it creates, one linearisation point per window) -> the measurements of every window, in host memory.  One-off
// staging (the stream is uploaded once, whole); the windows are cut on the device.
extern "C" int cpi_preintegrate_stream_host(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                            const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                            const cpi_outputs *out, int32_t *count) {
    static const char who[] = "cpi_preintegrate_stream_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (K < 0 || U < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (U == 0) return CPI_OK;
    if (K == 0) return refuse(ctx, who, "the stream is empty");
    if (!prm || !out || !stream || !update_times || !lin) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_qk(ctx, who, prm, q_k_lin));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    StreamsDev in;
    cpi_outputs d;
    CPI_TRY(stage_streams(st, 0, K, stream, nullptr, U, update_times, nullptr, lin, q_k_lin, &in));
    CPI_TRY(st.mirror(out, (size_t)U, &d));
    CPI_TRY(cpi_preintegrate_stream(ctx, prm, K, in.stream, U, in.update, N, in.lin, in.qk, in.ws, &d));
    CPI_TRY(st.download(out, d, (size_t)U));
    if (count) CPI_TRY(st.download(count, cpi_stream_counts(in.ws, U), (size_t)U));
    return st.finish();
}

// The multi-run entry from HOST memory.  Unlike the device entry it can read the offsets (check_offsets).
extern "C" int cpi_preintegrate_streams_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                             const int64_t *stream_offsets, int64_t U, const double *update_times,
                                             const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                             const cpi_outputs *out, int32_t *count) {
    static const char who[] = "cpi_preintegrate_streams_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (R < 0 || K < 0 || U < 0 || N < 0) return refuse(ctx, who, "negative size");
    if (U == 0) return CPI_OK;
    if (R == 0) return refuse(ctx, who, "U > 0 windows and no run");
    if (K == 0) return refuse(ctx, who, "the streams hold no reading");
    if (!prm || !out || !stream || !stream_offsets || !update_times || !update_offsets || !lin) return refuse(ctx, who, "NULL argument");
    CPI_TRY(check_qk(ctx, who, prm, q_k_lin));
    CPI_TRY(check_offsets(ctx, who, R, stream_offsets, K, update_offsets, U));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    StreamsDev in;
    cpi_outputs d;
    CPI_TRY(stage_streams(st, R, K, stream, stream_offsets, U, update_times, update_offsets, lin, q_k_lin, &in));
    CPI_TRY(st.mirror(out, (size_t)U, &d));
    CPI_TRY(cpi_preintegrate_streams(ctx, prm, R, K, in.stream, in.soff, U, in.update, in.uoff, N, in.lin, in.qk, in.ws, &d));
    CPI_TRY(st.download(out, d, (size_t)U));
    if (count) CPI_TRY(st.download(count, cpi_stream_counts(in.ws, U), (size_t)U));
    return st.finish();
}

// The running stream entries from HOST memory: the stream(s) are uploaded once, whole, and cut on the device; the U * N rows come
// back in chunks of whole windows, never more than 2^18 rows per chunk (N <= 65535: at least 4 windows), the
// kernels of a chunk and its download following each other on the context's stream.  The lane choice is that of the whole call,
// so the rows do not depend on the chunking.
static int stream_running_host_impl(cpi_ctx *ctx, const char *who, bool with_stj, const cpi_params *prm, bool many, int64_t R, int64_t K,
                                    const double *stream, const int64_t *stream_offsets, int64_t U, const double *update_times,
                                    const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                    const cpi_outputs *rows, int32_t *count) {
    bool noop;
    const int rc = stream_running_check(ctx, who, with_stj, prm, many, R, K, U, N, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin, rows, noop);
    if (rc != CPI_OK || noop) return rc;
    if (many) CPI_TRY(check_offsets(ctx, who, R, stream_offsets, K, update_offsets, U));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    StreamsDev in;
    cpi_outputs d;
    CPI_TRY(stage_streams(st, many ? R : 0, K, stream, many ? stream_offsets : nullptr, U, update_times, many ? update_offsets : nullptr, lin, q_k_lin, &in));
    // windows per chunk: as many whole windows as 2^18 rows hold (whole wavefronts of one-lane windows when that is 64 or more;
    // N <= 65535, so at least 4), never more than 2^18 rows of staging per output array
    int64_t cw = std::max<int64_t>(1, ((int64_t)1 << 18) / N);
    if (cw >= 64) cw = cw / 64 * 64;
    cw = std::min<int64_t>(U, cw);
    CPI_TRY(st.mirror(rows, (size_t)cw * (size_t)N, &d));
    RunArgs ra;
    ra.soff = (const long long *)in.soff; ra.uoff = (const long long *)in.uoff; ra.R = (int)R;
    const StreamCut sc = stream_cut(K, in.update, in.ws, U, many ? &ra : nullptr);
    CPI_TRY(cut_launch(ctx, sc, in.stream, U, N));
    const int L = stream_running_lanes(prm, U, N, rows);
    for (int64_t w0 = 0; w0 < U; w0 += cw) {
        const int64_t wn = std::min<int64_t>(cw, U - w0);
        CPI_TRY(stream_running_launch(ctx, prm, sc, in.stream, N, L, in.lin, in.qk, &d, w0, wn));
        CPI_TRY(st.download(rows, d, (size_t)wn * (size_t)N, (size_t)w0 * (size_t)N));
    }
    if (count) CPI_TRY(st.download(count, cpi_stream_counts(in.ws, U), (size_t)U));
    return st.finish();
}
extern "C" int cpi_preintegrate_stream_running_host(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                                    const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                                    const cpi_outputs *rows, int32_t *count) {
    return stream_running_host_impl(ctx, "cpi_preintegrate_stream_running_host", false, prm, false, 0, K, stream, nullptr, U, update_times,
                                    nullptr, N, lin, q_k_lin, rows, count);
}
extern "C" int cpi_preintegrate_streams_running_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                                     const int64_t *stream_offsets, int64_t U, const double *update_times,
                                                     const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                                     const cpi_outputs *rows, int32_t *count) {
    return stream_running_host_impl(ctx, "cpi_preintegrate_streams_running_host", false, prm, true, R, K, stream, stream_offsets, U,
                                    update_times, update_offsets, N, lin, q_k_lin, rows, count);
}
extern "C" int cpi_stream_running_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                                 const int64_t *stream_offsets, int64_t U, const double *update_times,
                                                 const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                                 const cpi_outputs *rows, int32_t *count) {
    const bool one = one_stream(R, stream_offsets, update_offsets);
    return stream_running_host_impl(ctx, "cpi_stream_running_stj_batch_host", true, prm, !one, one ? 0 : R, K, stream, stream_offsets, U,
                                    update_times, update_offsets, N, lin, q_k_lin, rows, count);
}

// cpi_query_stream_batch from host memory.  The stream(s) are staged whole, the running rows are computed into device staging by
// cpi_stream_running_stj_batch and never leave it (the covariance rows as P_sym), Q rows and qwin_out come down.  What the device form
// cannot check is checked here, before anything is enqueued: the offsets and qrun in range.
extern "C" int cpi_query_stream_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                           const int64_t *stream_offsets, int64_t U, const double *update_times,
                                           const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                           int64_t Q, const int32_t *qrun, const double *qtime, int32_t *qwin_out,
                                           const cpi_outputs *out) {
    static const char who[] = "cpi_query_stream_batch_host";
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!prm || !out) return refuse(ctx, who, "prm/out is NULL");
    const bool one = one_stream(R, stream_offsets, update_offsets);
    bool done;
    CPI_TRY(query_stream_check(ctx, who, prm, one, R, K, U, N, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin, Q, qtime, out, &done));
    if (done) return CPI_OK;
    if (!one) CPI_TRY(check_offsets(ctx, who, R, stream_offsets, K, update_offsets, U));
    if (qrun)
        for (int64_t k = 0; k < Q; k++)
            if (qrun[k] < 0 || qrun[k] >= R) return refuse(ctx, who, ("qrun[" + std::to_string(k) + "] = " + std::to_string(qrun[k]) + " is not a run of [0, R)").c_str());
    const Request rq = request_of(out);
    if (!rq.any() && !qwin_out) return CPI_OK;
    const bool stj = prm->model == CPI_MODEL_V2 && rq.jac;

    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    StreamsDev in;
    const int32_t *dqrun;
    const double *dqtime;
    int32_t *dqwin = nullptr;
    cpi_outputs rmask = {}, drows, d;
    double dummy;
    if (rq.any()) rmask.DT = rmask.alpha = rmask.beta = rmask.q = &dummy;   // mirror() allocates the fields that are set
    rmask.J_q = out->J_q; rmask.J_a = out->J_a; rmask.J_b = out->J_b; rmask.H_a = out->H_a; rmask.H_b = out->H_b;
    if (stj) rmask.J_q = rmask.J_a = rmask.J_b = rmask.H_a = rmask.H_b = rmask.O_a = rmask.O_b = &dummy;
    if (rq.cov) rmask.P_sym = &dummy;
    CPI_TRY(stage_streams(st, one ? 0 : R, K, stream, one ? nullptr : stream_offsets, U, update_times, one ? nullptr : update_offsets, lin, q_k_lin, &in));
    CPI_TRY(st.upload(qrun, (size_t)Q, &dqrun));
    CPI_TRY(st.upload(qtime, (size_t)Q, &dqtime));
    if (qwin_out) CPI_TRY(st.alloc((size_t)Q, &dqwin));
    CPI_TRY(st.mirror(&rmask, (size_t)U * (size_t)N, &drows));
    CPI_TRY(st.mirror(out, (size_t)Q, &d));
    if (N > 0 && rq.any())
        CPI_TRY(cpi_stream_running_stj_batch(ctx, prm, R, K, in.stream, in.soff, U, in.update, in.uoff, N, in.lin, in.qk, in.ws, &drows));
    CPI_TRY(cpi_query_stream_batch(ctx, prm, R, K, in.stream, in.soff, U, in.update, in.uoff, N, in.lin, in.qk, in.ws, &drows, Q, dqrun, dqtime, dqwin, &d));
    CPI_TRY(st.download(out, d, (size_t)Q));
    if (qwin_out) CPI_TRY(st.download(qwin_out, (const int32_t *)dqwin, (size_t)Q));
    return st.finish();
}

extern "C" int cpi_factor_eval_batch_host(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                          const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                          const double *states, int64_t S, const int32_t *idx_i,
                                          const int32_t *idx_j, double *err, double *H1, double *H2) {
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (!meas || !lin || !states || !err || !grav) return fail(ctx, CPI_ERR_INVALID, "cpi_factor_eval_batch_host: NULL argument");
    if (F <= 0) return F == 0 ? CPI_OK : fail(ctx, CPI_ERR_INVALID, "negative size");
    CPI_TRY(check_state_indices(ctx, "cpi_factor_eval_batch_host", F, S, idx_i, idx_j));
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    FactorsDev in;
    double *de, *dh1 = nullptr, *dh2 = nullptr;
    CPI_TRY(stage_factors(st, F, S, meas, lin, q_k_lin, states, idx_i, idx_j, &in));
    CPI_TRY(st.alloc((size_t)F * 15, &de));
    if (H1) CPI_TRY(st.alloc((size_t)F * 225, &dh1));
    if (H2) CPI_TRY(st.alloc((size_t)F * 225, &dh2));
    CPI_TRY(cpi_factor_eval_batch(ctx, model, grav, F, &in.meas, in.lin, in.qk, in.states, S, in.idx_i, in.idx_j, de, dh1, dh2));
    CPI_TRY(st.download(err, (const double *)de, (size_t)F * 15));
    if (H1) CPI_TRY(st.download(H1, (const double *)dh1, (size_t)F * 225));
    if (H2) CPI_TRY(st.download(H2, (const double *)dh2, (size_t)F * 225));
    return st.finish();
}

// cpi_retract_batch / cpi_local_batch from host memory: staged whole, synchronous.
extern "C" int cpi_retract_batch_host(cpi_ctx *ctx, int64_t S, const double *states_in, const double *delta, double *states_out) {
    CPI_TRY(retract_check(ctx, "cpi_retract_batch_host", S, states_in, delta, states_out));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (S == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    const double *ds, *dd;
    CPI_TRY(st.upload(states_in, (size_t)S * 16, &ds));
    CPI_TRY(st.upload(delta, (size_t)S * 15, &dd));
    double *dso = const_cast<double *>(ds);   // in place on the device copy
    CPI_TRY(cpi_retract_batch(ctx, S, ds, dd, dso));
    CPI_TRY(st.download(states_out, (const double *)dso, (size_t)S * 16));
    return st.finish();
}
extern "C" int cpi_local_batch_host(cpi_ctx *ctx, int64_t S, const double *x, const double *other, double *xi) {
    CPI_TRY(local_check(ctx, "cpi_local_batch_host", S, x, other, xi));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (S == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    const double *dx, *dox;
    double *dxi;
    CPI_TRY(st.upload(x, (size_t)S * 16, &dx));
    CPI_TRY(st.upload(other, (size_t)S * 16, &dox));
    CPI_TRY(st.alloc((size_t)S * 15, &dxi));
    CPI_TRY(cpi_local_batch(ctx, S, dx, dox, dxi));
    CPI_TRY(st.download(xi, (const double *)dxi, (size_t)S * 15));
    return st.finish();
}

// GTSAM's factor.error(values) for F factors held in host memory: the covariance of the measurement (P_sym when set, else the
// dense P packed here) is factorised on the device (cpi_sqrt_information_packed_batch), then cpi_factor_cost_tri_batch.
extern "C" int cpi_factor_cost_batch_host(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                          const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                          const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                          double *chi2, double *werr, double *total) {
    static const char who[] = "cpi_factor_cost_batch_host";
    if (model != CPI_MODEL_V1 && model != CPI_MODEL_V2) return refuse(ctx, who, "model must be 1 or 2");
    if (F < 0) return refuse(ctx, who, "negative size");
    if (F > 0) {
        if (!chi2) return refuse(ctx, who, "chi2 is NULL");
        if (!meas || !lin || !states || !grav) return refuse(ctx, who, "NULL argument");
        if (!meas->P_sym && !meas->P) return refuse(ctx, who, "meas must hold P_sym or P (the covariance that is factorised)");
        CPI_TRY(check_state_indices(ctx, who, F, S, idx_i, idx_j));
    }
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0) { if (total) total[0] = 0.0; return CPI_OK; }
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    std::vector<double> packed;   // declared BEFORE the staging: its destructor drains the stream while this buffer still exists
    Staging st(ctx);
    const double *psym = meas->P_sym;
    if (!psym) {   // the upper triangle of the dense P, CPI_TRI_INDEX order
        packed.resize((size_t)F * CPI_TRI_DOUBLES);
        for (int64_t f = 0; f < F; f++)
            for (int k = 0; k < 15; k++)
                for (int i = 0; i <= k; i++) packed[(size_t)f * CPI_TRI_DOUBLES + CPI_TRI_INDEX(i, k)] = meas->P[(size_t)f * 225 + k * 15 + i];
        psym = packed.data();
    }
    FactorsDev in;
    const double *dp;
    double *dr, *dc, *dw = nullptr, *dt = nullptr;
    CPI_TRY(stage_factors(st, F, S, meas, lin, q_k_lin, states, idx_i, idx_j, &in));
    CPI_TRY(st.upload(psym, (size_t)F * CPI_TRI_DOUBLES, &dp));
    CPI_TRY(st.alloc((size_t)F * CPI_TRI_DOUBLES, &dr));
    CPI_TRY(st.alloc((size_t)F, &dc));
    if (werr) CPI_TRY(st.alloc((size_t)F * 15, &dw));
    if (total) CPI_TRY(st.alloc(cpi_factor_cost_total_doubles(F), &dt));
    CPI_TRY(cpi_sqrt_information_packed_batch(ctx, F, dp, dr));
    CPI_TRY(cpi_factor_cost_tri_batch(ctx, model, grav, F, &in.meas, in.lin, in.qk, in.states, S, in.idx_i, in.idx_j, dr, dc, dw, dt));
    CPI_TRY(st.download(chi2, (const double *)dc, (size_t)F));
    if (werr) CPI_TRY(st.download(werr, (const double *)dw, (size_t)F * 15));
    if (total) CPI_TRY(st.download(total, (const double *)dt, (size_t)1));
    return st.finish();
}

// cpi_chain_solve_batch from host memory: every array a host array, staged whole, synchronous.  Host pointers: every chain's state
// and factor range can be (and is) validated here; the device form clamps or refuses them per chain instead.  delta travels up before
// the solve, so that the rows of no chain come back as the caller left them.
extern "C" int cpi_chain_solve_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                          const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                          const double *hess, const double *prior, const double *lambda, int32_t damping,
                                          double *delta, int32_t *status) {
    static const char who[] = "cpi_chain_solve_batch_host";
    CPI_TRY(chain_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, lambda, damping, delta, status, nullptr, true));
    CPI_TRY(chain_ranges_check(ctx, who, C, G, S, F, first, count, ffirst));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    ChainsDev in;
    const double *dl, *dd0 = nullptr;
    double *dd = nullptr;
    int32_t *ds = nullptr;
    CPI_TRY(stage_chains(st, C, G, S, F, first, count, ffirst, hess, prior, &in));
    CPI_TRY(st.upload(lambda, (size_t)C, &dl));
    if (S > 0) {
        CPI_TRY(st.upload((const double *)delta, (size_t)S * 15, &dd0));
        dd = const_cast<double *>(dd0);
    } else {
        CPI_TRY(st.alloc((size_t)1, &dd));
    }
    if (status) CPI_TRY(st.alloc((size_t)C, &ds));
    CPI_TRY(cpi_chain_solve_batch(ctx, C, G, S, F, in.first, in.count, in.ffirst, in.hess, in.prior, dl, damping, dd, ds, in.workspace));
    if (S > 0) CPI_TRY(st.download(delta, (const double *)dd, (size_t)S * 15));
    if (status) CPI_TRY(st.download(status, (const int32_t *)ds, (size_t)C));
    return st.finish();
}

// cpi_chain_marginals_batch from host memory: the undamped solve of the host arrays on the device, the marginals kernel on the
// workspace it left, cov / cross / status back.  cov and cross travel up before the kernels, so that the rows nobody writes come back
// as the caller left them.  The ranges are validated as in cpi_chain_solve_batch_host.
extern "C" int cpi_chain_marginals_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                              const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                              const double *hess, const double *prior,
                                              double *cov, double *cross, int32_t *status) {
    static const char who[] = "cpi_chain_marginals_batch_host";
    CPI_TRY(marginals_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, status, nullptr, cov, cross, true));
    CPI_TRY(chain_ranges_check(ctx, who, C, G, S, F, first, count, ffirst));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0 || S == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    ChainsDev in;
    const double *dc0, *dx0 = nullptr;
    double *dd;
    int32_t *ds;
    CPI_TRY(stage_chains(st, C, G, S, F, first, count, ffirst, hess, prior, &in));
    CPI_TRY(st.upload((const double *)cov, (size_t)S * 120, &dc0));
    if (cross) CPI_TRY(st.upload((const double *)cross, (size_t)S * 225, &dx0));
    CPI_TRY(st.alloc((size_t)S * 15, &dd));
    CPI_TRY(st.alloc((size_t)C, &ds));
    CPI_TRY(cpi_chain_solve_batch(ctx, C, G, S, F, in.first, in.count, in.ffirst, in.hess, in.prior, nullptr, CPI_DAMP_IDENTITY, dd, ds, in.workspace));
    CPI_TRY(cpi_chain_marginals_batch(ctx, C, G, S, in.first, in.count, ds, in.workspace, const_cast<double *>(dc0), const_cast<double *>(dx0)));
    CPI_TRY(st.download(cov, dc0, (size_t)S * 120));
    if (cross) CPI_TRY(st.download(cross, dx0, (size_t)S * 225));
    if (status) CPI_TRY(st.download(status, (const int32_t *)ds, (size_t)C));
    return st.finish();
}

// cpi_chain_marginalize_batch from host memory: every array a host array (drop too), staged whole, synchronous.  The ranges are
// validated as in cpi_chain_solve_batch_host, and every chain that has states must eliminate fewer than it has.
extern "C" int cpi_chain_marginalize_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                                const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                                const double *hess, const double *prior,
                                                int32_t M, const int32_t *drop,
                                                double *out, int32_t *status) {
    static const char who[] = "cpi_chain_marginalize_batch_host";
    CPI_TRY(marginalize_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, drop, out, status));
    CPI_TRY(chain_ranges_check(ctx, who, C, G, S, F, first, count, ffirst));
    for (int64_t c = 0; c < C; c++) {
        int64_t n = count ? count[c] : G;
        n = n < 0 ? 0 : (n > G ? G : n);
        const int64_t m = drop ? drop[c] : M;
        if (n > 0 && (m < 0 || m >= n))
            return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": drop of chain " + std::to_string(c) + " leaves [0, count)");
    }
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    ChainsDev in;
    const int32_t *dm;
    double *dout;
    int32_t *ds = nullptr;
    CPI_TRY(stage_chains(st, C, G, S, F, first, count, ffirst, hess, prior, &in, false));
    CPI_TRY(st.upload(drop, (size_t)C, &dm));
    CPI_TRY(st.alloc((size_t)C * 136, &dout));
    if (status) CPI_TRY(st.alloc((size_t)C, &ds));
    CPI_TRY(cpi_chain_marginalize_batch(ctx, C, G, S, F, in.first, in.count, in.ffirst, in.hess, in.prior, M, dm, dout, ds));
    CPI_TRY(st.download(out, (const double *)dout, (size_t)C * 136));
    if (status) CPI_TRY(st.download(status, (const int32_t *)ds, (size_t)C));
    return st.finish();
}

// cpi_chain_condense_batch from host memory: every array a host array, staged whole, synchronous.  The ranges are validated as in
// cpi_chain_solve_batch_host.  The workspace stays on the device: workspace_out NULL, or cpi_chain_condense_workspace_doubles(S) HOST
// doubles that receive it (what cpi_chain_expand_batch_host takes).  The reduced arrays travel up before the kernel, so that the rows
// nobody writes come back as the caller left them.
extern "C" int cpi_chain_condense_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                             const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                             const double *hess, const double *prior, const double *lambda, int32_t damping, int64_t K,
                                             double *rhess, double *rprior, int32_t *rcount,
                                             int32_t *status, double *workspace_out) {
    static const char who[] = "cpi_chain_condense_batch_host";
    CPI_TRY(condense_check(ctx, who, C, G, S, F, first, count, ffirst, hess, prior, lambda, damping, K, rhess, rprior, rcount, status, workspace_out, true));
    CPI_TRY(chain_ranges_check(ctx, who, C, G, S, F, first, count, ffirst));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    ChainsDev in;
    const int64_t Gr = cpi_chain_condense_states(G, K);
    const size_t nh = (size_t)C * (size_t)(Gr - 1) * 496, np = (size_t)C * (size_t)Gr * 136, nw = cpi_chain_condense_workspace_doubles(S);
    const double *dl, *dh0 = nullptr, *dp0, *dw0 = nullptr;
    double *dh = nullptr, *dw = nullptr;
    int32_t *dc, *ds = nullptr;
    CPI_TRY(stage_chains(st, C, G, S, F, first, count, ffirst, hess, prior, &in, false));
    CPI_TRY(st.upload(lambda, (size_t)C, &dl));
    if (nh > 0) {
        CPI_TRY(st.upload((const double *)rhess, nh, &dh0));
        dh = const_cast<double *>(dh0);
    } else {
        CPI_TRY(st.alloc((size_t)1, &dh));
    }
    CPI_TRY(st.upload((const double *)rprior, np, &dp0));
    if (workspace_out) {
        CPI_TRY(st.upload((const double *)workspace_out, nw, &dw0));
        dw = const_cast<double *>(dw0);
    } else {
        CPI_TRY(st.alloc(nw, &dw));
    }
    CPI_TRY(st.alloc((size_t)C, &dc));
    if (status && Gr > 1) CPI_TRY(st.alloc((size_t)C * (size_t)(Gr - 1), &ds));
    CPI_TRY(cpi_chain_condense_batch(ctx, C, G, S, F, in.first, in.count, in.ffirst, in.hess, in.prior, dl, damping, K, dh, const_cast<double *>(dp0), dc, ds, dw));
    if (nh > 0) CPI_TRY(st.download(rhess, (const double *)dh, nh));
    CPI_TRY(st.download(rprior, dp0, np));
    CPI_TRY(st.download(rcount, (const int32_t *)dc, (size_t)C));
    if (ds) CPI_TRY(st.download(status, (const int32_t *)ds, (size_t)C * (size_t)(Gr - 1)));
    if (workspace_out) CPI_TRY(st.download(workspace_out, (const double *)dw, nw));
    return st.finish();
}

// cpi_chain_expand_batch from host memory: every array a host array (the workspace too: what cpi_chain_condense_batch_host returned),
// staged whole, synchronous.  The state ranges are validated.  delta travels up before the kernel.
extern "C" int cpi_chain_expand_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S,
                                           const int64_t *first, const int32_t *count, int64_t K,
                                           const double *rdelta, const double *workspace, double *delta) {
    static const char who[] = "cpi_chain_expand_batch_host";
    CPI_TRY(expand_check(ctx, who, C, G, S, first, count, K, rdelta, workspace, delta));
    for (int64_t c = 0; c < C; c++) {
        const int64_t f = first ? first[c] : c * G;
        int64_t n = count ? count[c] : G;
        n = n < 0 ? 0 : (n > G ? G : n);
        if (f < 0 || f > S || n > S - f)
            return fail(ctx, CPI_ERR_INVALID, std::string(who) + ": the states of chain " + std::to_string(c) + " leave [0, S)");
    }
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    const int64_t Gr = cpi_chain_condense_states(G, K);
    const int64_t *df;
    const int32_t *dn;
    const double *dr, *dw, *dd0 = nullptr;
    double *dd = nullptr;
    CPI_TRY(st.upload(first, (size_t)C, &df));
    CPI_TRY(st.upload(count, (size_t)C, &dn));
    CPI_TRY(st.upload(rdelta, (size_t)C * (size_t)Gr * 15, &dr));
    CPI_TRY(st.upload(workspace, cpi_chain_condense_workspace_doubles(S), &dw));
    if (S > 0) {
        CPI_TRY(st.upload((const double *)delta, (size_t)S * 15, &dd0));
        dd = const_cast<double *>(dd0);
    } else {
        CPI_TRY(st.alloc((size_t)1, &dd));
    }
    CPI_TRY(cpi_chain_expand_batch(ctx, C, G, S, df, dn, K, dr, dw, dd));
    if (S > 0) CPI_TRY(st.download(delta, (const double *)dd, (size_t)S * 15));
    return st.finish();
}

// cpi_prior_relinearize_batch / cpi_chain_cost_batch / cpi_chain_accept_batch from host memory: every array a host array, staged whole,
// synchronous.  Outputs and in/out arrays travel up before the kernel, so that what nobody writes comes back as the caller left it.
extern "C" int cpi_prior_relinearize_batch_host(cpi_ctx *ctx, int64_t S, int64_t P, const int32_t *idx,
                                                const double *states, const double *anchor, const double *prior0,
                                                double *prior, double *pcost) {
    static const char who[] = "cpi_prior_relinearize_batch_host";
    CPI_TRY(lm_prior_check(ctx, who, S, P, idx, states, anchor, prior0, prior, pcost));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (P == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    const int32_t *di;
    const double *ds, *da, *d0, *dp = nullptr, *dc = nullptr;
    CPI_TRY(st.upload(idx, (size_t)P, &di));
    CPI_TRY(st.upload(S > 0 ? states : nullptr, (size_t)S * 16, &ds));
    CPI_TRY(st.upload(anchor, (size_t)P * 16, &da));
    CPI_TRY(st.upload(prior0, (size_t)P * 136, &d0));
    if (S > 0 && prior) CPI_TRY(st.upload((const double *)prior, (size_t)S * 136, &dp));
    if (S > 0 && pcost) CPI_TRY(st.upload((const double *)pcost, (size_t)S, &dc));
    if (S == 0) return st.finish();                    // every record is skipped
    CPI_TRY(cpi_prior_relinearize_batch(ctx, S, P, di, ds, da, d0, const_cast<double *>(dp), const_cast<double *>(dc)));
    if (prior) CPI_TRY(st.download(prior, dp, (size_t)S * 136));
    if (pcost) CPI_TRY(st.download(pcost, dc, (size_t)S));
    return st.finish();
}

// first / count / ffirst and the two term arrays of a chain cost, staged whole
struct LmTermsDev {
    const int64_t *first, *ffirst;
    const int32_t *count;
    const double *chi2, *pcost;
};
static int stage_lm_terms(Staging &st, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count, const int64_t *ffirst,
                          const double *chi2, const double *pcost, LmTermsDev *d) {
    CPI_TRY(st.upload(first, (size_t)C, &d->first));
    CPI_TRY(st.upload(count, (size_t)C, &d->count));
    CPI_TRY(st.upload(ffirst, (size_t)C, &d->ffirst));
    CPI_TRY(st.upload(F > 0 ? chi2 : nullptr, (size_t)F, &d->chi2));
    CPI_TRY(st.upload(S > 0 ? pcost : nullptr, (size_t)S, &d->pcost));
    if (!d->chi2 && G > 1) {   // F == 0: no chain has a factor (the ranges are validated), and the device form wants a pointer it never reads
        double *none;
        CPI_TRY(st.alloc((size_t)1, &none));
        d->chi2 = none;
    }
    return CPI_OK;
}
extern "C" int cpi_chain_cost_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                         const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                         const double *chi2, const double *pcost, double *cost) {
    static const char who[] = "cpi_chain_cost_batch_host";
    CPI_TRY(lm_cost_check(ctx, who, C, G, S, F, first, count, ffirst, chi2, pcost, cost));
    CPI_TRY(chain_ranges_check(ctx, who, C, G, S, F, first, count, ffirst));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    LmTermsDev in;
    double *dc;
    CPI_TRY(stage_lm_terms(st, C, G, S, F, first, count, ffirst, chi2, pcost, &in));
    CPI_TRY(st.alloc((size_t)C, &dc));
    CPI_TRY(cpi_chain_cost_batch(ctx, C, G, S, F, in.first, in.count, in.ffirst, in.chi2, in.pcost, dc));
    CPI_TRY(st.download(cost, (const double *)dc, (size_t)C));
    return st.finish();
}
extern "C" int cpi_chain_accept_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                           const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                           const cpi_lm_params *params,
                                           const double *chi2_new, const double *pcost_new, const double *trial,
                                           double *cost, double *states, double *chi2, double *lambda,
                                           int32_t *phase, int32_t *accepted) {
    static const char who[] = "cpi_chain_accept_batch_host";
    CPI_TRY(lm_accept_check(ctx, who, C, G, S, F, first, count, ffirst, params, chi2_new, pcost_new, trial, cost, states, chi2, lambda, phase, accepted));
    CPI_TRY(chain_ranges_check(ctx, who, C, G, S, F, first, count, ffirst));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (C == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    LmTermsDev in;
    const double *dt, *dcost, *dstates, *dchi2 = nullptr, *dlam;
    const int32_t *dphase;
    int32_t *dacc = nullptr;
    CPI_TRY(stage_lm_terms(st, C, G, S, F, first, count, ffirst, chi2_new, pcost_new, &in));
    CPI_TRY(st.upload(S > 0 ? trial : nullptr, (size_t)S * 16, &dt));
    CPI_TRY(st.upload((const double *)cost, (size_t)C, &dcost));
    CPI_TRY(st.upload(S > 0 ? (const double *)states : nullptr, (size_t)S * 16, &dstates));
    if (F > 0 && chi2) CPI_TRY(st.upload((const double *)chi2, (size_t)F, &dchi2));
    CPI_TRY(st.upload((const double *)lambda, (size_t)C, &dlam));
    CPI_TRY(st.upload((const int32_t *)phase, (size_t)C, &dphase));
    if (accepted) CPI_TRY(st.alloc((size_t)C, &dacc));
    CPI_TRY(cpi_chain_accept_batch(ctx, C, G, S, F, in.first, in.count, in.ffirst, params, in.chi2, in.pcost, dt, const_cast<double *>(dcost),
                                   const_cast<double *>(dstates), const_cast<double *>(dchi2), const_cast<double *>(dlam),
                                   const_cast<int32_t *>(dphase), dacc));
    CPI_TRY(st.download(cost, dcost, (size_t)C));
    if (S > 0) CPI_TRY(st.download(states, dstates, (size_t)S * 16));
    if (dchi2) CPI_TRY(st.download(chi2, dchi2, (size_t)F));
    CPI_TRY(st.download(lambda, dlam, (size_t)C));
    CPI_TRY(st.download(phase, dphase, (size_t)C));
    if (accepted) CPI_TRY(st.download(accepted, (const int32_t *)dacc, (size_t)C));
    return st.finish();
}

// cpi_state_fix_batch from host memory: every array a host array, staged whole, synchronous.  mfirst is validated first.
extern "C" int cpi_state_fix_batch_host(cpi_ctx *ctx, int64_t S, int64_t M, int32_t kind, const int64_t *mfirst,
                                        const double *states, const double *z, const double *R,
                                        const double *weight, const double *base,
                                        const double *pcost_base, double *out,
                                        double *pcost, double *chi2) {
    static const char who[] = "cpi_state_fix_batch_host";
    CPI_TRY(fix_check(ctx, who, S, M, kind, mfirst, states, z, R, weight, base, pcost_base, out, pcost, chi2));
    for (int64_t s = 0; s < S; s++)
        if (mfirst[s] < 0 || mfirst[s + 1] > M || mfirst[s + 1] < mfirst[s])
            return refuse(ctx, who, ("the fixes of state " + std::to_string(s) + " leave [0, M] or mfirst decreases there").c_str());
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (S == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    const int64_t *df;
    const double *ds, *dz, *dR, *dw, *db, *dpb;
    double *dout = nullptr, *dpc = nullptr, *dchi = nullptr;
    CPI_TRY(st.upload(mfirst, (size_t)S + 1, &df));
    CPI_TRY(st.upload(states, (size_t)S * 16, &ds));
    CPI_TRY(st.upload(M > 0 ? z : nullptr, (size_t)M * kFixZ[kind], &dz));
    CPI_TRY(st.upload(M > 0 ? R : nullptr, (size_t)M * kFixR[kind], &dR));
    CPI_TRY(st.upload(M > 0 ? weight : nullptr, (size_t)M, &dw));
    CPI_TRY(st.upload(base, (size_t)S * 136, &db));
    CPI_TRY(st.upload(pcost_base, (size_t)S, &dpb));
    if (out) CPI_TRY(st.alloc((size_t)S * 136, &dout));
    if (pcost) CPI_TRY(st.alloc((size_t)S, &dpc));
    if (chi2 && M > 0) CPI_TRY(st.alloc((size_t)M, &dchi));
    if (!dout && !dpc && !dchi) return st.finish();    // chi2 alone with M == 0: nothing to write
    CPI_TRY(cpi_state_fix_batch(ctx, S, M, kind, df, ds, dz, dR, dw, db, dpb, dout, dpc, dchi));
    if (out) CPI_TRY(st.download(out, (const double *)dout, (size_t)S * 136));
    if (pcost) CPI_TRY(st.download(pcost, (const double *)dpc, (size_t)S));
    if (dchi) CPI_TRY(st.download(chi2, (const double *)dchi, (size_t)M));
    return st.finish();
}

// cpi_state_between_batch from host memory: every array a host array, staged whole, synchronous.  mfirst and the state indices are
// validated first.  hess == hess_base / chi2 == chi2_base (in place) run in place on the staged copy.
extern "C" int cpi_state_between_batch_host(cpi_ctx *ctx, int64_t F, int64_t M, int32_t kind, const int64_t *mfirst,
                                            const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                            const double *z, const double *R, const double *weight,
                                            const double *hess_base, const double *chi2_base,
                                            double *hess, double *chi2, double *chi2_m) {
    static const char who[] = "cpi_state_between_batch_host";
    CPI_TRY(between_check(ctx, who, F, M, kind, mfirst, states, S, idx_i, idx_j, z, R, weight, hess_base, chi2_base, hess, chi2, chi2_m));
    for (int64_t f = 0; f < F; f++)
        if (mfirst[f] < 0 || mfirst[f + 1] > M || mfirst[f + 1] < mfirst[f])
            return refuse(ctx, who, ("the measurements of factor " + std::to_string(f) + " leave [0, M] or mfirst decreases there").c_str());
    if (F > 0) CPI_TRY(check_state_indices(ctx, who, F, S, idx_i, idx_j));
    if (!ctx) return fail(nullptr, CPI_ERR_INVALID, "ctx is NULL");
    if (F == 0) return CPI_OK;
    DeviceGuard guard_;
    CPI_HIP(ctx, guard_.enter(ctx->device));
    Staging st(ctx);
    const int64_t *df;
    const int32_t *di, *dj;
    const double *ds, *dz, *dR, *dw, *db = nullptr, *dcb = nullptr;
    double *dh = nullptr, *dc = nullptr, *dm = nullptr;
    CPI_TRY(st.upload(mfirst, (size_t)F + 1, &df));
    CPI_TRY(st.upload(states, (size_t)S * 16, &ds));
    CPI_TRY(st.upload(idx_i, (size_t)F, &di));
    CPI_TRY(st.upload(idx_j, (size_t)F, &dj));
    CPI_TRY(st.upload(M > 0 ? z : nullptr, (size_t)M * kBetweenZ[kind], &dz));
    CPI_TRY(st.upload(M > 0 ? R : nullptr, (size_t)M * kBetweenR[kind], &dR));
    CPI_TRY(st.upload(M > 0 ? weight : nullptr, (size_t)M, &dw));
    if (hess) {
        CPI_TRY(st.upload(hess_base, (size_t)F * 496, &db));
        if (hess == hess_base) dh = const_cast<double *>(db); else CPI_TRY(st.alloc((size_t)F * 496, &dh));
    }
    if (chi2) {
        CPI_TRY(st.upload(chi2_base, (size_t)F, &dcb));
        if (chi2 == chi2_base) dc = const_cast<double *>(dcb); else CPI_TRY(st.alloc((size_t)F, &dc));
    }
    if (chi2_m && M > 0) CPI_TRY(st.alloc((size_t)M, &dm));
    if (!dh && !dc && !dm) return st.finish();    // chi2_m alone with M == 0: nothing to write
    CPI_TRY(cpi_state_between_batch(ctx, F, M, kind, df, ds, S, di, dj, dz, dR, dw, db, dcb, dh, dc, dm));
    if (hess) CPI_TRY(st.download(hess, (const double *)dh, (size_t)F * 496));
    if (chi2) CPI_TRY(st.download(chi2, (const double *)dc, (size_t)F));
    if (dm) CPI_TRY(st.download(chi2_m, (const double *)dm, (size_t)M));
    return st.finish();
}
