// cpi_args.hpp -- kernel argument blocks and the launcher interface between the translation units of libcpi_amd.so.
//
// The library is twenty translation units, compiled in parallel by cpi_amd/build.py and linked into one shared object:
//   cpi_mean.hip    cpi_mean_kernel / cpi_mean_tiled_kernel / cpi_tile_*_kernel       (cpi_mean_kernels.hpp)
//   cpi_running.hip cpi_mean_running_kernel / cpi_mean_stream_running_kernel: a row after every interval, from plain knots /
//                   from windows cut out of IMU stream(s) in place         (cpi_running_kernels.hpp, cpi_running_body.inc)
//   cpi_cov.hip     cpi_cov_kernel<1|2> / cpi_forster_kernel / cpi_cov_running_kernel  (cpi_cov_kernels.hpp)
//   cpi_running_resume.hip  cpi_mean_running_carry_kernel / cpi_cov_running_carry_kernel: the running rows from and to carry
//                   records, over the bodies of the two units above (cpi_running_body.inc, cov_body)
//   cpi_running_resume_stj.hip  cpi_cov_running_stj_carry_kernel: cov_body with the read-out of model 2's Discrete_J_b columns after
//                   every interval for windows that continue from carry records (cpi_running_resume_stj_batch)
//   cpi_query.hip   cpi_query_kernel: the measurement at arbitrary times inside a window, one partial interval from a running row
//                                                    (cpi_query_kernels.hpp: query_mean_body; cpi_query_locate.hpp)
//   cpi_query_cov.hip  cpi_query_cov_kernel: the covariance at arbitrary times, one partial interval of the covariance recursion
//                   from a running P / P_sym row               (cpi_query_cov_kernels.hpp over cpi_covq_body.hpp; cpi_query_locate.hpp)
//   cpi_stj.hip     cpi_cov_running_stj_kernel / cpi_query_stj_kernel: model 2's bias Jacobians (the Discrete_J_b columns of cov_body)
//                   after every interval and at arbitrary times
//                                              (cpi_cov_kernels.hpp, cpi_stj_kernels.hpp: query_stj_body; cpi_query_locate.hpp)
//   cpi_query_stream.hip  cpi_squery_mean_kernel / cpi_squery_cov_kernel / cpi_squery_jac2_kernel: the three query kernels by
//                   ABSOLUTE time over IMU stream(s) read in place -- window lookup over the update times, search over the
//                   patched stamps of the cut, then the same bodies
//                                                    (cpi_query_stream_kernels.hpp: StreamLocator, over the three query bodies)
//   cpi_query_open.hip  cpi_query_open_kernel / cpi_query_cov_open_kernel / cpi_query_stj_open_kernel: the three query kernels for
//                   windows that continue from a carried state -- the same bodies, their i == 0 gather reading a base row
//                                                    (cpi_query_open_kernels.hpp over the three query bodies)
//   cpi_merge.hip   cpi_merge_kernel: consecutive preintegrated windows joined into one measurement, a segmented left fold over
//                   measurement rows (no IMU data is read)                             (cpi_merge_kernels.hpp)
//   cpi_trial.hip   cpi_retract_kernel / cpi_local_kernel / cpi_factor_cost_kernel / cpi_cost_*_kernel: the optimiser's trial step --
//                   states moved along a step, and the whitened cost of the factors there with its deterministic total
//                                                            (cpi_trial_kernels.hpp over cpi_factor_kernels.hpp's input fetch)
//   cpi_chain.hip   cpi_chain_solve_kernel: the damped block-tridiagonal solve of chains of IMU factors, on the rows of the Hessian
//                   sweep                                    (cpi_chain_kernels.hpp over cpi_factor_kernels.hpp's DPP multiply-adds)
//   cpi_marginals.hip  cpi_marginals_kernel: the state covariances of solved chains -- the diagonal and first off-diagonal blocks of
//                   the inverse, one backward recursion over the factor the solve left in the workspace
//                                   (cpi_marginals_kernels.hpp over cpi_factor_kernels.hpp's DPP multiply-adds; cpi_chain_util.hpp)
//   cpi_marginalize.hip  cpi_marginalize_kernel: the leading states of every chain eliminated into a prior on the first
//                   state that stays -- the forward half of the solve, undamped, no workspace
//                                 (cpi_marginalize_kernels.hpp over cpi_factor_kernels.hpp's DPP multiply-adds; cpi_chain_util.hpp)
//   cpi_condense.hip  cpi_condense_kernel / cpi_expand_kernel: chains cut into segments of K factors, every segment's interior states
//                   eliminated by a 16-lane group of its own into one 31 x 31 factor row between its ends, and the solution of the
//                   short chain of segment ends substituted back -- parallelism ALONG a chain
//                                   (cpi_condense_kernels.hpp over cpi_factor_kernels.hpp's DPP multiply-adds; cpi_chain_util.hpp)
//   cpi_lm.hip      cpi_lm_prior_kernel / cpi_lm_cost_kernel / cpi_lm_accept_kernel: the Levenberg-Marquardt step per chain -- the prior
//                   at the current states with its cost, the objective per chain, and the decision (accept, copy, lambda, phase)
//                                                                                  (cpi_lm_kernels.hpp; cpi_chain_util.hpp)
//   cpi_fix.hip     cpi_fix_kernel<kind>: absolute measurements of states (position, velocity, orientation, pose) added to their
//                   rows [Lam eta] and to their cost                                                   (cpi_fix_kernels.hpp)
//   cpi_between.hip cpi_between_kernel<kind>: measurements between the two states of an IMU factor (position, orientation, pose)
//                   added to the factor's 31 x 31 row and to its chi2                              (cpi_between_kernels.hpp)
//   cpi_factor.hip  evaluateError sweeps, square-root information, Hessian blocks, state prediction
//                                                                                      (cpi_factor_kernels.hpp)
//   cpi_abi.hip     the C-ABI of include/cpi_amd.h: argument checks, launch heuristics, device sets (RCCL), the
//                   host-pointer pipeline.  No kernels.
// A kernel TU exports plain host functions (namespace cpi::launch) that pick the template instantiation and enqueue it
// on the given stream; nothing else crosses a TU boundary (no relocatable device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/cpi_amd.h"

namespace cpi {

struct PreArgs {
    long long W;
    int N;
    const double *knots;
    const long long *first;
    const int *count;
    const double *lin;
    const double *qk;
    // Windows cut out of ONE IMU stream in flight (cpi_preintegrate_stream; GraphSolver_IMU.cpp:50-69): knots = the stream,
    // first[w] = the front reading of window w, count[w] = whole intervals + the partial tail interval; knot 0 of the window
    // carries the stamp tstart[w] instead of its own, and when tend[w] is not NaN the last interval is the tail
    // [stamp of the last real knot, tend[w]] with that knot's reading held.  Both NULL: plain knots.
    const double *tstart;
    const double *tend;
    // FUSED cut (mean-only requests of cpi_preintegrate_stream; cpi_mean_kernel<..., CUT = 2>): knots = the stream of K
    // readings, update[W] = the update times; every wavefront finds where the reference's deque stands for its own windows
    // (the arithmetic of cpi_cut_windows_kernel, in registers) and writes the TRUE interval count to count_out[W] --
    // first / count / tstart / tend stay NULL and no cut kernel runs.  K > 0 also tells a CUT = 1 launch where the stream
    // ends (fast addressing: a wavefront whose furthest read stays inside the stream needs no per-element pointers).
    const double *update;
    long long K;
    int *count_out;
    double grav[3];
    double q4[4];      // sigma^2 of the four diagonal blocks of Q_c (CpiBase.h:54-57)
    int write_means;   // kernel writes DT/alpha/beta/q
    int write_jac;     // kernel writes the Jacobians it owns
    int dbg;           // development switches of the experimental kernels (0 in every shipped path)
    cpi_outputs out;
};

// Resumable preintegration (cpi_preintegrate_resume): the carry record of a window (include/cpi_amd.h).  Offsets in doubles;
// the means block is written by whichever kernel owns the means of the call, the Jacobian block by the mean kernel, the
// covariance block by the covariance kernel.  R is column-major.
namespace carry {
static const int TAG = 0, DT = 1, ALPHA = 2, BETA = 5, R = 8, JAC = 17;   // JAC: J_q J_a J_b H_a H_b (O_a O_b) column-major
// tag bits: 1 always set, 2 = covariance state held, 4 = analytic Jacobians held, 8 = imu_avg, 16 = stj, 32 * model
static const int TAG_P = 2, TAG_J = 4, TAG_HDR = ~(TAG_P | TAG_J);
constexpr int cov_off(int model) { return JAC + (model == 2 ? 63 : 45); }
constexpr int doubles(int model) { return model == 1 ? 288 : (model == 2 ? cov_off(2) + 27 * 18 : 0); }
}  // namespace carry
struct CarryArgs {
    const double *in;   // [W][carry::doubles] or NULL = the zero state
    double *out;        // [W][carry::doubles]
    int need;           // tag bits carry_in must hold: the header + the parts this call continues
    int tag_out;        // the tag this call leaves (written by the owner of the means)
    int own_means;      // this kernel writes the tag and the means of the record
};

// Many IMU streams in one call (cpi_preintegrate_streams): run r owns the knots [soff[r], soff[r + 1]) of PreArgs::knots and the
// windows [uoff[r], uoff[r + 1]).  Both arrays live in device memory and are CLAMPED where they are read (cpi_mean_kernels.hpp:
// run_of / run_window): a wrong offset gives wrong windows, never an out-of-bounds read.  A separate kernel argument, so that
// PreArgs -- and with it the code of every existing kernel -- stays as it was.
struct RunArgs {
    const long long *soff;   // [R + 1]
    const long long *uoff;   // [R + 1]
    int R;                   // >= 1
};

// tiles[b][s][k][i] = field k (t, w, a) of knot s of window 64 b + i (include/cpi_amd.h: cpi_preintegrate_tiled_batch)
struct TiledArgs {
    long long W;
    int N;
    const double *tiles;
    const int *count;
    const double *lin;
    const double *qk;
    double grav[3];
    cpi_outputs out;
    int dbg;            // CPI_EXPERIMENTS builds only: 1 = fetch without arithmetic
    long long ts, ss;   // doubles between consecutive tiles / consecutive steps of a tile
};

// cpi_query_batch: query k asks for the measurement of window qwin[k] at time qtime[k]; rows = the W * N rows
// cpi_preintegrate_running wrote for the same windows (include/cpi_amd.h).  qwin lives in device memory and is CLAMPED into [0, W).
struct QueryArgs {
    long long W;
    int N;
    const double *knots;
    const long long *first;
    const int *count;
    const double *lin;
    const double *qk;
    double grav[3];
    cpi_outputs rows;      // DT / alpha / beta / q always; J_q ... H_b when out asks for them
    long long Q;
    const int *qwin;       // [Q]
    const double *qtime;   // [Q]
    int trips;             // ceil(log2(N + 1)): steps of the interval search, the same for every lane
    cpi_outputs out;       // arrays of Q rows
};

// cpi_query_open_batch: the state window w had BEFORE knot 0 of the queried segment = row w * N + N - 1 of every array of rows
// (ordinary rows, e.g. the previous chunk's).  It stands where the zero state stands in the closed entries.  A kernel argument of
// its own, so that QueryArgs -- and with it the code of every existing kernel -- stays as it was.
struct QueryBase {
    cpi_outputs rows;
    int N;                 // >= 1
};

// cpi_query_stream_batch: query k asks for the measurement of run qrun[k] at the ABSOLUTE time qtime[k]; the kernels find the
// window among the run's update times and the interval among the patched stamps of the cut (first / count / tstart / tend: the
// workspace of the stream entries, filled by the cut kernel in front of them); rows = the U * N rows of the running stream entries.
// qrun and uoff live in device memory and are CLAMPED where they are read.  A struct of its own, so that QueryArgs and PreArgs --
// and with them the code of every existing kernel -- stay as they were.
struct StreamQueryArgs {
    long long U;
    int N;
    const double *stream;    // [K][7], read in place
    long long K;
    const double *update;    // [U]
    const long long *uoff;   // [R + 1], or NULL: one run owning [0, U)
    int R;
    const long long *first;
    const int *count;
    const double *tstart;
    const double *tend;
    const double *lin;
    const double *qk;
    double grav[3];
    cpi_outputs rows;        // as QueryArgs::rows
    long long Q;
    const int *qrun;         // [Q] or NULL (run 0)
    const double *qtime;     // [Q]
    int *qwin_out;           // [Q] or NULL: the GLOBAL window found, -1 for a run without update times
    int wtrips;              // ceil(log2(U + 1)): steps of the window lookup, the same for every lane
    int trips;               // ceil(log2(N + 1)): steps of the interval search
    cpi_outputs out;         // arrays of Q rows
};

// cpi_merge_batch: output row j = in[first[j]] o in[first[j] + 1] o ... (count[j] consecutive rows, oldest first).  first and count
// live in device memory and are CLAMPED where they are read (cpi_merge_kernels.hpp: group_range).
struct MergeArgs {
    long long M;             // output rows (groups)
    int G;                   // the largest group, >= 1
    long long in_rows;
    cpi_outputs in;          // DT / alpha / beta / q always; J_q ... H_b and P or P_sym when the request needs them
    const long long *first;  // [M] or NULL: group j starts at row j * G
    const int *count;        // [M] or NULL: every group has G rows
    cpi_outputs out;         // arrays of M rows
};

struct FactorArgs {
    long long F;
    double grav[3];
    cpi_outputs meas;
    const double *lin;
    const double *qk;
    const double *states;
    long long S;               // number of states: indices are clamped into [0, S) (no out-of-bounds read whatever idx holds)
    const int *idx_i;
    const int *idx_j;
    double *err;
    double *H1;
    double *H2;
    const double *sqrt_info;   // optional [F][225] upper-triangular R: outputs are whitened (R err, R H1, R H2)
    int r_tri;                 // sqrt_info is the packed upper triangle [F][120] (include/cpi_amd.h: CPI_TRI_INDEX)
};

// cpi_chain_solve_batch: chain c owns the states [first[c], first[c] + count[c]) and the hess rows from ffirst[c] on.  first, count,
// ffirst and lambda live in device memory; the ranges are CLAMPED or refused where they are read (cpi_chain_kernels.hpp: chain_range).
struct ChainArgs {
    long long C;             // chains
    int G;                   // the longest chain in states, >= 1
    long long S, F;          // rows of delta / prior / workspace records; rows of hess
    const long long *first;  // [C] or NULL: chain c starts at state c * G
    const int *count;        // [C] or NULL: every chain has G states
    const long long *ffirst; // [C] or NULL: first[c] - c
    const double *hess;      // [F][496]
    const double *prior;     // [S][136] or NULL
    const double *lambda;    // [C] or NULL (0)
    int diagonal;            // CPI_DAMP_DIAGONAL
    double *delta;           // [S][15]
    int *status;             // [C] or NULL
    double *workspace;       // [S][chn::WS_D]
};

// cpi_chain_marginals_batch: C, G, S, first, count as the solve that wrote workspace had them (cpi_chain_util.hpp: chain_states).
struct MarginalsArgs {
    long long C;              // chains
    int G;                    // the longest chain in states, >= 1
    long long S;              // rows of workspace records / cov / cross
    const long long *first;   // [C] or NULL: chain c starts at state c * G
    const int *count;         // [C] or NULL: every chain has G states
    const int *status;        // [C] or NULL: as the solve wrote it; a chain whose status is not 0 gets NaN
    const double *workspace;  // [S][chn::WS_D], read only
    double *cov;              // [S][120]
    double *cross;            // [S][225] or NULL
};

// cpi_chain_marginalize_batch: the chains of cpi_chain_solve_batch (the same clamps), the leading drop[c] states of chain c eliminated
// into one prior row per chain.  drop lives in device memory; a value outside [0, n_c) refuses the chain where it is read.
struct MarginalizeArgs {
    long long C;             // chains
    int G;                   // the longest chain in states, >= 1
    long long S, F;          // rows of prior; rows of hess
    const long long *first;  // [C] or NULL: chain c starts at state c * G
    const int *count;        // [C] or NULL: every chain has G states
    const long long *ffirst; // [C] or NULL: first[c] - c
    const double *hess;      // [F][496]
    const double *prior;     // [S][136] or NULL
    int M;                   // states to eliminate where drop is NULL
    const int *drop;         // [C] or NULL
    double *out;             // [C][136]
    int *status;             // [C] or NULL
};

// cpi_chain_condense_batch: the chains of cpi_chain_solve_batch (the same clamps) cut into segments of K factors; Gr reduced states per
// chain slot (cpi_chain_condense_states(G, K)).  The reduced arrays are in the tile layout: state j of chain c at row c * Gr + j.
struct CondenseArgs {
    long long C;             // chains
    int G;                   // the longest chain in states, >= 1
    long long S, F;          // rows of prior / workspace records; rows of hess
    const long long *first;  // [C] or NULL: chain c starts at state c * G
    const int *count;        // [C] or NULL: every chain has G states
    const long long *ffirst; // [C] or NULL: first[c] - c
    const double *hess;      // [F][496]
    const double *prior;     // [S][136] or NULL
    const double *lambda;    // [C] or NULL (0)
    int diagonal;            // CPI_DAMP_DIAGONAL
    int K, Gr;               // factors per segment (1 <= K <= max(G - 1, 1)); reduced states per chain slot
    double *rhess;           // [C * (Gr - 1)][496]
    double *rprior;          // [C * Gr][136]
    int *rcount;             // [C]
    int *status;             // [C * (Gr - 1)] or NULL, per segment
    double *workspace;       // [S][chn::CS_D]; interior records only
};

// cpi_chain_expand_batch: C, G, S, first, count, K as the condense that wrote workspace had them.
struct ExpandArgs {
    long long C;
    int G;
    long long S;
    const long long *first;
    const int *count;
    int K, Gr;
    const double *rdelta;     // [C * Gr][15]: the reduced solve's delta
    const double *workspace;  // [S][chn::CS_D], read only
    double *delta;            // [S][15]
};

// cpi_prior_relinearize_batch: record p belongs to state idx[p] (NULL: p); an index outside [0, S) skips the record where it is read.
struct LmPriorArgs {
    long long S, P;
    const int *idx;          // [P] or NULL
    const double *states;    // [S][16]
    const double *anchor;    // [P][16]
    const double *prior0;    // [P][136]
    double *prior;           // [S][136] or NULL
    double *pcost;           // [S] or NULL
};

// cpi_chain_cost_batch / cpi_chain_accept_batch: the chains of cpi_chain_solve_batch (the same clamps; cpi_chain_util.hpp: chain_range).
struct LmCostArgs {
    long long C;             // chains
    int G;                   // the longest chain in states, >= 1
    long long S, F;          // rows of pcost / states; rows of chi2
    const long long *first;  // [C] or NULL: chain c starts at state c * G
    const int *count;        // [C] or NULL: every chain has G states
    const long long *ffirst; // [C] or NULL: first[c] - c
    const double *chi2;      // [F] or NULL (G == 1); the trial's chi2 for the accept kernel
    const double *pcost;     // [S] or NULL; the trial's for the accept kernel
    double *cost;            // [C]: out (cost), in/out (accept)
};
struct LmAcceptArgs {
    cpi_lm_params p;         // validated by the entry (include/cpi_amd.h)
    const double *trial;    // [S][16]
    double *states;          // [S][16] in/out
    double *chi2;            // [F] in/out or NULL
    double *lambda;          // [C] in/out
    int *phase;              // [C] in/out
    int *accepted;           // [C] or NULL
};

// cpi_state_fix_batch: state s owns the fixes mfirst[s] .. mfirst[s + 1] - 1 (clamped into [0, M] where they are read).
struct FixArgs {
    long long S, M;
    const long long *mfirst; // [S + 1]
    const double *states;    // [S][16]
    const double *z;         // [M][3 | 3 | 4 | 7]
    const double *R;         // [M][6 | 6 | 6 | 21]
    const double *weight;    // [M] or NULL
    const double *base;      // [S][136] or NULL
    const double *pcost_base;// [S] or NULL
    double *out;             // [S][136] or NULL
    double *pcost;           // [S] or NULL
    double *chi2;            // [M] or NULL
};

// cpi_state_between_batch: factor f owns the measurements mfirst[f] .. mfirst[f + 1] - 1 (clamped into [0, M] where they are read)
// between the states idx_i[f] and idx_j[f] (f and f + 1 where NULL; clamped into [0, S)).
struct BetweenArgs {
    long long F, M, S;
    const long long *mfirst; // [F + 1]
    const double *states;    // [S][16]
    const int *idx_i, *idx_j;// [F] or NULL
    const double *z;         // [M][3 | 4 | 7]
    const double *R;         // [M][6 | 6 | 21]
    const double *weight;    // [M] or NULL
    const double *hess_base; // [F][496] or NULL; == hess: the in-place form
    const double *chi2_base; // [F] or NULL
    double *hess;            // [F][496] or NULL
    double *chi2;            // [F] or NULL
    double *chi2_m;          // [M] or NULL
};

struct PredictArgs {
    long long F;
    double grav[3];
    cpi_outputs meas;
    const double *states_i;
    long long S;
    const int *idx_i;
    double *states_j;
};

// Window assembly on the device (cpi_assemble_tiles, include/cpi_amd.h): one IMU stream cut at update times straight into
// the tiled layout.
struct AssembleArgs {
    long long K;            // knots of the stream
    const double *stream;   // [K][7]
    long long U;            // windows
    const double *update;   // [U] update times, non-decreasing
    int N;                  // rows of a tile - 1 (>= the largest count)
    double *tiles;          // [ceil(U/64)][N+1][7][64]
    int *count;             // [U]
    long long ts, ss;
};

namespace launch {
// ---- cpi_mean.hip
bool mean_lanes_supported(int L);
int mean_lane_choices(const int **list);   // the supported L values, ascending
void mean(int model, bool jac, bool avg, int L, const PreArgs &a, hipStream_t st);
void mean_carry(int model, bool jac, bool avg, int L, const PreArgs &a, const CarryArgs &c, hipStream_t st);
// S wavefronts per tile (1 = one wavefront owns the tile; > 1 = SPLIT); big_lds_set: per-context bit set of the
// instantiations whose dynamic-LDS limit was already raised
hipError_t mean_tiled(int model, bool avg, bool counted, int S, const TiledArgs &a, hipStream_t st, unsigned *big_lds_set);
void tile_knots(long long W, int N, const double *knots, const long long *first, const int *count, double *tiles, hipStream_t st);
void assemble_tiles(const AssembleArgs &a, hipStream_t st);
void cut_windows(long long K, const double *stream, long long U, const double *update, int N, long long *first, int *count,
                 double *tstart, double *tend, hipStream_t st);
// cpi_preintegrate_streams: the cut of cut_windows for windows of many runs, and the fused mean-only kernel (CUT = 3)
void cut_runs(long long K, const double *stream, long long U, const double *update, const RunArgs &r, long long *first, int *count,
              double *tstart, double *tend, hipStream_t st);
void mean_runs(int model, bool avg, int L, const PreArgs &a, const RunArgs &r, hipStream_t st);
// ---- cpi_running.hip (cpi_preintegrate_running: a.out holds W * N rows; L: any of mean_lane_choices)
void mean_running(int model, bool jac, bool avg, int L, const PreArgs &a, hipStream_t st);
// cpi_preintegrate_stream[s]_running: the same rows for the windows that cut_windows / cut_runs left in a.first / count / tstart /
// tend; a.knots = the stream of a.K readings, read in place
void mean_stream_running(int model, bool jac, bool avg, int L, const PreArgs &a, hipStream_t st);
// ---- cpi_cov.hip
void cov_running(int model, bool avg, const PreArgs &a, hipStream_t st);   // P / P_sym rows only
void cov(int model, bool avg, const PreArgs &a, hipStream_t st);
void cov_carry(int model, bool avg, const PreArgs &a, const CarryArgs &c, hipStream_t st);
void forster(const PreArgs &a, hipStream_t st);
// ---- cpi_running_resume.hip (cpi_preintegrate_running_resume: the running rows from c.in to c.out)
void mean_running_carry(int model, bool jac, bool avg, int L, const PreArgs &a, const CarryArgs &c, hipStream_t st);   // always owns tag + means of c.out
void cov_running_carry(int model, bool avg, const PreArgs &a, const CarryArgs &c, hipStream_t st);   // P / P_sym rows + the covariance block of c.out
// ---- cpi_running_resume_stj.hip (cpi_running_resume_stj_batch, model 2: cov_running_carry + the rows of J_q ... O_b that a.out asks for)
void cov_running_carry_stj(bool avg, const PreArgs &a, const CarryArgs &c, hipStream_t st);
// ---- cpi_query.hip (cpi_query_batch; jac: model 1 only)
void query(int model, bool jac, bool avg, const QueryArgs &a, hipStream_t st);
// ---- cpi_query_cov.hip (cpi_query_cov_batch: a.out.P / P_sym from a.rows.q and a.rows.P or P_sym; q4 as PreArgs::q4)
void query_cov(int model, bool avg, const QueryArgs &a, const double q4[4], hipStream_t st);
// ---- cpi_stj.hip (model 2; cpi_running_stj_batch: cov_running + the rows of J_q ... O_b that a.out asks for;
// cpi_query_stj_batch: a.out.J_q ... O_b from a.rows.q and all seven Jacobian fields of a.rows)
void cov_running_stj(bool avg, const PreArgs &a, hipStream_t st);
void query_stj(bool avg, const QueryArgs &a, hipStream_t st);
// ---- cpi_query_open.hip (cpi_query_open_batch: query / query_cov / query_stj with b standing where the zero state stood)
void query_open(int model, bool jac, bool avg, const QueryArgs &a, const QueryBase &b, hipStream_t st);
void query_cov_open(int model, bool avg, const QueryArgs &a, const double q4[4], const QueryBase &b, hipStream_t st);
void query_stj_open(bool avg, const QueryArgs &a, const QueryBase &b, hipStream_t st);
// ---- cpi_query_stream.hip (cpi_query_stream_batch: the three launchers above over StreamQueryArgs; each writes a.qwin_out when set)
void squery_mean(int model, bool jac, bool avg, const StreamQueryArgs &a, hipStream_t st);
void squery_cov(int model, bool avg, const StreamQueryArgs &a, const double q4[4], hipStream_t st);
void squery_jac2(bool avg, const StreamQueryArgs &a, hipStream_t st);
// ---- cpi_merge.hip (cpi_merge_batch; jac: a.out asks for a Jacobian, cov: a.out asks for P / P_sym)
void merge(bool jac, bool cov, const MergeArgs &a, hipStream_t st);
// ---- cpi_trial.hip (cpi_retract_batch, cpi_local_batch, cpi_factor_cost[_tri]_batch; a.sqrt_info / a.r_tri say where R is)
void retract(long long S, const double *states_in, const double *delta, double *states_out, hipStream_t st);
void local_coordinates(long long S, const double *x, const double *other, double *xi, hipStream_t st);
void factor_cost(int model, int lpf, const FactorArgs &a, double *chi2, double *werr, hipStream_t st);   // lpf 16 | 8 | 4
size_t cost_total_doubles(long long F);
void cost_total(long long F, const double *chi2, double *workspace, hipStream_t st);   // workspace[0] = 0.5 sum chi2
// ---- cpi_chain.hip (cpi_chain_solve_batch)
size_t chain_workspace_doubles(long long S);
void chain_solve(const ChainArgs &a, hipStream_t st);
// ---- cpi_marginals.hip (cpi_chain_marginals_batch)
void chain_marginals(const MarginalsArgs &a, hipStream_t st);
// ---- cpi_marginalize.hip (cpi_chain_marginalize_batch)
void chain_marginalize(const MarginalizeArgs &a, hipStream_t st);
// ---- cpi_condense.hip (cpi_chain_condense_batch, cpi_chain_expand_batch)
size_t condense_workspace_doubles(long long S);
long long condense_groups(long long C, int Gr);   // 16-lane groups of a launch, 4 per workgroup
void chain_condense(const CondenseArgs &a, hipStream_t st);
void chain_expand(const ExpandArgs &a, hipStream_t st);
// ---- cpi_lm.hip (cpi_prior_relinearize_batch, cpi_chain_cost_batch, cpi_chain_accept_batch)
void lm_prior(const LmPriorArgs &a, hipStream_t st);
void lm_cost(const LmCostArgs &a, hipStream_t st);
void lm_accept(const LmCostArgs &a, const LmAcceptArgs &b, hipStream_t st);
// ---- cpi_fix.hip (cpi_state_fix_batch)
void state_fix(int kind, const FixArgs &a, hipStream_t st);                                   // kind: CPI_FIX_*
// ---- cpi_between.hip (cpi_state_between_batch)
void state_between(int kind, const BetweenArgs &a, hipStream_t st);                           // kind: CPI_BETWEEN_*
// ---- cpi_factor.hip
void factor(int model, bool whiten, int lpf, const FactorArgs &a, hipStream_t st);            // lpf 16 | 8 | 4
void factor_packed(int model, int lpf, const FactorArgs &a, double *packed, hipStream_t st);  // lpf 2 | 3 | 4 | 6 | 8
void factor_hessian(int model, const FactorArgs &a, double *hess, hipStream_t st);
void sqrt_info(long long F, const double *P, double *R, bool packed, hipStream_t st);   // packed: P_sym [F][120] -> R_tri [F][120]
void predict(int model, const PredictArgs &a, hipStream_t st);
#ifdef CPI_TEST_HOOKS
void test_quat_ops(int op, long long n, const double *in, double *out, hipStream_t st);   // libcpi_amd_test.so only
#endif
void unpack_slabs(int n, const long long *lo, const long long *cnt, const long long *wb, const double *staging, long long stride,
                  const cpi_outputs &root_out, hipStream_t st);
#ifdef CPI_EXPERIMENTS
// measurement-only kernels (cpi_mean_experimental.hpp; tools/exp/): never part of the default build
struct MeanDmaCfg { int kc, s, aligned; };
long long mean_dma(int model, const MeanDmaCfg &c, bool avg, const PreArgs &a, hipStream_t st);   // leading windows handled
bool mean_blk(int model, int L, bool avg, const PreArgs &a, hipStream_t st);
long long mean_line(int model, bool avg, const PreArgs &a, hipStream_t st);                       // leading windows handled
void tiled_fetch_probe(const TiledArgs &a, size_t lds, hipStream_t st);
#endif
}  // namespace launch
}  // namespace cpi
