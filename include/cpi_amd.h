/*
 * cpi_amd.h -- C-ABI of the MI355X-native batched continuous-preintegration engine.
 *
 * This is the drop-in boundary for the rpng/cpi hot path.  The reference has no FFI layer: the
 * boundary there is two C++ class interfaces compiled into the caller,
 *   - the preintegrator  CpiBase / CpiV1 / CpiV2   (cpi_compare/src/cpi/CpiBase.h:40-145,
 *     CpiV1.h:62, CpiV2.h:84): ctor(sigmas, imu_avg), setLinearizationPoints(), feed_IMU() called
 *     once per IMU interval (GraphSolver_IMU.cpp:50-69), results read from public members
 *     (GraphSolver_IMU.cpp:74-75,129-130);
 *   - the factor  ImuFactorCPIv1/v2::evaluateError(state_i, state_j, H1, H2)
 *     (cpi_compare/src/gtsam/ImuFactorCPIv1.h:139 / .cpp:37, ImuFactorCPIv2.h:151 / .cpp:38),
 *     called by GTSAM once per factor per re-linearisation.
 * The entry points below are the batched equivalents a binding of those two interfaces would call
 * (see INTEGRATION.md for the reference-side stub).  Plain pointers and sizes only.
 *
 * Conventions
 *   - all arithmetic is IEEE double; all pointers are DEVICE pointers unless the name says _host;
 *   - every 3x3 / 15x15 matrix is COLUMN-MAJOR (Eigen's default, so Eigen::Map works unchanged);
 *   - quaternions are JPL [x y z w] with w >= 0 (quat_ops.h:80-82);
 *   - error-state / tangent order is [theta b_g v b_a p] (ImuFactorCPIv1.cpp:80);
 *   - JPLNavState is 16 doubles [q(4) b_g(3) v(3) b_a(3) p(3)] (JPLNavState.h:62-66);
 *   - calls on one cpi_ctx are ordered on its HIP stream and return without synchronising;
 *     distinct contexts (one per GPU / per stream) are independent.  No global state.
 */
#ifndef CPI_AMD_H
#define CPI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPI_ABI_VERSION 3   /* 3 (round 6): cpi_outputs gained a 13th field, P_sym (the covariance as its packed upper triangle) -- a binding
                               built against version 2 passes a 12-field struct and must be rebuilt; new symbols
                               cpi_sqrt_information_packed_batch, cpi_factor_eval_whitened_tri_batch, cpi_factor_hessian_tri_batch,
                               cpi_group_gather_chunk, cpi_shard_chunk_bounds; this number also records round 4's workspace-contract
                               change of cpi_preintegrate_stream (below), which version 2 carried only in prose.
                               2: state count S in the factor / predict entries; device-set entries (cpi_group_*);
                               additions within 2 (new symbols only): tiled layout entries, cpi_host_alloc / _free;
                               round 3: cpi_preintegrate_stream (+ _workspace_bytes, _counts), cpi_tile_windows,
                               cpi_assemble_tiles, cpi_preintegrate_tiled_batch_host,
                               cpi_outputs_slab_doubles / _bind_slab, cpi_group_last_gather_messages,
                               cpi_preintegrate_stream_host;
                               round 4, a CONTRACT change without a new symbol: after cpi_preintegrate_stream the workspace
                               holds the true interval counts (cpi_stream_counts) and NOTHING ELSE a caller may read -- a
                               mean-only request runs no cut kernel, so the first / tstart / tend records round 3 left there
                               are no longer written (they were never declared);
                               additions within 3 (new symbols only): cpi_carry_doubles, cpi_preintegrate_resume,
                               cpi_preintegrate_resume_host (resumable preintegration); cpi_streams_workspace_bytes,
                               cpi_preintegrate_streams, cpi_preintegrate_streams_host (many IMU streams in one call);
                               cpi_preintegrate_running, cpi_preintegrate_running_host (the measurement after every interval);
                               cpi_preintegrate_stream_running, cpi_preintegrate_streams_running,
                               cpi_preintegrate_stream_running_host, cpi_preintegrate_streams_running_host (the running rows
                               from IMU stream(s), windows cut in place); cpi_preintegrate_running_resume,
                               cpi_preintegrate_running_resume_host (the running rows of a window that continues from a
                               carry record); cpi_query_batch, cpi_query_batch_host (the measurement at arbitrary times inside
                               a window); cpi_query_cov_batch, cpi_query_cov_batch_host (the same with the covariance P / P_sym
                               at the query times); cpi_running_stj_batch, cpi_running_stj_batch_host,
                               cpi_query_stj_batch, cpi_query_stj_batch_host (model 2's seven bias Jacobians after every
                               interval and at the query times); cpi_stream_running_stj_batch,
                               cpi_stream_running_stj_batch_host (those rows from IMU stream(s), cut in place);
                               cpi_query_stream_batch, cpi_query_stream_batch_host (the query family by absolute time over IMU
                               stream(s): the window and the interval are found on the device);
                               cpi_running_resume_stj_batch, cpi_running_resume_stj_batch_host (model 2's Jacobian rows from a
                               carry record); cpi_query_open_batch, cpi_query_open_batch_host (the query family for a window
                               that continues from a carried state, given as a base row); cpi_merge_batch, cpi_merge_batch_host
                               (consecutive preintegrated windows joined into one measurement: a segmented fold over measurement
                               rows, no IMU data); cpi_retract_batch, cpi_local_batch, cpi_factor_cost_batch,
                               cpi_factor_cost_tri_batch, cpi_factor_cost_total_doubles and the host forms
                               cpi_retract_batch_host, cpi_local_batch_host, cpi_factor_cost_batch_host (the optimiser's trial
                               step: the states moved along a solved step, and the whitened cost 0.5 |R e|^2 of the factors at
                               the trial states with a deterministic total); cpi_chain_solve_batch,
                               cpi_chain_solve_workspace_doubles, cpi_chain_solve_batch_host (the damped block-tridiagonal
                               solve of chains of IMU factors on the rows of cpi_factor_hessian_*: the step of the loop above);
                               cpi_chain_marginals_batch, cpi_chain_marginals_batch_host (the state covariances of solved
                               chains: the diagonal and first off-diagonal blocks of the inverse, from the factor the solve
                               left in its workspace); cpi_chain_marginalize_batch, cpi_chain_marginalize_batch_host (the
                               oldest states of a chain eliminated into a prior on the first state that stays: the step of a
                               fixed-lag smoother between two optimisations); cpi_chain_condense_states,
                               cpi_chain_condense_workspace_doubles, cpi_chain_condense_batch, cpi_chain_expand_batch,
                               cpi_chain_condense_batch_host, cpi_chain_expand_batch_host (segment condensation: the interior
                               states of every run of K factors eliminated in parallel into one factor row between its ends,
                               and the back-substitution: parallelism along a chain); cpi_prior_relinearize_batch,
                               cpi_chain_cost_batch, cpi_chain_accept_batch, cpi_prior_relinearize_batch_host,
                               cpi_chain_cost_batch_host, cpi_chain_accept_batch_host (the Levenberg-Marquardt
                               step per chain on the device: the prior at the current states with its cost, the objective
                               per chain, and the decision -- accept or reject, copy, lambda, phase);
                               cpi_state_fix_batch, cpi_state_fix_batch_host (absolute measurements of states --
                               position, velocity, orientation, pose fixes -- added to their rows [Lam eta] and to their
                               cost: how a GPS fix, a zero-velocity update or a mocap pose enters that loop);
                               cpi_state_between_batch, cpi_state_between_batch_host (measurements between the two
                               consecutive states an IMU factor joins -- relative position, orientation, pose -- added to
                               the factor's row of cpi_factor_hessian_* and to its chi2: how odometry enters that loop) */

enum { CPI_OK = 0, CPI_ERR_INVALID = 1, CPI_ERR_HIP = 2, CPI_ERR_NO_DEVICE = 3, CPI_ERR_RCCL = 4 };
enum {
    CPI_MODEL_V1 = 1, CPI_MODEL_V2 = 2,
    /* cpi_preintegrate_batch only: the "Forster discrete" comparator, i.e. what GraphSolver::createimufactor_discrete
     * (GraphSolver_IMU.cpp:141-232) gets from GTSAM's PreintegratedCombinedMeasurements (manifold preintegration),
     * already converted the way that call site does it: alpha = deltaPij, beta = deltaVij,
     * q = rot_2_quat(deltaRij^T), J_q = -delRdelBiasOmega, J_a / J_b = delP / delV delBiasOmega,
     * H_a / H_b = delP / delV delBiasAcc, P = preintMeasCov with blocks 1 and 4 swapped (swapcovariance :240-254)
     * = order [theta b_g v b_a p].  Reading i is held over [t_i, t_i+1] (no averaging: imu_avg, q_k_lin, grav,
     * lanes_per_window are ignored).  The result is the measurement of an ImuFactorCPIv1 (:227-231): evaluate it
     * with model CPI_MODEL_V1.  GTSAM is not part of the reference tree: parity of this model is UNPINNED
     * (oracle/forster_oracle.c). */
    CPI_MODEL_FORSTER = 3
};

typedef struct cpi_ctx cpi_ctx;

/* Replaces: CpiBase ctor arguments (CpiBase.h:52), the imu_avg flag (CpiBase.h:95), the
 * state_transition_jacobians flag (CpiV2.h:58) and the gravity passed to setLinearizationPoints
 * (CpiBase.h:73-80; one global gravity per batch, as in Config.h / GraphSolver_IMU.cpp:44). */
typedef struct {
    double sigma_w, sigma_wb, sigma_a, sigma_ab;
    double grav[3];
    int32_t model;                       /* CPI_MODEL_V1 | CPI_MODEL_V2 | CPI_MODEL_FORSTER (preintegration only) */
    int32_t imu_avg;                     /* 0 / 1 */
    int32_t state_transition_jacobians;  /* model 2 only; reference default 1 */
    int32_t lanes_per_window;            /* mean kernel: 0 = auto, else 1,2,3,4,5,6,8,12,16,32,64 (tuning knob;
                                            ignored by the covariance kernel and by model 2 with analytic Jacobians).
                                            cpi_preintegrate_tiled_batch reads it as WAVEFRONTS PER TILE: 0 = auto, else 1..8 */
} cpi_params;

/* Replaces: the public result members of CpiBase / CpiV2 (CpiBase.h:99-124, CpiV2.h:62-63).
 * Structure-of-arrays over the W windows of a batch; any pointer may be NULL = "not wanted":
 *   DT, alpha, beta, q all NULL      -> means are not written
 *   J_q ... O_b all NULL             -> bias / orientation Jacobians are not computed
 *   P and P_sym both NULL            -> the covariance recursion is skipped (mean-only kernel) */
typedef struct {
    double *DT;     /* [W]       CpiBase::DT        */
    double *alpha;  /* [W][3]    alpha_tau          */
    double *beta;   /* [W][3]    beta_tau           */
    double *q;      /* [W][4]    q_k2tau            */
    double *J_q;    /* [W][9]    orientation wrt b_w */
    double *J_a;    /* [W][9]    alpha wrt b_w      */
    double *J_b;    /* [W][9]    beta wrt b_w       */
    double *H_a;    /* [W][9]    alpha wrt b_a      */
    double *H_b;    /* [W][9]    beta wrt b_a       */
    double *O_a;    /* [W][9]    alpha wrt q_k_lin (model 2) */
    double *O_b;    /* [W][9]    beta wrt q_k_lin  (model 2) */
    double *P;      /* [W][225]  P_meas, dense column-major (the drop-in form: Eigen::Map<Matrix<double,15,15>>) */
    double *P_sym;  /* [W][120]  P_meas as its packed upper triangle (CPI_TRI_INDEX below; P_meas is symmetric -- the
                                 reference itself asserts it, CpiV1.h:352-353 -- so the dense form carries 105 redundant doubles
                                 = 840 of the 2 248 bytes a model-1 window writes with everything out).  P and P_sym are independent: either, both or
                                 neither; the entries of P_sym are bit for bit the entries (i, j), i <= j, of P */
} cpi_outputs;

/* Packed triangles (ABI 3).  A symmetric 15 x 15 matrix (P_meas) is stored as its upper triangle, an upper-triangular one (the
 * square-root information R) as its non-zero part, both COLUMN by column -- LAPACK's packed 'U' order, the order
 * cpi_factor_hessian_batch already writes its 31 x 31 triangle in:
 *     entry (i, j), i <= j, at  CPI_TRI_INDEX(i, j) = i + j (j + 1) / 2,      120 doubles = 960 bytes instead of 1 800.
 * Column j is the run [j (j + 1) / 2, j (j + 1) / 2 + j].  INTEGRATION.md section 4a shows the Eigen one-liners
 * (selfadjointView<Upper> / triangularView<Upper>) a GTSAM-side binding unpacks them with; cpi_amd.unpack_sym / unpack_tri /
 * pack_sym are the Python mirrors. */
#define CPI_TRI_DOUBLES 120
#define CPI_TRI_INDEX(i, j) ((i) + (j) * ((j) + 1) / 2)

/* device < 0: use the current HIP device.  stream: a hipStream_t (NULL = the default stream). */
int cpi_ctx_create(int device, void *stream, cpi_ctx **out);
void cpi_ctx_destroy(cpi_ctx *ctx);
/* Later calls on ctx are issued on `stream` (a hipStream_t of the context's device).  The caller orders the two streams. */
int cpi_ctx_set_stream(cpi_ctx *ctx, void *stream);
/* Captured batch calls.  While ctx's stream is being captured into a HIP graph, consecutive cpi_preintegrate_batch calls that
 * issue one kernel (means, or means + analytic Jacobians; no covariance) are left UNORDERED in the graph, up to `depth` of them at
 * a time, when the library can prove from the arguments that the memory they touch is disjoint: no array one call writes
 * (W x n x 8 bytes per non-NULL output) overlaps an array the other reads or writes (knots, lin, q_k_lin, count, outputs).
 * Their kernels may then run concurrently when the graph is replayed.  What a caller may rely on:
 *   - results are bit for bit those of the serial order (calls that share memory stay ordered; a call with a `first` array,
 *     whose knot span the host cannot see, is ordered against everything);
 *   - everything the caller captures on the stream before such calls happens before them, and everything captured after them
 *     (any other entry of this library, a copy, a kernel, an event record, hipStreamEndCapture) happens after ALL of them;
 *   - at most `depth` calls are in flight; call i is ordered behind call i - depth and everything before it;
 *   - eager (non-captured) execution is never relaxed.
 * depth 1 = every node depends on the previous one (the shape before this entry existed); clamped to [1, 4]; 2 is the fastest
 * depth measured (profiles/capture_overlap.md).  This "look-back" shape is an opt-in: through this entry, or through
 * CPI_AMD_CAPTURE_OVERLAP=<depth> read once by cpi_ctx_create; a new context starts with the strand shape of
 * cpi_ctx_set_capture_strands below, which gives every call ONE predecessor and was measured faster.  A process that sets GPU_MAX_HW_QUEUES below 4 keeps depth 1
 * (parallel branches of a graph need four hardware queues); the library never sets that variable.  Two cases keep the serial
 * shape because overlap was measured not to pay there (profiles/capture_overlap.md): launches of more than one wavefront per
 * SIMD (1 024 wavefronts), and captures in which several contexts of the process take part (the caller spread the calls by hand).  A caller that writes one of
 * the arrays from ANOTHER stream of the same capture orders the streams with events as before. */
int cpi_ctx_set_capture_overlap(cpi_ctx *ctx, int32_t depth);
/* The same relaxation in another graph shape, and the one a new context starts with: `n` STRANDS (clamped to [1, 4]; 1 = the
 * serial chain).  Every captured call of the kind above gets exactly one predecessor: the last call of the one strand whose
 * calls (all of them, since the strands were last joined) touch memory that conflicts with its own, or of the least recently
 * extended strand when it conflicts with none.  A call that conflicts with several strands, or whose footprint the host cannot
 * bound while several strands are in use, joins them: it follows the last call of every strand and everything later follows it.
 * The guarantees are those listed above, with "at most n calls are in flight" in place of the depth's.
 * cpi_ctx_set_capture_overlap selects the look-back shape, this entry the strand shape; the later call holds.  At cpi_ctx_create:
 * GPU_MAX_HW_QUEUES below 4 keeps the chain; else CPI_AMD_CAPTURE_STRANDS=<n> selects strands; else CPI_AMD_CAPTURE_OVERLAP=<depth>
 * selects the look-back shape (=2 is the graph of the library before this entry existed); neither set: 4 strands, the fastest
 * measured on 10 000-window batches (profiles/capture_strands.md). */
int cpi_ctx_set_capture_strands(cpi_ctx *ctx, int32_t n);
const char *cpi_last_error(const cpi_ctx *ctx); /* ctx may be NULL: last error of a failed create */
int cpi_abi_version(void);
const char *cpi_build_id(void);   /* sha256[:16] of the sources this library was built from (cpi_amd/build.py: source_id) */
int cpi_ctx_synchronize(cpi_ctx *ctx);

/* Replaces: the per-window loop  CpiV{1,2} cpi(...); cpi.setLinearizationPoints(...);
 *           while (...) cpi.feed_IMU(t0,t1,w0,a0,w1,a1);   (GraphSolver_IMU.cpp:43-69, 97-124).
 *
 * knots   IMU knot records {t, w[3], a[3]} (7 doubles).  Interval i of a window is
 *         feed_IMU(t_i, t_{i+1}, w_i, a_i, w_{i+1}, a_{i+1}); intervals with t_{i+1}-t_i <= 0 are
 *         skipped exactly like the reference (dt==0: CpiV1.h:72; dt<0: GraphSolver_IMU.cpp:52).
 *         A tail interval [t_last, updatetime] is expressed by a final knot
 *         {updatetime, w_last, a_last} (GraphSolver_IMU.cpp:64-69).  A knot whose t is NaN is a
 *         separator: both intervals touching it are skipped, so non-chained feed_IMU calls
 *         (the reference only ever uses t_1 - t_0) can be expressed in one window.  Skipped intervals
 *         are run as dt = 0 (an exact no-op of the arithmetic, no divergence): their READINGS must be
 *         finite -- the separators the facades emit carry zeros.
 * first   [W] index of each window's first knot, or NULL for the dense layout knots[W][N+1][7].
 * count   [W] number of intervals of each window (<= N), or NULL = every window has N.  Values outside
 *         [0, N] are clamped into it by the kernels (the array lives in HBM and cannot be validated by the call).
 *         Windows may share knots (consecutive windows cut from one stream).
 * N       maximum number of intervals per window.
 * lin     [W][6]  {b_w_lin[3], b_a_lin[3]}  (CpiBase.h:113-114)
 * q_k_lin [W][4]  JPL q_GtoK linearisation orientation (CpiBase.h:115); required for model 2.
 * Zero-length windows produce the identity / zero state.  W == 0 is a no-op. */
int cpi_preintegrate_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                           const double *knots, const int64_t *first, const int32_t *count,
                           const double *lin, const double *q_k_lin, const cpi_outputs *out);

/* Resumable preintegration -- the incremental object of the reference (CpiBase::feed_IMU, CpiBase.h:99-124) for a batch:
 * continue each window from a carried state and hand the state back.
 *
 * Call A on the knots [k0 .. km] of a window, then call B with carry_in = A's carry_out on [km .. kn]: B's outputs are the
 * measurement of ALL the intervals so far and equal one cpi_preintegrate_batch call on [k0 .. kn] (up to the rounding of a
 * different association; a NULL carry_in reproduces cpi_preintegrate_batch bit for bit).  Consecutive segments share their
 * boundary knot (imu_avg needs it).  knots / first / count / N, dt <= 0 and NaN separators as in cpi_preintegrate_batch;
 * a segment with count 0 passes the state through.  lin, q_k_lin, the sigmas, grav, model, imu_avg and
 * state_transition_jacobians must stay the same along a chain (setLinearizationPoints comes before the first feed_IMU).
 *
 * carry_in   [W][cpi_carry_doubles(model)] or NULL = the zero state (CpiBase constructor)
 * carry_out  [W][cpi_carry_doubles(model)], required; must not overlap carry_in (the two kernels of a model-1 "everything"
 *            call run concurrently and both read carry_in)
 * out        as in cpi_preintegrate_batch; the means are computed into carry_out even when out asks for none.
 * CPI_MODEL_FORSTER, carry_out == NULL and overlapping carry ranges return CPI_ERR_INVALID.  No host synchronisation:
 * the device entry can be captured into a graph.
 *
 * The carry record is opaque to callers; for binding authors (doubles, matrices column-major):
 *   [0]        tag: an integer-valued double, 1 + 2 (covariance state held) + 4 (analytic Jacobians held) + 8 imu_avg
 *              + 16 state_transition_jacobians + 32 model.  0 and NaN are never valid.
 *   [1]        DT          [2..4] alpha     [5..7] beta     [8..16] R, the rotation the recursion carries (never a quaternion)
 *   [17..]     J_q J_a J_b H_a H_b (+ O_a O_b, model 2), 9 each: when the call computes the analytic Jacobians
 *   [62..286]  model 1: P, 15 x 15                                              (when the call runs the covariance kernel)
 *   [80..565]  model 2: the 18 carried rows of the 18 covariance columns and of the 9 Discrete_J_b columns, 18 doubles per
 *              column in the kernel's column order (the theta_klin unit block stays implicit)
 * A call needs the parts it continues: the covariance state when it runs the covariance kernel (P / P_sym wanted, or model 2
 * Jacobians with state_transition_jacobians), the analytic Jacobians when it computes them.  A window whose carry_in tag
 * lacks a needed part or differs in model / imu_avg / state_transition_jacobians gets NaN in all its requested outputs and
 * in its carry_out (the host cannot see device data: this is the guard against a silently wrong continuation); the other
 * windows are unaffected. */
size_t cpi_carry_doubles(int32_t model);   /* doubles per window of a carry record: 288 (model 1), 566 (model 2); 0 otherwise */
int cpi_preintegrate_resume(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                            const double *knots, const int64_t *first, const int32_t *count,
                            const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                            const cpi_outputs *out);

/* Running preintegration -- the measurement after EVERY interval: the reference's public members (DT, alpha_tau, beta_tau,
 * q_k2tau, the bias Jacobians, P_meas) as they stand after each feed_IMU, for a batch of windows in one call.
 *
 * Arguments as cpi_preintegrate_batch.  `rows` is an ordinary cpi_outputs whose arrays hold W * N rows: row w * N + i is what
 * cpi_preintegrate_batch returns for window w cut after interval i (intervals 0 .. i), up to the rounding of a different
 * association.  Row offsets are computed in 64 bits.
 *   - a skipped interval (dt <= 0, a NaN-stamp separator) is an exact no-op: its row repeats the previous row bit for bit (row
 *     0 of such a window is the zero state: DT = 0, alpha = beta = 0, q = [0 0 0 1], Jacobians and P zero);
 *   - rows i >= count[w] repeat the window's final state, so row w * N + N - 1 is always the window's measurement; count is
 *     clamped into [0, N]; count = 0 gives N zero-state rows;
 *   - any pointer of rows may be NULL with the meaning it has in cpi_outputs; P and P_sym are independent, and a P_sym row is
 *     bit for bit the upper triangle of the P row.
 * Models 1 and 2, imu_avg 0 / 1, dense and ragged (first / count) layouts; lanes_per_window is honoured by the mean kernel.
 * Means for both models, the five analytic bias Jacobians for model 1, the covariance for both models.  CPI_ERR_INVALID:
 * CPI_MODEL_FORSTER, and any Jacobian field (J_q ... O_b) with model 2 (its Jacobians are read out of the state transition
 * matrix at the end of the recursion).  W == 0 or N == 0 is a no-op; N <= 65535 and the 32-bit grid limit on W as in
 * cpi_preintegrate_batch.  No host synchronisation and a single stream: the call can be captured into a graph.
 * Composition: with F = W * N and idx_i[row] = row / N, cpi_predict_batch turns the rows into IMU-rate predicted states.
 * Running rows from IMU stream(s), windows cut in place: cpi_preintegrate_stream_running / cpi_preintegrate_streams_running below.
 * Running rows of a window that is still open (from and to a carry record): cpi_preintegrate_running_resume below.
 * Running Jacobian rows for model 2 (state_transition_jacobians): cpi_running_stj_batch below. */
int cpi_preintegrate_running(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                             const double *knots, const int64_t *first, const int32_t *count,
                             const double *lin, const double *q_k_lin, const cpi_outputs *rows);

/* Running preintegration from a carry record -- IMU-rate rows for windows that are still open: the IMU readings arrive in
 * chunks, every call integrates the new intervals only, writes one row per new interval and hands the state back.  The union of
 * the two contracts above, nothing else:
 *   - knots / first / count / N / lin / q_k_lin, dense and ragged layouts, dt <= 0, NaN-stamp separators, clamping of count into
 *     [0, N], models 1 and 2, imu_avg 0 / 1, lanes_per_window (0 = the choice cpi_preintegrate_running makes), N <= 65535 and
 *     the 32-bit grid limit on W: as cpi_preintegrate_running;
 *   - carry_in (NULL = the zero state), carry_out (required, must not overlap carry_in: both kernels read carry_in and write
 *     disjoint parts of carry_out), the record layout, the tag rules and what must stay the same along a chain: as
 *     cpi_preintegrate_resume.  Consecutive segments share their boundary knot.
 *   - rows holds W * N rows, 64-bit offsets.  Row w * N + i is the measurement of ALL intervals integrated so far: those the
 *     record stands for plus intervals 0 .. i of this segment.
 *   - a skipped interval repeats the previous row bit for bit.  The "previous row" of row 0 is the CARRIED state read out as a
 *     row: DT, alpha, beta of the record, q = rot_2_quat(R) of the record's rotation, the record's five Jacobians (model 1), P /
 *     P_sym read out of the record's covariance state as the running kernel reads out a row.  With carry_in == NULL that is the
 *     zero-state row of cpi_preintegrate_running.  Rows i >= count[w] repeat the final state, so row w * N + N - 1 is always the
 *     state carry_out holds; count = 0 gives N copies of the carried row and passes the state through.
 *   - carry_out describes exactly the state of row N - 1: its DT / alpha / beta are bit for bit that row's, rot_2_quat of its R
 *     is bit for bit that row's q, its Jacobians (model 1, when computed) are that row's, and the P read out of its covariance
 *     state is that row's P.  An all-skipped segment fed with this record therefore reproduces the last row of the call that
 *     wrote it: "repeats the previous row" holds across calls.
 *   - requests: means for both models, the five analytic bias Jacobians for model 1, P and / or P_sym for both models.  Any
 *     Jacobian field with model 2, and CPI_MODEL_FORSTER, return CPI_ERR_INVALID.  Every pointer of rows may be NULL: nothing is
 *     written to rows, carry_out still receives the means.
 *   - tags: the call needs, and leaves, header | covariance state (P or P_sym wanted) | analytic Jacobians (model-1 Jacobian
 *     rows wanted) -- the rule of cpi_preintegrate_resume.  The records of the two resume entries are interchangeable in both
 *     directions, so a chain may mix them: running rows while the window is open, and one final cpi_preintegrate_resume on a
 *     segment of 0 intervals to read model 2's Jacobians out of the carried state-transition columns (the chain must then have
 *     asked for P or P_sym throughout, and state_transition_jacobians must be set).
 *   - a window whose carry_in tag lacks a needed part or differs in model / imu_avg / state_transition_jacobians gets NaN in ALL
 *     N rows of every requested field (all four components of q) and a NaN tag in carry_out; the other windows are unaffected.
 *   - W == 0 is a no-op.  N == 0 writes no rows and passes every window's state through to carry_out (the zero state for a
 *     NULL carry_in): a caller never holds an undefined record.
 *   - the kernels run one after the other on the context's stream: no side stream, no host synchronisation; a capture of the
 *     call is a chain without parallel branches.
 *   - with carry_in == NULL the rows are bit for bit those of cpi_preintegrate_running on the same arguments, for every model,
 *     request and lanes_per_window.
 * Not provided: running Jacobian rows for model 2; running rows from a carry record for the STREAM entries
 * (cpi_preintegrate_stream[s]_running); the Forster comparator.  (Model 2's running Jacobian rows without a carry record:
 * cpi_running_stj_batch below; from a carry record: cpi_running_resume_stj_batch below.) */
int cpi_preintegrate_running_resume(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                    const double *knots, const int64_t *first, const int32_t *count,
                                    const double *lin, const double *q_k_lin,
                                    const double *carry_in, double *carry_out, const cpi_outputs *rows);

/* The measurement at ARBITRARY TIMES inside a window: a camera, a lidar point or a rolling-shutter row stamped between two IMU
 * readings, a keyframe time chosen after the fact, the poses at the 100 k point times of one lidar sweep for deskewing.  The rows
 * of cpi_preintegrate_running hold the state after every interval, so a query is one gather and at most one partial interval
 * instead of a window of its own re-integrated from the start.  The semantics are the reference's own: GraphSolver_IMU.cpp:64-69
 * closes a window at `updatetime` by holding the front reading over [t_front, updatetime]; a query is that tail interval applied
 * to a running row.
 *
 *   prm, W, N, knots, first, count, lin, q_k_lin   the arguments of the cpi_preintegrate_running call that wrote rows
 *   rows    W * N rows, the output of cpi_preintegrate_running on THOSE arguments: DT, alpha, beta, q always; J_q ... H_b where
 *           out asks for the same field
 *   Q, qwin [Q], qtime [Q]   query k asks for window qwin[k] at time qtime[k]; any order, repeats allowed
 *   out     arrays of Q rows; any pointer may be NULL = "not wanted"
 * Query k: let w = qwin[k], n = the window's count clamped into [0, N], t_0 .. t_n its knot stamps, t_q = qtime[k].
 *   - PRECONDITION: the stamps t_0 .. t_n of a queried window are finite and non-decreasing (NaN-stamp separators are not
 *     supported here).  Otherwise the result of that query is unspecified -- but even then no read leaves the window's knots
 *     [k0, k0 + n] or its rows [w N, w N + N);
 *   - i = the largest index in [0, n] with t_i <= t_q; t_q < t_0: i = 0 and nothing is integrated;
 *   - base state = the zero-state row (DT = 0, alpha = beta = 0, q = [0 0 0 1], Jacobians 0) when i == 0, else row w N + i - 1;
 *   - i < n and t_q > t_i: the base state advanced by feed_IMU(t_i, t_q, w_i, a_i, w_i, a_i) -- reading i held, as for the
 *     reference's tail; the rotation is rebuilt from the row's quaternion (quat_2_Rot);
 *   - otherwise (t_q == t_i, or t_q >= t_n: there is no extrapolation) the base state, COPIED BIT FOR BIT in every requested field;
 *   - t_q NaN: NaN in every requested field of that query (all four components of q);
 *   - out[k] equals cpi_preintegrate_batch on the window [knot 0 .. knot i, {t_q, w_i, a_i}] up to rounding.
 * Requests: DT / alpha / beta / q for models 1 and 2, imu_avg 0 / 1; J_q J_a J_b H_a H_b for model 1.  CPI_ERR_INVALID: P / P_sym
 * in out, any Jacobian field with model 2, CPI_MODEL_FORSTER, model 2 without q_k_lin, a NULL prm / rows / out / qwin / qtime / lin /
 * knots, a rows without DT / alpha / beta / q or without a Jacobian field out asks for (N > 0), negative sizes, W == 0 with Q > 0,
 * N > 65535, Q > 2^31 - 1, an unsupported lanes_per_window (validated as elsewhere, otherwise ignored).  Q == 0 is a no-op.
 * N == 0: every query gets the zero state and rows is not read.
 * qwin lives in device memory and cannot be validated by the call: the kernel CLAMPS it into [0, W) -- a wrong index gives a
 * wrong row, never an out-of-bounds read.  cpi_query_batch_host validates it.
 * One kernel on the context's stream, no host synchronisation: the call can be captured into a graph (after the
 * cpi_preintegrate_running that feeds it: a chain without parallel branches).
 * Composition: cpi_predict_batch(F = Q, meas = out, idx_i = qwin) gives the predicted states AT the query times.
 * Not provided: P / P_sym at query times (they need the covariance kernel's lane-spread RK4 step); Jacobians for model 2; windows
 * cut from IMU streams in place (cpi_preintegrate_stream[s]_running: assemble the windows, or query per update time); rows that
 * continue from a carry record (cpi_preintegrate_running_resume); extrapolation past t_n.  (The covariance at query times is a
 * call of its own: cpi_query_cov_batch below; the Jacobians of model 2 at query times: cpi_query_stj_batch below; streams
 * queried in place by absolute time: cpi_query_stream_batch below; rows that continue from a carry record: cpi_query_open_batch
 * below.) */
int cpi_query_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                    const double *knots, const int64_t *first, const int32_t *count,
                    const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                    int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);

/* cpi_query_batch WITH THE COVARIANCE: the noise model of a keyframe stamped between two IMU readings, or chosen after the fact,
 * so that the factor at a query time can be whitened (cpi_sqrt_information_*) and enter cpi_factor_hessian_* -- without
 * preintegrating a cut copy of the window from its start.  A superset of cpi_query_batch: the arguments, the choice of i, the
 * precondition on the stamps, the clamping of qwin on the device, "no read leaves the window's knots or rows", Q == 0, N == 0, a NaN
 * t_q and every refusal of cpi_query_batch (with its text) are the same, except that out may also hold
 *   out->P [Q][225] and / or out->P_sym [Q][120] (independent of each other), for models 1 and 2, imu_avg 0 / 1, dense and ragged
 *   layouts.
 * The mean and Jacobian fields of out are written by cpi_query_batch's own kernel under cpi_query_batch's requirements on rows and
 * are bit for bit what cpi_query_batch writes; with neither P nor P_sym in out the call IS cpi_query_batch.
 * With P or P_sym in out, rows must hold (N > 0) q and P or P_sym -- CPI_ERR_INVALID names what is missing -- and nothing else: the
 * partial interval needs of the row only its rotation (DT / alpha / beta only when out asks for a mean field).  Query k, with i as
 * in cpi_query_batch:
 *   - base matrix S = zeros when i == 0, else row w N + i - 1 of rows->P; when only rows->P_sym is given, that row mirrored across
 *     the diagonal (rows->P is preferred when both are given);
 *   - no step (t_q on a stamp, before t_0, at or past t_n): out->P[k] = S and out->P_sym[k] = its upper triangle, BIT FOR BIT (i == 0:
 *     all +0);
 *   - step (i < n and t_q > t_i): S propagated by the reference's covariance step (RK4, four stages) over feed_IMU(t_i, t_q, w_i,
 *     a_i, w_i, a_i); the rotation at the start of the interval is quat_2_Rot of the row's q ([0 0 0 1] for i == 0), and R(q_k_lin) g
 *     enters for model 2 as it does elsewhere.  Model 2 carries 18 rows and columns (the theta clone): after every interval the
 *     reference clones and marginalises, so at a row boundary they are determined by the 15 x 15 row -- rows 15..17 of every column
 *     are its rows 0..2, columns 15..17 are columns 0..2 -- and are rebuilt from it.  out->P_sym[k] is bit for bit the upper triangle
 *     of out->P[k], and out->P[k] equals the P of cpi_preintegrate_batch on [knot 0 .. knot i, {t_q, w_i, a_i}] up to rounding;
 *   - t_q NaN: NaN in all 225 / 120 entries.
 * The kernels (cpi_query_batch's for the means, one more for the covariance) run one after the other on the context's stream: no
 * side stream, no host synchronisation; a capture of cpi_preintegrate_running followed by this call is a chain without parallel
 * branches.
 * Composition: out->P_sym -> cpi_sqrt_information_packed_batch -> cpi_factor_eval_whitened_tri_batch / cpi_factor_hessian_tri_batch
 * with idx_i = qwin: the whitened keyframe factor AT the query time.
 * Still not provided: model-2 Jacobians at query times; windows cut from IMU streams in place; rows from a carry record;
 * extrapolation past t_n.  (The model-2 Jacobians at query times are a call of their own: cpi_query_stj_batch below; streams queried in
 * place by absolute time: cpi_query_stream_batch below; rows from a carry record: cpi_query_open_batch below.) */
int cpi_query_cov_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                        const double *knots, const int64_t *first, const int32_t *count,
                        const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                        int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);

/* cpi_preintegrate_running WITH MODEL 2's JACOBIAN ROWS: J_q J_a J_b H_a H_b O_a O_b after every interval, so that a model-2 factor
 * can be closed at any IMU reading (evaluateError of model 2 needs all seven).  A superset of cpi_preintegrate_running: the
 * arguments and every rule of its contract are the same.  Without a Jacobian field in rows, or with model 1, the call IS
 * cpi_preintegrate_running (the same kernels, bit for bit the same rows).
 * With model 2, state_transition_jacobians != 0 and any of J_q ... O_b in rows: row w * N + i of each requested field is what
 * cpi_preintegrate_batch (state_transition_jacobians = 1) returns for window w cut after interval i -- the read-out of the nine
 * transition columns of Discrete_J_b (b_w, b_a, theta_klin) that the covariance kernel does at the end of a window, done after
 * every interval, with its signs and blocks (J_q = -theta rows of the b_w columns, ...).  The running contract holds for these rows
 * as it stands: a skipped interval repeats the previous row bit for bit, rows i >= count[w] repeat the final state, row 0 of a window
 * that has integrated nothing is all zeros, count is clamped into [0, N], dense and ragged layouts, imu_avg 0 / 1, 64-bit row
 * offsets.  The transition columns ride on the covariance recursion, so the covariance kernel runs whether or not P / P_sym are
 * asked for; the mean rows and the P / P_sym rows of the call are bit for bit those of cpi_preintegrate_running on the same
 * arguments.
 * CPI_ERR_INVALID beyond cpi_preintegrate_running's: model 2 with state_transition_jacobians == 0 and a Jacobian field (the analytic
 * O_a / O_b recursion has no running form).  CPI_MODEL_FORSTER is refused as there.
 * No host synchronisation and a single stream: a capture of the call is a chain without parallel branches.
 * Still not provided: these rows for the stream entries (cpi_preintegrate_stream[s]_running); for the carry-record entries
 * (cpi_preintegrate_running_resume); model 2's analytic Jacobians (state_transition_jacobians == 0); extrapolation past t_n.
 * (From IMU stream(s) cut in place: cpi_stream_running_stj_batch below; from a carry record: cpi_running_resume_stj_batch below.) */
int cpi_running_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                          const double *knots, const int64_t *first, const int32_t *count,
                          const double *lin, const double *q_k_lin, const cpi_outputs *rows);

/* cpi_query_cov_batch WITH MODEL 2's JACOBIANS: everything a model-2 keyframe factor at a query time needs, in one call.  A
 * superset of cpi_query_cov_batch: the arguments, the choice of i, the precondition on the stamps, the clamping of qwin on the device,
 * "no read leaves the window's knots or rows", Q == 0, N == 0, a NaN t_q are the same; the mean fields and P / P_sym are written by
 * the kernels of cpi_query_batch / cpi_query_cov_batch and are bit for bit what those entries write; model-1 Jacobians are handled as
 * there; with no model-2 Jacobian field in out the call IS cpi_query_cov_batch.
 * With model 2, state_transition_jacobians != 0 and any of J_q ... O_b in out: rows -- written by cpi_running_stj_batch on the
 * same arguments -- must hold (N > 0) q and ALL SEVEN Jacobian fields, whatever subset out asks for (CPI_ERR_INVALID names what is
 * missing).  Query k, with i as in cpi_query_batch:
 *   - no step (t_q on a stamp, before t_0, at or past t_n): the Jacobians of row w N + i - 1 copied BIT FOR BIT; zeros when i == 0;
 *   - step (i < n and t_q > t_i): the nine transition columns are rebuilt from row w N + i - 1 -- at a row boundary they are
 *     determined by the seven matrices: b_w column c = [-J_q[:,c] | e_c | J_b[:,c] | 0 | J_a[:,c] | -J_q[:,c]], b_a column c =
 *     [0 | 0 | H_b[:,c] | e_c | H_a[:,c] | 0], theta_klin column c = [0 | 0 | O_b[:,c] | 0 | O_a[:,c] | 0] over the rows [theta | b_w |
 *     v | b_a | p | theta clone]; i == 0: the initial state -- and advanced by the reference's RK4 step over feed_IMU(t_i, t_q, w_i,
 *     a_i, w_i, a_i) with the start rotation quat_2_Rot of the row's q, then read out as at the end of a window.  The result equals
 *     cpi_preintegrate_batch (state_transition_jacobians = 1) on [knot 0 .. knot i, {t_q, w_i, a_i}] up to rounding;
 *   - t_q NaN: NaN in every requested field.
 * CPI_ERR_INVALID beyond cpi_query_cov_batch's: model 2 with state_transition_jacobians == 0 and a Jacobian field in out.
 * The kernels run one after the other on the context's stream: no side stream, no host synchronisation; a capture of
 * cpi_running_stj_batch followed by this call is a chain without parallel branches.
 * Composition: out (means, seven Jacobians, P_sym) -> cpi_sqrt_information_packed_batch -> cpi_factor_eval_whitened_tri_batch /
 * cpi_factor_hessian_tri_batch with model 2 and idx_i = qwin.
 * Still not provided: windows cut from IMU streams in place (the stream entries); rows that continue from a carry record
 * (cpi_preintegrate_running_resume); model 2's analytic Jacobians (state_transition_jacobians == 0); extrapolation past t_n.
 * (Streams queried in place by absolute time: cpi_query_stream_batch below; rows that continue from a carry record:
 * cpi_query_open_batch below.) */
int cpi_query_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                        const double *knots, const int64_t *first, const int32_t *count,
                        const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                        int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);

/* cpi_preintegrate_running_resume WITH MODEL 2's JACOBIAN ROWS: the seven matrices after every interval of a window that is still
 * open, so that a live model-2 estimator gets them per IMU reading and not only at a chunk's end.  A superset of
 * cpi_preintegrate_running_resume, as cpi_running_stj_batch is of cpi_preintegrate_running: the arguments and every rule of its
 * contract are the same.  Without a Jacobian field in rows, or with model 1, the call IS cpi_preintegrate_running_resume (the same
 * kernels, bit for bit the same rows and records).
 * With model 2, state_transition_jacobians != 0 and any of J_q ... O_b in rows: row w * N + i of each requested field is the
 * read-out of the nine Discrete_J_b transition columns behind interval i of this segment, continued from the columns carry_in
 * holds -- exactly the read-out of cpi_running_stj_batch.  The covariance kernel runs whether or not P / P_sym are asked for.
 *   - tags: the call needs, and leaves, header | covariance state (the transition columns are part of it).  The tag, NaN and
 *     pass-through rules of cpi_preintegrate_running_resume hold unchanged.
 *   - the running contract holds for the new rows: a skipped interval repeats the previous row bit for bit, the "previous row" of
 *     row 0 is the carried columns read out, rows i >= count[w] repeat the final state, count = 0 gives N copies of the carried
 *     read-out, and a window whose record does not fit gets NaN in all N rows of every requested field.  A call with N = 1 and
 *     every count 0 therefore reads a record out as one ordinary row per window (it reads knot first[w] of each window and nothing
 *     behind it): the base row of cpi_query_open_batch.
 *   - carry_in == NULL gives bit for bit the rows of cpi_running_stj_batch.  The mean and P / P_sym rows and carry_out are bit
 *     for bit those of cpi_preintegrate_running_resume on the same arguments (with P or P_sym in rows), so records stay
 *     interchangeable with both older resume entries, and a zero-interval cpi_preintegrate_resume on carry_out returns the seven
 *     matrices of row N - 1 bit for bit: both read the same columns the same way.
 * CPI_ERR_INVALID beyond cpi_preintegrate_running_resume's: model 2 with state_transition_jacobians == 0 and a Jacobian field.
 * CPI_MODEL_FORSTER is refused as there.
 * One stream, no host synchronisation: a capture of the call is a chain without parallel branches.
 * Still not provided: carry records for the stream entries; model 2's analytic Jacobians in running form
 * (state_transition_jacobians == 0); extrapolation past t_n. */
int cpi_running_resume_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                 const double *knots, const int64_t *first, const int32_t *count,
                                 const double *lin, const double *q_k_lin,
                                 const double *carry_in, double *carry_out, const cpi_outputs *rows);

/* cpi_query_stj_batch FOR A WINDOW THAT IS STILL OPEN: a camera frame stamped inside the IMU chunk that has just arrived, of a
 * window that continues from a carried state.  The arguments of cpi_query_stj_batch -- knots, first, count, rows describe the
 * SEGMENT (the chunk), rows being what a resume entry (cpi_preintegrate_running_resume, cpi_running_resume_stj_batch) wrote for
 * it -- plus
 *   base, base_N   the state each window had BEFORE knot 0 of the segment, as ordinary rows: the row of window w is row
 *                  w * base_N + base_N - 1 of every array of base.  base_N = 1: W contiguous rows (what an N = 1, all-counts-0 call
 *                  of cpi_running_resume_stj_batch writes from the record).  base_N = the previous chunk's N: the previous call's
 *                  rows used in place, without a gather -- that row is the one its carry_out describes.
 * No record is parsed here: the base row stands where the zero state stands in the closed entries.  The semantics are the
 * family's with "the zero state when i == 0" read as "the base row of window w":
 *   - a query on or before the segment's first stamp (t_q <= t_0) returns the base row BIT FOR BIT in every requested field;
 *   - a query inside interval 0 advances the base row by feed_IMU(t_0, t_q, w_0, a_0, w_0, a_0): the means, model 1's Jacobians, P
 *     (the clone rows and columns rebuilt as for any row) and model 2's nine columns (rebuilt from the base row's seven matrices as
 *     for any row);
 *   - i > 0 is unchanged, and so are the clamping of qwin, Q == 0, a NaN t_q, and "no read leaves the window's knots, its rows, or
 *     row w * base_N + base_N - 1 of base".  N == 0: every query gets the base row and rows is not read;
 *   - a gathered state (row or base) whose q[0] is NaN -- the rows a refused carry leaves -- gives NaN in every requested field of
 *     that query (all four components of q).
 * base must hold what rows must hold for the same request (for every N); CPI_ERR_INVALID names base and what is missing.
 * base_N < 1 with a non-NULL base is refused.  base == NULL: the call IS cpi_query_stj_batch, bit for bit.
 * On a view of a closed window -- first + m, count - m, rows m ..., base = row m - 1 -- the call returns bit for bit what
 * cpi_query_stj_batch returns on the whole window for every t_q >= t_m: the arithmetic behind the gather is the same code.
 * The kernels run one after the other on the context's stream; a capture of cpi_running_resume_stj_batch followed by this call
 * is a chain without parallel branches.
 * Composition: out -> cpi_sqrt_information_packed_batch -> cpi_factor_eval_whitened_tri_batch with idx_i = qwin.
 * Still not provided: carry records for the stream entries; model 2's analytic Jacobians in running form; extrapolation past t_n. */
int cpi_query_open_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                         const double *knots, const int64_t *first, const int32_t *count,
                         const double *lin, const double *q_k_lin, const cpi_outputs *rows,
                         int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out,
                         const cpi_outputs *base, int32_t base_N);

/* Consecutive preintegrated windows JOINED: from the measurements of [t0, t1], [t1, t2], ... to the measurement of [t0, tn], without
 * the IMU readings.  Keyframe decimation (camera-rate windows of one cpi_preintegrate_stream call turned into keyframe-rate windows),
 * keyframe removal (a state leaves a smoother and the two IMU factors that met at it become one), and the building block of a
 * parallel-in-time integration.  A segmented left fold over measurement rows:
 *     out row j = in[first[j]] o in[first[j] + 1] o ... o in[first[j] + count[j] - 1]        (oldest first)
 *   in      in_rows measurement rows, ordinary cpi_outputs arrays: what cpi_preintegrate_batch / _stream / ... wrote
 *   M, G    M output rows (groups); G >= 1 is the largest group
 *   first   [M] first input row of each group, or NULL: group j is the rows [j G, j G + count[j])
 *   count   [M] rows of each group, or NULL: every group has G rows.  Clamped into [0, G]; a group is clipped at in_rows (first is
 *           clamped into [0, in_rows]): both arrays live in device memory and cannot be validated by the call -- a wrong value gives a
 *           wrong row, never a read outside in.  Groups may share and skip rows
 *   out     arrays of M rows; any pointer may be NULL = "not wanted"; P and P_sym are independent, and a P_sym row is bit for bit the
 *           upper triangle of the P row
 * The composition, for A (earlier) followed by B (later), R_X = quat_2_Rot(q_X), error-state order [theta b_g v b_a p]:
 *     DT = DT_A + DT_B      R = R_B R_A, q = rot_2_quat(R)  (the sign and branch preintegration itself would emit)
 *     beta = beta_A + R_A^T beta_B                          alpha = alpha_A + beta_A DT_B + R_A^T alpha_B
 *     J_q = R_B J_q_A + J_q_B                               H_b = H_b_A + R_A^T H_b_B
 *     J_b = J_b_A + R_A^T (J_b_B + [beta_B x] J_q_A)        H_a = H_a_A + DT_B H_b_A + R_A^T H_a_B
 *     J_a = J_a_A + DT_B J_b_A + R_A^T (J_a_B + [alpha_B x] J_q_A)
 *     P = Phi~ P_A Phi~^T + T P_B T^T, then 0.5 (P + P^T):  T = blkdiag(I, I, R_A^T, I, R_A^T), Phi~ = T Phi(B) T^T, and Phi(B) = the
 *         identity plus the blocks (theta,theta) R_B - I, (theta,b_g) -J_q, (v,theta) -[beta x], (v,b_g) J_b, (v,b_a) H_b,
 *         (p,theta) -[alpha x], (p,b_g) J_a, (p,v) DT I, (p,b_a) H_a of B -- the state transition rebuilt from B's public fields.
 *         The (v,v) and (p,p) blocks of Phi~ are I and its (p,v) block is DT_B I BY CONSTRUCTION: the products R_A^T I R_A and
 *         R_A^T (DT_B I) R_A are never formed.
 * Operand quaternions are taken AS GIVEN and not normalised: R_X = quat_2_Rot(q_X) is orthonormal only as far as q_X is unit.  A q
 * off unit by eps (| |q|^2 - 1 | = eps; 6e-8 for a q that went through float32) moves the joined means and Jacobians by O(eps)
 * times their size: the caller's input error, passed on and not amplified.  With the three blocks above held at I, I and DT_B I the
 * covariance of such operands stays the covariance of the NORMALISED quaternions to O(eps) as well (a fold of 8 float32 operands: 4e-7
 * relative; the dense triple product would put R_A^T R_A there and be ten times further off).  The q written for a joined row is normalised, with w >= 0.  -q is the same
 * operand as q (quat_2_Rot is even in q): every output is the same bit for bit.  A zero-state row among the operands (first, last or
 * inside a group) is the identity of the composition: every field but q comes out bit for bit as without it, q to rounding.
 * The means and Jacobians equal one preintegration of the joined window up to rounding; P equals it up to the RK4 truncation of the
 * reference's own covariance recursion (about 1e-8 relative to sqrt(P_ii P_jj) at 200 Hz and ordinary rates; it grows like
 * (|w| dt)^5).
 * CONTRACT: all windows of a group were preintegrated at the SAME linearisation point {b_w_lin, b_a_lin}, with the same sigmas and
 * imu_avg.  The call cannot see lin: rows of different lin compose into numbers that are no measurement of anything (as a chain of
 * resume calls must keep lin, cpi_preintegrate_resume).
 *   - count = 0 writes the zero-state row of cpi_preintegrate_running: DT = 0, alpha = beta = 0, q = [0 0 0 1], Jacobians and P zero;
 *   - count = 1 copies the input row BIT FOR BIT in every requested field (q as it is, not requantised; with only P_sym in `in` the
 *     dense P is that triangle mirrored);
 *   - what out may ask for depends on what in holds (in_rows > 0): the means need DT alpha beta q; any Jacobian needs the means and
 *     all five Jacobians; P / P_sym need the means, all five Jacobians and P or P_sym (dense P is used when given, else the packed
 *     triangle).  A request without P / P_sym never reads in's P / P_sym; a request for the means alone reads the four mean fields
 *     alone.
 * Model 1 only.  Model 2 is not composable from its outputs: its alpha and beta carry gravity through each window's own q_k_lin, and
 * q_k_lin of window k + 1 is an estimate, not R_A (x) q_k_lin.  The Forster comparator's P does not come from this recursion.  Both
 * return CPI_ERR_INVALID, as do: in lacking a field the request needs, O_a or O_b in out, G < 1, M < 0 or in_rows < 0, an array of
 * out overlapping an array of in, a NULL in / out.  Every refusal comes before the context is looked at.  M == 0 is a no-op.  Row
 * offsets are computed in 64 bits.  One kernel on the context's stream, no host synchronisation: the call can be captured into a
 * graph.
 * Not provided: model 2 and the Forster comparator; rows of different lin; the inverse (taking a prefix away: the measurement
 * between two running rows). */
int cpi_merge_batch(cpi_ctx *ctx, int32_t model, int64_t M, int32_t G, int64_t in_rows, const cpi_outputs *in,
                    const int64_t *first /*[M] or NULL*/, const int32_t *count /*[M] or NULL*/, const cpi_outputs *out);

/* Replaces: the whole caller side of GraphSolver::createimufactor_cpi_v1 / _v2 (GraphSolver_IMU.cpp:43-75, 97-130) for every
 * window of a trajectory at once, reading ONE IMU stream IN PLACE: no knot is copied, for any model and any output.
 *   stream        [K][7] knot records {t, w[3], a[3]} in arrival order, stamps NON-DECREASING (device memory)
 *   update_times  [U] non-decreasing: window u covers (update_times[u-1], update_times[u]] exactly as the reference cuts it
 *                 (GraphSolver_IMU.cpp:50-69): whole intervals while imu_times[1] <= updatetime, then the partial tail interval
 *                 with the front reading held, after which the front stamp is overwritten by the update time; window 0 starts
 *                 at the stream's first reading
 *   N             upper bound of the intervals of a window (whole + tail); a longer window is truncated to N intervals --
 *                 check cpi_stream_counts, which holds the TRUE counts after the call.  Give a TIGHT bound: the kernels'
 *                 loops run to the longest window of a wavefront, but the automatic lane split of the mean kernel
 *                 (cpi_params.lanes_per_window = 0) is chosen from N, not from the counts
 *   lin, q_k_lin  per window, as in cpi_preintegrate_batch
 *   workspace     cpi_stream_workspace_bytes(U) bytes of device memory, 16-byte aligned (28 bytes per window: where the
 *                 reference's deque stands at each update, found by interpolation search because the stamps are sorted).
 *                 After the call it holds the TRUE interval counts (cpi_stream_counts); the rest of its contents is
 *                 unspecified: a mean-only request (DT / alpha / beta / q and nothing else, models 1 and 2) runs NO cut kernel --
 *                 every wavefront of the mean kernel finds its own windows in its prologue and only the counts are written
 * The kernels patch the first knot's stamp and build the tail interval's closing knot from its predecessor in flight.
 * The readings must be finite: a NaN / Inf reading invalidates (only) the windows that contain it.
 * Results are bit-identical to cpi_preintegrate_batch on the knots / first / count that the host assemblers
 * (cpi_amd/stream.py, cpi_host::assemble_windows) produce from the same stream. */
size_t cpi_stream_workspace_bytes(int64_t U);
int cpi_preintegrate_stream(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                            const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                            void *workspace, const cpi_outputs *out);
const int32_t *cpi_stream_counts(const void *workspace, int64_t U);   /* device pointer into the workspace: count[U] */

/* Many trajectories at once: cpi_preintegrate_stream for R runs (IMU streams) in ONE call, every window cut in place.
 *   stream          [K][7] the runs' readings back to back (device memory); run r owns the knots
 *                   [stream_offsets[r], stream_offsets[r + 1]).  Stamps NON-DECREASING within a run; nothing is assumed across
 *                   runs (every run may start its clock at 0)
 *   stream_offsets  [R + 1] (device memory): 0 = stream_offsets[0] <= ... <= stream_offsets[R] = K
 *   update_times    [U] (device memory); run r owns the windows u in [update_offsets[r], update_offsets[r + 1]), whose update
 *                   times are non-decreasing
 *   update_offsets  [R + 1] (device memory): 0 = update_offsets[0] <= ... <= update_offsets[R] = U
 *   N, lin, q_k_lin, out   as in cpi_preintegrate_stream, indexed by the GLOBAL window u in [0, U)
 *   workspace       cpi_streams_workspace_bytes(R, U) bytes of device memory, 16-byte aligned.  Its layout starts with that of
 *                   cpi_stream_workspace_bytes(U), so cpi_stream_counts(workspace, U) holds the TRUE counts after the call;
 *                   the rest of its contents is unspecified.  (Today the two sizes are equal for every R.)
 * Window u of run r is, bit for bit, window u - update_offsets[r] of a cpi_preintegrate_stream call on the readings and update
 * times of run r alone with the same N and params and the same lane split (cpi_params.lanes_per_window: the automatic choice
 * depends on U, so only a pinned value gives the per-run call's split) -- except the covariance of model 3, which depends on
 * the windows that share its wavefront in the last bits (~1e-22 of a covariance entry); the whole call is bit for bit
 * cpi_preintegrate_batch on the windows the host assemblers cut out of every run, for every model: the first window of a run starts at that run's first
 * reading, and the models (1, 2, 3 = Forster), the outputs, the tail interval and truncation to N intervals follow
 * cpi_preintegrate_stream.  A run without readings yields windows of 0 intervals (the identity / zero state, count 0); a run
 * without update times contributes nothing; runs of 1, 2 or 3 readings are fine.  K == 0 with U > 0 (no reading at all) and
 * R == 0 with U > 0 return CPI_ERR_INVALID; U == 0 is a no-op.
 * The offsets live in device memory and cannot be validated by the call: the kernels CLAMP them (into [0, K] / [0, U]) --
 * wrong offsets give wrong windows, never an out-of-bounds read.  cpi_preintegrate_streams_host validates them.
 * A mean-only request (models 1 and 2) runs ONE kernel: every wavefront finds the run of its windows (a bisection over
 * update_offsets, done once per wavefront unless it straddles a run boundary) and cuts its windows in its prologue; every other
 * request runs a cut kernel first, as cpi_preintegrate_stream does.  No host synchronisation: the call can be captured into a
 * graph. */
size_t cpi_streams_workspace_bytes(int64_t R, int64_t U);
int cpi_preintegrate_streams(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                             const int64_t *stream_offsets, int64_t U, const double *update_times, const int64_t *update_offsets,
                             int32_t N, const double *lin, const double *q_k_lin, void *workspace, const cpi_outputs *out);

/* Running preintegration from IMU stream(s), cut in place: the rows of cpi_preintegrate_running for the windows of
 * cpi_preintegrate_stream / cpi_preintegrate_streams, with ZERO copies of the IMU data and no host assembly.
 *   - inputs, the window semantics, N as a truncating bound, the clamped offsets of the multi-stream form and the workspace
 *     are exactly those of cpi_preintegrate_stream / cpi_preintegrate_streams (cpi_stream_workspace_bytes(U) /
 *     cpi_streams_workspace_bytes(R, U) bytes, 16-byte aligned; after the call cpi_stream_counts(workspace, U) holds the TRUE
 *     counts, the rest of its contents is unspecified).  The cut kernel always runs (there is no fused-cut variant);
 *   - rows as in cpi_preintegrate_running: U * N rows, row u * N + i = window u after interval i; a skipped interval (dt <= 0)
 *     repeats the previous row bit for bit; rows i >= count[u] repeat the window's final state, so row u * N + N - 1 is the
 *     measurement cpi_preintegrate_stream[s] returns; a window of 0 intervals (an update time before the first reading, two
 *     equal update times, a run without readings) gives N zero-state rows; a window longer than N gives the rows of its first N
 *     intervals, none of them a tail; a P_sym row is bit for bit the upper triangle of the P row; 64-bit row offsets.  Give a
 *     TIGHT N: the output is U * N rows;
 *   - bit-identity: the rows are bit for bit those of cpi_preintegrate_running on the knots / first / count that the host
 *     assemblers (cpi_amd/stream.py, cpi_host::assemble_windows) cut from the same stream(s), with count clamped to N and the same
 *     N, params and lanes_per_window (0 included: the automatic lane choice is the same function of U, N and the request in
 *     both entries).  Window u of run r of the multi-stream call is bit for bit window u - update_offsets[r] of the
 *     single-stream call on run r alone at a pinned lanes_per_window;
 *   - models 1 and 2, imu_avg 0 / 1; means and covariance for both, the five analytic bias Jacobians for model 1.
 *     CPI_ERR_INVALID: CPI_MODEL_FORSTER, any Jacobian field (J_q ... O_b) with model 2, model 2 without q_k_lin, N > 65535, an
 *     unsupported lanes_per_window, a NULL workspace / stream / update_times / lin / rows (or offsets), K == 0 or R == 0 with
 *     U > 0.  U == 0 or N == 0 is a no-op (nothing is written, the workspace included).
 * The kernels (cut, means / Jacobians, covariance) run one after the other on the context's stream, without host
 * synchronisation: the call can be captured into a graph without parallel branches.  No read leaves the K readings of the
 * stream, whatever the offsets hold and wherever a window lies.
 * Composition: with F = U * N and idx_i[row] = row / N, cpi_predict_batch turns the rows into IMU-rate predicted states. */
int cpi_preintegrate_stream_running(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                    const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                    void *workspace, const cpi_outputs *rows);
int cpi_preintegrate_streams_running(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                     const int64_t *stream_offsets, int64_t U, const double *update_times,
                                     const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                     void *workspace, const cpi_outputs *rows);

/* cpi_preintegrate_stream_running / cpi_preintegrate_streams_running WITH MODEL 2's JACOBIAN ROWS: to them what cpi_running_stj_batch
 * is to cpi_preintegrate_running.  One entry serves one stream or many: the single-stream form is R == 1 with stream_offsets ==
 * update_offsets == NULL (cpi_preintegrate_stream_running); otherwise the arguments and every rule are those of
 * cpi_preintegrate_streams_running.  Without a model-2 Jacobian field in rows the call IS the older entry: the same kernels, rows
 * bit for bit.  With model 2, state_transition_jacobians != 0 and any of J_q ... O_b in rows, the Jacobian rows are bit for bit the
 * rows of cpi_running_stj_batch on the knots / first / count that the host assemblers cut from the same stream(s), with count
 * clamped to N and the same N, params and lanes_per_window; the mean and P / P_sym rows are those of the older entry.  The cut kernel,
 * the stream mean kernel and cpi_running_stj_batch's covariance kernel (which reads the cut windows in place) run one after the other
 * on the context's stream: a capture is a chain without parallel branches.
 * CPI_ERR_INVALID beyond the older entries': model 2 with state_transition_jacobians == 0 and a Jacobian field, with
 * cpi_running_stj_batch's text.
 * Still not provided: rows from a carry record; model 2's analytic Jacobians; the device-set (cpi_group_*) path. */
int cpi_stream_running_stj_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                 const int64_t *stream_offsets, int64_t U, const double *update_times,
                                 const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                 void *workspace, const cpi_outputs *rows);

/* The query family BY ABSOLUTE TIME over IMU stream(s) read in place: what cpi_query_batch / cpi_query_cov_batch /
 * cpi_query_stj_batch return, for a caller that holds a resident stream, its update times and point stamps in absolute time (a lidar
 * sweep to deskew, keyframes chosen after the fact) -- no host assembly, no copy of the IMU data, no window index computed by the
 * caller.  The call finds the window and the interval on the device and returns the window index it found.
 *   prm, R, K, stream, stream_offsets, U, update_times, update_offsets, N, lin, q_k_lin
 *             the arguments of the cpi_preintegrate_stream[s]_running / cpi_stream_running_stj_batch call that wrote rows (R == 1
 *             with both offsets NULL: one stream)
 *   rows      the U * N rows that call wrote; what they must hold per request is what the three query entries say
 *   workspace cpi_streams_workspace_bytes(R, U) bytes, 16-byte aligned.  The call runs the cut kernel into it ITSELF (deterministic,
 *             U lanes): it depends on nothing an earlier call left there.  Afterwards cpi_stream_counts holds the true counts
 *   Q, qrun [Q] (int32; may be NULL when R == 1: run 0), qtime [Q]   query k asks for run qrun[k] at the absolute time qtime[k]
 *   qwin_out  [Q] int32, may be NULL: the GLOBAL window index of every query, -1 for a run without update times
 *   out       arrays of Q rows; any pointer may be NULL = "not wanted"
 * Window lookup, query k: r = qrun[k] CLAMPED into [0, R); [u0, u1) = the run's windows from the clamped update_offsets.  u1 <= u0:
 * NaN in every requested field and qwin_out[k] = -1.  Otherwise u = u0 + #{v in [u0, u1) : update_times[v] < t_q}, clamped to
 * u1 - 1: window u covers (update[u - 1], update[u]], so u is the first window of the run whose update time is not before t_q; of equal
 * update times the first wins; a time past the last update gets the last window; a NaN t_q gives u0.  No read leaves
 * update_times[0, U), whatever qrun or the offsets hold.
 * Inside the window the semantics are exactly those of the three query entries on the window as the kernels see it: t_0 = the
 * patched front stamp, t_1 .. t_{n-1} the stream's own stamps, t_n = the update time when the window has a tail, else the stream's
 * stamp; n = the cut count clamped into [0, N].  i, the base row u N + i - 1, the held-reading step over [t_i, t_q], the bit-for-bit
 * copy when there is no step, NaN for a NaN t_q, no extrapolation, model 2's clone rows and transition columns rebuilt from the row:
 * all unchanged.
 * DEFINING PROPERTY: with knots / first / count = what the host assemblers cut from the stream(s) (count clamped to N), out is bit for
 * bit what cpi_query_stj_batch(..., rows, Q, qwin_out, qtime, out) writes, for every field, model and request.
 * Requests and refusals: the union of the three query entries (means for models 1 and 2, model-1 Jacobians, P / P_sym, model 2's
 * seven Jacobians with state_transition_jacobians != 0).  CPI_ERR_INVALID as the stream entries: CPI_MODEL_FORSTER, N > 65535,
 * Q > 2^31 - 1, K == 0 or R == 0 with U > 0, U == 0 with Q > 0, a NULL argument.  Q == 0 is a no-op.
 * The kernels (cut, then one per group of fields) run one after the other on the context's stream, with no side stream and no host
 * synchronisation: a capture is a chain without parallel branches.
 * Composition: cpi_predict_batch and the factor sweeps with idx_i = qwin_out, as with cpi_query_*_batch.
 * Still not provided: rows from a carry record; model 2's analytic Jacobians (state_transition_jacobians == 0); extrapolation past
 * t_n; the device-set (cpi_group_*) path. */
int cpi_query_stream_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                           const int64_t *stream_offsets, int64_t U, const double *update_times,
                           const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                           void *workspace, const cpi_outputs *rows, int64_t Q, const int32_t *qrun, const double *qtime,
                           int32_t *qwin_out, const cpi_outputs *out);

/* The same loop for the mean outputs (DT, alpha, beta, q) on the TILED layout: the knots of 64 consecutive windows
 * interleaved per step,
 *     tiles[ceil(W/64)][N+1][7][64]      tiles[b][s][k][i] = field k of {t, w[3], a[3]} of knot s of window 64 b + i,
 * so that a wavefront (one tile, one lane per window) reads every step as seven coalesced 512-byte rows: one linear
 * stream per wavefront, no staging -- the mean-only recursion is HBM-bound and this is the layout it wants on MI355X
 * (DESIGN.md 3.1a).  Small batches (< 640 tiles) split a tile's steps over four wavefronts, same results to rounding
 * (prm->lanes_per_window = 1..8 pins the number of wavefronts per tile).
 * Columns past W inside the last tile are never written back.  count as in cpi_preintegrate_batch: a lane never reads
 * its column past row count[w], whatever lies there (unwritten memory, NaN) is harmless; rows of the tile array past the
 * largest count must still be ALLOCATED as the shape says.  Skipped intervals (dt <= 0, NaN dt) inside a window need
 * finite readings, as above.  Any Jacobian / covariance pointer in out -> CPI_ERR_INVALID (those kernels are FP64-bound:
 * the layout would buy nothing).
 *
 * PRODUCERS of the layout -- a caller never needs a dense copy first:
 *   cpi_assemble_tiles    cuts ONE IMU stream (device memory) into windows at successive update times and writes them
 *                         straight into tiles + count: the loop of GraphSolver::createimufactor_cpi_v1/v2
 *                         (GraphSolver_IMU.cpp:50-69 -- whole intervals while imu_times[1] <= updatetime, then the partial
 *                         tail interval with the front reading repeated, the front stamp overwritten by the update time)
 *                         for every window at once.  stream [K][7] knot records with NON-DECREASING stamps, update_times
 *                         [U] non-decreasing (then the deque state at the start of a window depends on the previous update
 *                         time alone; a stream with backward stamps needs the host assembler).  count[u] receives the TRUE
 *                         number of intervals of window u; rows beyond N are not written -- a caller sizes N >= max count
 *                         (the kernels clamp count to N).
 *                         WHEN: the copy costs 1.1-1.2 ms per 1 M x 50 windows (twice the tiled kernel it feeds), so a caller
 *                         that preintegrates a stream ONCE uses cpi_preintegrate_stream above (windows cut in place, no copy:
 *                         0.65-0.69 ms mean-only); tiles pay when the SAME windows are preintegrated again and again at new
 *                         linearisation points -- from about the 8th use (profiles/r05_assembler.md).
 *   cpi_tile_windows      re-tiles windows the caller already holds in the layouts of cpi_preintegrate_batch (dense
 *                         knots[W][N+1][7] with first == NULL, or a shared stream indexed by first[W] / count[W]); rows
 *                         past a window's last knot repeat that knot.  A full extra pass: for one-off use and tests.
 *                         cpi_tile_knots is the dense special case (first = count = NULL).
 *   host side             cpi_amd/csrc/cpi_host.hpp (assemble_windows_tiled, CpiBatch::flush_means) and
 *                         cpi_amd/stream.py (assemble_windows(..., layout="tiled")) write knot s of window w at
 *                         (((w / 64) (N+1) + s) 7 + k) 64 + w % 64 while they assemble; cpi_preintegrate_tiled_batch_host
 *                         takes such tiles from HOST memory through the chunked upload / kernel / download pipeline. */
int cpi_preintegrate_tiled_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *tiles,
                                 const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *out);
int cpi_assemble_tiles(cpi_ctx *ctx, int64_t K, const double *stream /*[K][7]*/, int64_t U, const double *update_times /*[U]*/,
                       int32_t N, double *tiles /*[ceil(U/64)][N+1][7][64]*/, int32_t *count /*[U]*/);
int cpi_tile_windows(cpi_ctx *ctx, int64_t W, int32_t N, const double *knots, const int64_t *first, const int32_t *count,
                     double *tiles);
int cpi_tile_knots(cpi_ctx *ctx, int64_t W, int32_t N, const double *knots /*[W][N+1][7]*/, double *tiles);

/* Replaces: ImuFactorCPIv1::evaluateError / ImuFactorCPIv2::evaluateError, one call per factor
 * (ImuFactorCPIv1.cpp:37-208, ImuFactorCPIv2.cpp:38-212), as driven by GTSAM's linearize loop.
 *
 * Factor f reads its measurement from the preintegration outputs of window f (field -> ctor
 * mapping of GraphSolver_IMU.cpp:74-75,129-130: J_b->J_beta, J_a->J_alpha, H_b->H_beta,
 * H_a->H_alpha, O_b->O_beta, O_a->O_alpha), its linearisation biases from lin[f] and, for
 * model 2, q_K_lin from q_k_lin[f].
 * states  [S][16] JPLNavState array; idx_i/idx_j [F] select state_i/state_j (NULL: f and f+1, which needs S >= F+1).
 *         S is the number of states: the device-pointer entries cannot inspect idx (it lives in HBM), so the kernels
 *         CLAMP every index into [0, S) -- a wrong index yields a wrong factor, never an out-of-bounds read; the
 *         _host variant validates the indices and returns CPI_ERR_INVALID.
 * err     [F][15] unwhitened residual; H1, H2 [F][225] dense column-major Jacobians wrt the two
 *         states' tangent vectors; H1/H2 may be NULL (the boost::optional<Matrix&> = none case). */
int cpi_factor_eval_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                          const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                          const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                          double *err, double *H1, double *H2);

/* Fast path of the same evaluation for callers that assemble their own Hessian blocks (note on
 * a11): of the 450 doubles of the dense H1 / H2 pair only 54 depend on the current states; everything else is 0, +-I
 * or a copy of a measurement field the caller already holds.  packed [F][72] (576 B per factor), 3x3 blocks
 * column-major:
 *    [ 0..14]  err                                   (ImuFactorCPIv1.cpp:81-88)
 *    [15..23]  H1(0,0)   d e_theta / d theta_K       (:109)          [24..32]  H1(6,0)   d e_v / d theta_K   (:120)
 *    [33..41]  H1(12,0)  d e_p / d theta_K           (:132)          [42..50]  H1(0,3)   d e_theta / d b_g,K (:112)
 *    [51..59]  Rk = quat_2_Rot(q_GtoK)                               [60..68]  H2(0,0)   d e_theta / d theta_K+1 (:169)
 *    [69..71]  0 (padding to a multiple of 16 bytes)
 * The remaining blocks of the dense pair follow from these and the measurement (ImuFactorCPIv1.cpp:113-143,172-185):
 *    H1(3,3) = H1(9,9) = -I;  H1(6,3) = -J_beta;  H1(6,6) = -Rk;  H1(6,9) = -H_beta;  H1(12,3) = -J_alpha;
 *    H1(12,6) = -deltatime Rk;  H1(12,9) = -H_alpha;  H1(12,12) = -Rk;  H2 = blkdiag(H2(0,0), I, Rk, I, Rk);  all others 0.
 * Same arguments as cpi_factor_eval_batch.  (cpi_amd.unpack_factor in the Python mirror rebuilds the dense pair.) */
int cpi_factor_eval_packed_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                 const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                 const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                 double *packed);

/* Replaces: gtsam::noiseModel::Gaussian::Covariance(P_meas) in the factor constructors
 * (ImuFactorCPIv1.h:82, ImuFactorCPIv2.h:86).  GTSAM (bitbucket gtborg/gtsam @ c21186c6, not in the
 * reference tree) builds the square-root information  R = chol_upper(P^-1)  (Gaussian::Covariance ->
 * Gaussian::Information(cov.inverse()) -> Eigen::LLT::matrixU) once per factor, R^T R = P^-1.
 * Here R = B^-1 with P = B B^T, B upper triangular (the same matrix, obtained without forming P^-1).
 * P [F][225] column-major symmetric positive definite; sqrt_info [F][225] column-major upper triangular
 * (strict lower part written as zeros, +0.0).
 * A failing pivot: the factorisation runs from pivot 14 up to pivot 0, pivot k being P[k][k] less what rows k + 1 .. 14 explain of
 * it.  A pivot that is zero, -0.0, negative, NaN or +inf fails, and then rows 0 .. k of that factor's R are NaN in every entry of
 * the upper triangle, while rows k + 1 .. 14 hold what they hold for a P whose leading rows are healthy (for k = 0 that is ONE
 * row of NaNs).  Row 0 multiplies every residual, so chi2 of that factor (cpi_factor_cost_*) and its Hessian block
 * (cpi_factor_hessian_*: f and everything row 0 reaches) are NaN; no other factor of the call is touched.
 * Both triangles of P are read: P must be mirrored bit for bit.  A caller who holds one triangle uses the packed form.
 * Binary scaling is exact: P x 4^k gives R x 2^-k bit for bit as long as every value and intermediate stays in the normal range.
 * sqrt_info == P exactly (in place) is allowed and gives the same bits; any other overlap of the two arrays is refused. */
int cpi_sqrt_information_batch(cpi_ctx *ctx, int64_t F, const double *P, double *sqrt_info);
/* The same factorisation on packed triangles (ABI 3): P_sym [F][120] in (cpi_outputs.P_sym of the covariance kernels), R_tri
 * [F][120] out -- 1 920 bytes per factor instead of 3 600, of which the dense form spends 840 on the mirrored half of P and
 * 840 on zeros it writes below R's diagonal.  Entry for entry the same values as cpi_sqrt_information_batch computes from the
 * dense form of the same P (same arithmetic, same order: bit-identical) -- the failing-pivot rule, the exact binary scaling and
 * the aliasing rule (R_tri == P_sym exactly allowed, any other overlap refused) included.  Only the given triangle is read. */
int cpi_sqrt_information_packed_batch(cpi_ctx *ctx, int64_t F, const double *P_sym, double *R_tri);

/* cpi_factor_eval_batch followed by GTSAM's NoiseModelFactor::linearize whitening
 * (Gaussian::WhitenSystem): err <- R err, H1 <- R H1, H2 <- R H2 with R = sqrt_info[f]. */
int cpi_factor_eval_whitened_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                   const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                   const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                   const double *sqrt_info, double *err, double *H1, double *H2);
/* The same with R as its packed upper triangle R_tri [F][120] (cpi_sqrt_information_packed_batch): 840 bytes less to read per
 * factor, identical outputs (the 105 entries the dense form stores below the diagonal are zeros the kernel never multiplied by). */
int cpi_factor_eval_whitened_tri_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                       const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                       const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                       const double *R_tri, double *err, double *H1, double *H2);

/* The same evaluation carried one step further down GTSAM's pipeline: the factor's
 * contribution to the normal equations.  NoiseModelFactor::linearize turns (e, H1, H2) into the JacobianFactor
 * [A1 A2 | b] = [R H1, R H2 | -R e]; a HessianFactor built from it holds the augmented information matrix
 *     [A1 A2 b]^T [A1 A2 b] = [ G  g ; g^T  f ],   G = A^T A (30 x 30),  g = A^T b (30),  f = b^T b,
 * over the tangent vectors of (state_i, state_j).  hess [F][496]: its upper triangle, packed column-major
 * (entry (i, d), i <= d <= 30, at i + d (d + 1) / 2; rows / columns 0-14 state_i, 15-29 state_j, 30 the b column).
 * The whitened Jacobians never leave the chip.  (GTSAM is not in the reference tree: PARITY UNPINNED, checked against a
 * numpy restatement of the definition above on the outputs of cpi_factor_eval_whitened_batch.) */
int cpi_factor_hessian_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                             const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                             const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                             const double *sqrt_info, double *hess);
/* ... with R as its packed upper triangle R_tri [F][120]: identical hess. */
int cpi_factor_hessian_tri_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                                 const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                                 const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                 const double *R_tri, double *hess);

/* Replaces: GraphSolver::getpredictedstate_v1 / _v2 (GraphSolver_IMU.cpp:263-281, 289-307):
 * states_j[f] = prediction of X(k+1) from states_i[idx_i[f]] and measurement f.  states_i [S][16]; idx_i NULL: state f. */
int cpi_predict_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                      const cpi_outputs *meas, const double *states_i, int64_t S, const int32_t *idx_i,
                      double *states_j);

/* ---- The optimiser's trial step.  With cpi_factor_hessian_* these close the loop
 *     linearise -> solve (the caller's) -> retract -> cost -> accept / reject
 * on the device: none of them synchronises the host, and each is a chain of kernels without branches on the context's stream, so
 * the whole iteration captures into one graph.  No general sparse solver is provided; for graphs whose factors form chains
 * (IMU factors between consecutive states, plus whatever touches one state at a time) cpi_chain_solve_batch below is the solve.
 *
 * cpi_retract_batch replaces: JPLNavState::retract (gtsam/JPLNavState.cpp:37-71), the map along which every H1 / H2 of the
 * evaluateError sweeps is a derivative.  states_out[s] = retract(states_in[s], delta[s]):
 *   states  [S][16] = [q(4) bg(3) v(3) ba(3) p(3)];  delta [S][15] = [dtheta bg v ba p]
 *   n = |dtheta|, dq = [sin(n/2)/n dtheta, cos(n/2)], normalised, negated if dq.w < 0, the identity where that gave NaN (the
 *   reference's n == 0: 0 / 0), q_out = quat_multiply(dq, q) with its own normalisation and w >= 0 flip; the other twelve entries
 *   are x + delta, bit for bit the IEEE sums.  A zero step therefore gives quat_multiply(identity, q), not a copy of q.
 * IN PLACE: states_out may equal states_in exactly (same bits as the out-of-place call).  Any other overlap among the three arrays
 * is CPI_ERR_INVALID ("overlaps" in cpi_last_error).
 * cpi_local_batch replaces: JPLNavState::localCoordinates (JPLNavState.cpp:80-88):
 *   xi[s][0..2] = 2 vec(quat_multiply(other[s].q, inv(x[s].q))),  xi[s][3..14] = other[s][4..15] - x[s][4..15]  (IEEE differences).
 * xi may not overlap x or other.  Both: S == 0 is a no-op; NULL pointers and S < 0 are CPI_ERR_INVALID; every refusal comes
 * before the context is looked at. */
int cpi_retract_batch(cpi_ctx *ctx, int64_t S, const double *states_in, const double *delta, double *states_out);
int cpi_local_batch(cpi_ctx *ctx, int64_t S, const double *x, const double *other, double *xi);

/* The cost of F factors at the given states.  Replaces: GTSAM's NoiseModelFactor::error(values) = 0.5 |R e|^2 for every factor of
 * the graph, and their sum (GTSAM is absent from the reference tree: PARITY UNPINNED like the other entries of SURVEY.md 8 f1) --
 * what Levenberg-Marquardt / dogleg accept or reject a step by, what a line search evaluates, what gates outliers (chi2 is the
 * squared Mahalanobis distance).  Arguments as cpi_factor_eval_whitened_batch / _tri_batch; state indices are clamped into [0, S).
 *   sqrt_info [F][225] dense column-major upper-triangular R (cpi_sqrt_information_batch) / R_tri [F][120] its packed triangle
 *   chi2   [F]      required: chi2[f] = sum_i werr_i^2 -- every square rounded by itself (no fused multiply-add), added in ascending
 *                   order left to right, (..((w0 w0 + w1 w1) + w2 w2) + ..) + w14 w14.  It is the `f` entry (30, 30) of
 *                   cpi_factor_hessian_* up to rounding (that one is e^T (R^T R) e)
 *   werr   [F][15]  or NULL: R e, bit for bit the err of cpi_factor_eval_whitened[_tri]_batch on the same inputs
 *   total  NULL, or a workspace of cpi_factor_cost_total_doubles(F) doubles: element 0 receives 0.5 * sum_f chi2[f], the rest is
 *          scratch for partial sums.  The library allocates nothing.  A reduction of fixed shape without floating-point atomics,
 *          enqueued behind the cost kernel: the same inputs give the same bits on every run, with or without werr.
 * The dense and the packed form give the same bits.  A factor whose R holds NaN (cpi_sqrt_information_* met a non-positive pivot)
 * gets chi2 = NaN and makes total NaN; the other factors are not affected.
 * No output may overlap an input or another output: CPI_ERR_INVALID, "overlaps" in cpi_last_error.  Also refused: a model other
 * than 1 and 2, F < 0, NULL chi2 / R / required input, what cpi_factor_eval_batch refuses.  Every refusal comes before the context
 * is looked at.  F == 0 writes total[0] = 0 when total is given. */
size_t cpi_factor_cost_total_doubles(int64_t F);
int cpi_factor_cost_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                          const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                          const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                          const double *sqrt_info, double *chi2, double *werr, double *total);
int cpi_factor_cost_tri_batch(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                              const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                              const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                              const double *R_tri, double *chi2, double *werr, double *total);

/* The step of the loop above for CHAINS of IMU factors.  Replaces: the elimination of a chain by GTSAM's linear solver (the
 * GaussianFactorGraph of the linearised IMU factors and single-state priors, eliminated along the trajectory; GTSAM is absent from
 * the reference tree: PARITY UNPINNED like the other entries of SURVEY.md 8 f1, checked against a long-double dense solve of the
 * definition below).  NOT replicated: the minDiagonal / maxDiagonal clamps of GTSAM's LevenbergMarquardtParams on the damping
 * diagonal -- a caller who wants them clamps the prior's diagonal or lambda.  Not a general sparse solver: factors that couple
 * non-adjacent states (visual factors) are out of scope.
 * Chain c has n_c states s = 0 .. n_c - 1 and n_c - 1 factors, factor k joining states k and k + 1.  With H_k the 31 x 31 matrix of
 * hess row k (the packing of cpi_factor_hessian_*) and Pr_s the optional 16 x 16 prior [Lam eta; eta^T .] of state s:
 *     D_s = H_{s-1}[15:30, 15:30] + H_s[0:15, 0:15] + Pr_s[0:15, 0:15]       (a missing neighbour contributes nothing)
 *     U_s = H_s[0:15, 15:30]                                                  (block (s, s + 1))
 *     g_s = H_{s-1}[15:30, 30] + H_s[0:15, 30] + Pr_s[0:15, 15]
 *     D_s += lambda_c I (CPI_DAMP_IDENTITY)   or   D_s += lambda_c diag(D_s) (CPI_DAMP_DIAGONAL; diag taken after the sums above)
 *     A delta = g,   A = blocktridiag(U_{s-1}^T, D_s, U_s)
 * g is taken as hess holds it (g = A^T b, b = -R e): delta is the Gauss-Newton / Levenberg-Marquardt step, and cpi_retract_batch
 * takes it as it is.  Block Cholesky along the chain (L_s = chol(D_s - W_{s-1}^T W_{s-1}), W_s = L_s^-1 U_s), forward and back.
 *   C chains; G >= 1 the longest chain in states; S rows of delta / prior; F rows of hess            (the layout of cpi_merge_batch)
 *   first  [C] the chain's first state, NULL: c * G;  count [C] its number of states, clamped into [0, G], NULL: G; a chain is
 *          clipped at S.  ffirst [C]: the factor joining states first + k and first + k + 1 is hess row ffirst[c] + k; NULL:
 *          first_c - c (factors in chain order when the chains tile the states back to back).  The idx_i / idx_j of the Hessian
 *          sweep are these pairs.
 *   hess   [F][496];  prior NULL or [S][136], the packed upper triangle in the same column-major rule ((i, d) at i + d (d + 1) / 2;
 *          entry 135 is never read);  lambda NULL or [C] DEVICE doubles (a Levenberg-Marquardt loop keeps lambda on the device);
 *          NULL gives the bits of lambda = 0
 *   delta  [S][15]; rows of no chain are not written.  status NULL or [C]: 0 solved; s + 1: the pivot block of state s was not
 *          positive definite (a pivot that is not > 0, the rule of cpi_sqrt_information_*); -1: the chain's factor rows leave
 *          [0, F) -- such a chain reads nothing outside the arrays.  A failed or refused chain has NaN in every delta row of its
 *          own; no other chain is affected.  count = 1 solves (Lam + damping) delta = eta; count = 0 writes nothing, status 0.
 *          A NaN in g alone (D and U finite) meets no pivot: the status is not affected by it (0 when every block is positive
 *          definite) and every delta row of the chain is NaN; a NaN in D or U is a pivot that is not > 0.  A block that is exactly
 *          zero is a failed pivot (0 is not > 0): no prior, one state and lambda = 0 give status 1, and so does CPI_DAMP_DIAGONAL
 *          on a zero diagonal whatever lambda is (lambda * 0).
 *   workspace  cpi_chain_solve_workspace_doubles(S) doubles of the caller's ([R y] and W of every state, 360 doubles each); its
 *          contents after the call are what cpi_chain_marginals_batch reads and are not declared otherwise.  The library
 *          allocates nothing.
 * A chain's bits depend on its own data only, not on C or on its position.  Chains that share states are the caller's error: the
 * contents are unspecified, no access goes out of bounds.  One kernel on the context's stream, no host synchronisation: capturable.
 * 16 lanes work on a chain, 4 chains share a wavefront; there is no parallelism ALONG a chain, so one long chain runs at the
 * latency of its states in sequence (profiles/chain_solve.md).  cpi_chain_condense_batch below cuts long chains into segments that
 * are eliminated in parallel and hands this entry a short chain.
 * Refused before the context is looked at (CPI_ERR_INVALID): NULL hess when G > 1, NULL delta / workspace, negative sizes, G < 1 or
 * G > 2^31 - 1, a damping other than the two, any output that overlaps an input or another output ("overlaps" in cpi_last_error).  C == 0 is a
 * no-op. */
enum { CPI_DAMP_IDENTITY = 0, CPI_DAMP_DIAGONAL = 1 };
size_t cpi_chain_solve_workspace_doubles(int64_t S);
int cpi_chain_solve_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                          const int64_t *first, const int32_t *count, const int64_t *ffirst,
                          const double *hess, const double *prior, const double *lambda, int32_t damping,
                          double *delta, int32_t *status, double *workspace);

/* The uncertainty of what the loop above converged to: the covariance of every state of a solved chain, and of every pair of
 * neighbouring states.  Replaces: GTSAM's Marginals (marginalCovariance of one state, jointMarginalCovariance of two neighbours) for
 * graphs that are chains; GTSAM is absent from the reference tree: PARITY UNPINNED, checked against a long-double dense inverse.
 * Covariance blocks further than one state apart are out of scope.
 * WHAT IS INVERTED: the matrix A that cpi_chain_solve_batch factorised into workspace, DAMPING INCLUDED.  The covariance of the
 * estimate therefore comes from a solve with lambda = NULL at the converged states (factor_hessian -> chain_solve(lambda = NULL) ->
 * chain_marginals); the delta of that solve is the remaining Gauss-Newton step -- a convergence check, not something to apply.
 * After a damped solve the result is (A + damping)^-1, which is no covariance of anything.  The coordinates are the tangent space
 * of cpi_retract_batch ([theta bg v ba p]) at the states the Hessian was linearised at.
 * With [R_s | W_s] the block row of the Cholesky factor in the workspace (W_s = R_s^-T U_s), one backward recursion along the chain:
 *     Sigma[n-1][n-1] = R_{n-1}^-1 R_{n-1}^-T;    s = n - 2 .. 0:  K_s = R_s^-1 W_s,   Sigma[s][s+1] = -K_s Sigma[s+1][s+1],
 *     Sigma[s][s] = R_s^-1 R_s^-T + K_s Sigma[s+1][s+1] K_s^T
 *   C, G, S, first, count: the values of the solve that wrote workspace, with the same meaning and the same clamping.
 *   workspace  cpi_chain_solve_workspace_doubles(S) DEVICE doubles as that solve left them; read only.  (The solve writes no W for a
 *          chain's last state; it is never read.)
 *   status NULL or [C] as the solve wrote it: a chain whose status is not 0 gets NaN in every cov and cross row of its own states,
 *          and no other chain is affected.  NULL: the caller vouches for every chain.
 *   cov    [S][120]: Sigma[s][s], the packed upper triangle in the packing of cpi_outputs.P_sym ((i, j), i <= j, at
 *          CPI_TRI_INDEX(i, j) = i + j (j + 1) / 2).  A row is a valid input row of cpi_sqrt_information_packed_batch, which turns a
 *          marginal into the square-root information of the prior a fixed-lag window carries on.  The block is symmetric by
 *          construction (one triangle is computed).
 *   cross  NULL or [S][225]: row s holds Sigma[s][s+1] column-major, rows for state s and columns for state s + 1.  The row of a
 *          chain's last state is not written.
 * Rows of states that belong to no chain are not written; count = 0 writes nothing; count = 1 gives (Lam + damping)^-1.
 * A chain's bits depend on its own records only, not on C or on its position.  The library allocates nothing; one kernel on the
 * context's stream, no host synchronisation: a capture is a chain without parallel branches.  16 lanes work on a chain and there
 * is no parallelism ALONG a chain (profiles/chain_marginals.md).
 * Refused before the context is looked at (CPI_ERR_INVALID): negative sizes, G < 1 or G > 2^31 - 1, a NULL workspace or cov when
 * S > 0, cov or cross overlapping workspace, first, count, status or each other ("overlaps" in cpi_last_error).  C == 0 is a no-op. */
int cpi_chain_marginals_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S,
                              const int64_t *first, const int32_t *count, const int32_t *status,
                              const double *workspace, double *cov, double *cross);

/* What a fixed-lag smoother does between two optimisations: the window slides, the oldest m states of a chain leave, and what they
 * knew becomes a prior on the first state that stays.  Replaces: GTSAM's marginalisation of the leading variables of a chain (the
 * elimination of those variables and the LinearContainerFactor that carries the resulting marginal factor on; GTSAM is absent from
 * the reference tree: PARITY UNPINNED, checked against a long-double Schur complement of the definition below).  Out of scope:
 * eliminating states from a chain's tail or interior, damping (marginalisation is of the UNDAMPED system: there is no lambda),
 * the constant term of the marginal cost.
 * With the chains, H_k, Pr_s, D_s, U_s and g_s of cpi_chain_solve_batch (lambda = 0), E the eliminated states 0 .. m - 1, A_EE and g_E
 * their part of the system built from the factors 0 .. m - 1 and the priors 0 .. m - 1 alone, and A_Em = U_{m-1} the one block that
 * couples them to state m:
 *     Lam = Pr_m[0:15, 0:15] + H_{m-1}[15:30, 15:30] - A_mE A_EE^-1 A_Em
 *     eta = Pr_m[0:15, 15]   + H_{m-1}[15:30, 30]    - A_mE A_EE^-1 g_E                  (Pr_* absent when prior is NULL)
 * the Schur complement of the eliminated states onto state m.  H_m and everything later do NOT enter: the factors the next window
 * keeps are counted once.  (The marginal covariance of cpi_chain_marginals_batch is the right prior only for a window that starts
 * at the LAST state and shares no factor with this one.)  The arithmetic is the forward half of the solve, stopped at state m.
 *   C G S F first count ffirst hess prior: those of cpi_chain_solve_batch, with the same clamps and the same rule for ffirst
 *   M, drop   drop NULL or [C] DEVICE int32: m_c, the number of leading states of chain c to eliminate; NULL: M for every chain.
 *          0 <= m_c < n_c is required per chain, n_c the chain's clamped number of states.
 *   out    [C][136]: row c is the prior row of state m_c of the reduced chain in the packing of prior ([Lam eta; eta^T .], (i, d) at
 *          i + d (d + 1) / 2).  Entry 135 is written as 0.0; entry 135 of the input priors is never read.  One triangle is written:
 *          Lam is symmetric by construction.  m = 0 gives Pr_0 with entry 135 zeroed (zeros without a prior): the values pass
 *          through as they are.
 *   status NULL or [C]: 0 success; s + 1: the block of the ELIMINATED state s was not positive definite (a block at a state >= m
 *          is not looked at); -1: the chain's factor rows leave [0, F) (the solve's rule) or m_c is outside [0, n_c) -- a chain
 *          without states is refused this way.  A chain whose status is not 0 gets a NaN row; no other chain is affected.
 *          Status 0 does not promise a finite row: only the pivots of the eliminated blocks are looked at.  A NaN in Pr_m, in the
 *          trailing block, U or g of factor m - 1, or in a right-hand side (g, eta) further back reaches the entries of the row it
 *          touches and leaves the status as it is; the solve of the reduced chain reports it (a status, or a NaN delta where only
 *          eta is hit).  An exactly zero block of either sign (0.0 or -0.0) is a failed pivot (0 is not > 0): no prior and a zero
 *          factor row give status 1.  Scaling hess and prior by 4^k scales out by 4^k exactly (bit for bit) as long as every
 *          intermediate stays inside the normal range: every term is homogeneous of degree one in them.
 * WHAT IT GUARANTEES: replace row first_c + m_c of prior by out[c] and solve the chain first + m, count - m, ffirst + m on the SAME
 * hess and prior arrays (the ragged arguments of cpi_chain_solve_batch): with lambda = NULL the delta rows are those the full
 * chain's solve gives for the kept states, and cpi_chain_marginals_batch of the reduced chain gives the full chain's cov and cross
 * rows of the kept states, to rounding.  The result is a LINEAR prior at the states hess was linearised at.
 * Only the rows of hess at factors < m_c and of prior at states <= m_c are read.  A chain's bits depend on its own data only, not
 * on C or on its position.  The library allocates nothing and there is no workspace; one kernel on the context's stream, no host
 * synchronisation: a capture is a chain without parallel branches.  16 lanes work on a chain, 4 chains share a wavefront, and
 * there is no parallelism ALONG a chain (profiles/chain_marginalize.md).
 * Refused before the context is looked at (CPI_ERR_INVALID): negative sizes, G < 1 or G > 2^31 - 1, NULL hess when G > 1, NULL out,
 * out or status overlapping an input or each other ("overlaps" in cpi_last_error).  C == 0 is a no-op. */
int cpi_chain_marginalize_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                const double *hess, const double *prior,
                                int32_t M, const int32_t *drop,
                                double *out, int32_t *status);

/* Segment condensation: long chains solved in parallel ALONG the chain.  A run of consecutive IMU factors with the states between its
 * two ends eliminated is again a 31 x 31 factor row between two states, in the packing of hess.  Every chain is cut into segments of
 * K factors; each segment's interior states are eliminated by a 16-lane group of its own (cpi_chain_condense_batch); the short
 * reduced chain of segment ends goes to cpi_chain_solve_batch as it is; and the result is substituted back into the interiors, again
 * one group per segment (cpi_chain_expand_batch).  A chain of 549 states at K = 23 is 24 independent eliminations of 22 states, one
 * solve of 25 states and 24 independent back-substitutions, where the solve alone walks 549 dependent steps forward and 549 back.
 * Replaces: nothing in the reference tree (GTSAM's elimination ordering is absent from it: PARITY UNPINNED); checked against the
 * long-double dense solve of the definition of cpi_chain_solve_batch.  The reduced chain is also the exact linear counterpart of
 * cpi_merge_batch -- the keyframe-rate system of an IMU-rate chain: cpi_chain_marginals_batch on it gives the full chain's cov rows
 * at the kept states.  Out of scope: a segment option of the Levenberg-Marquardt loop; marginals of interior states (the reduced
 * chain's marginals are the separators'); a K per chain or separators chosen by the caller; condensing the reduced chain again
 * (recursion); any change of a default.
 * Chains, H_k, Pr_s, D_s, U_s, g_s, lambda_c and the two dampings are those of cpi_chain_solve_batch, with the same clamps and the
 * same refusal of factor rows that leave [0, F).
 * LAYOUT.  The separators of a chain of n >= 2 states are the states 0, K, 2K, ... below n - 1, plus the last state n - 1; segment j
 * spans the factors between separator j and separator j + 1 (the last one may be shorter than K); m = ceil((n - 1) / K) + 1 reduced
 * states, m = n for n < 2.  Gr = cpi_chain_condense_states(G, K) = ceil((G - 1) / K) + 1 for G >= 2 and G below that.  The reduced
 * arrays are in the tile layout that NULL first / ffirst mean to the solve: reduced state j of chain c is row c * Gr + j, reduced
 * factor j is row c * (Gr - 1) + j.
 * CONDENSE.  For a segment with left separator a and interiors t = a + 1 .. b - 1, M = H_a to begin with (blocks M_aa, M_at, M_tt, m_a,
 * m_t and the scalar c), and per interior t
 *     D  = M_tt + H_t[0:15, 0:15] + Pr_t[0:15, 0:15] + damping_t          g = m_t + H_t[0:15, 30] + Pr_t[0:15, 15]
 *     L  = chol(D),  Wa = L^-1 M_at^T,  Wn = L^-1 U_t,  y = L^-1 g
 *     M_aa -= Wa^T Wa     M_a,t+1 = -Wa^T Wn     M_t+1,t+1 = H_t[15:30, 15:30] - Wn^T Wn
 *     m_a  -= Wa^T y      m_t+1   = H_t[15:30, 30] - Wn^T y      c += H_t[30, 30] - y^T y
 * damping_t = lambda_c I, or lambda_c diag(D_t) with D_t the FULL block of the solve's definition (H_{t-1}[15:30, 15:30] + H_t[0:15,
 * 0:15] + Pr_t: the diagonal WITHOUT the Schur term, as the solve takes it).  The final M is reduced factor row j.  The prior row of
 * separator s is Pr_s with its damping on the diagonal -- lambda_c, or lambda_c diag(D_s) from H_{s-1}, H_s and Pr_s --, entry 135
 * written as 0.0 (that of the input is never read); with lambda NULL the values pass through as they are.  The damping is baked in:
 * the reduced chain is solved with lambda = NULL, and its system is exactly the Schur complement of the damped full system onto the
 * separators, for both dampings.  A segment of one factor (K = 1, or a short tail) is H_k bit for bit.
 * EXPAND.  Every separator's delta row is the reduced solve's row, copied; for the interiors t = b - 1 .. a + 1:
 * delta_t = L_t^-T (y_t - Wa_t delta_a - Wn_t delta_{t+1}).
 *   C G S F first count ffirst hess prior lambda damping: those of cpi_chain_solve_batch
 *   K        >= 1, the factors of a segment, one value per call
 *   rhess    [C * (Gr - 1)][496]; rprior [C * Gr][136]; rcount [C]: rcount[c] = m_c.  Rows of reduced slots beyond m_c are not written.
 *   status   NULL or [C * (Gr - 1)], per segment slot: 0 the segment succeeded (a slot beyond the chain's segments: 0 as well); s + 1:
 *            the block of interior state s (an index within the chain) had a pivot that is not > 0; -1: the chain's factor rows leave
 *            [0, F).  Separators are not factorised here: the reduced solve reports them.  A failed or refused segment writes NaN
 *            into its rhess row: the reduced solve then fails that chain and only that chain, and the expansion carries the NaN into
 *            every row of the chain.
 *   workspace  cpi_chain_condense_workspace_doubles(S) doubles of the caller's: one record of 585 doubles per state, indexed by state
 *            -- L's triangle with the reciprocal pivots and y as the solve stores them, then Wn, then Wa.  Only the records of interior
 *            states are written or read.
 *   rdelta   [C * Gr][15]: the delta of the reduced solve;  delta [S][15]: rows of no chain are not written.
 * The caller runs cpi_chain_condense_batch, then cpi_chain_solve_batch(ctx, C, Gr, C * Gr, C * (Gr - 1), NULL, rcount, NULL, rhess,
 * rprior, NULL, damping, rdelta, rstatus, a solve workspace for C * Gr states), then cpi_chain_expand_batch with the C, G, S, first,
 * count and K of the condense.  A chain's bits depend on its own data and on K only, not on C or on its position.  One kernel each on
 * the context's stream, 16 lanes per segment and 4 segments per wavefront; the library allocates nothing and reads nothing back:
 * both are capturable, and a capture of the three calls is a chain without parallel branches (profiles/chain_condense.md).
 * Refused before the context is looked at (CPI_ERR_INVALID): negative sizes, G < 1 or G > 2^31 - 1, K < 1, a damping other than the
 * two, NULL hess or rhess when G > 1, NULL rprior / rcount / workspace (condense), NULL rdelta / workspace / delta (expand), any
 * output that overlaps an input or another output ("overlaps" in cpi_last_error).  C == 0 is a no-op. */
int64_t cpi_chain_condense_states(int64_t G, int64_t K);
size_t cpi_chain_condense_workspace_doubles(int64_t S);
int cpi_chain_condense_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                             const int64_t *first, const int32_t *count, const int64_t *ffirst,
                             const double *hess, const double *prior, const double *lambda, int32_t damping, int64_t K,
                             double *rhess, double *rprior, int32_t *rcount,
                             int32_t *status, double *workspace);
int cpi_chain_expand_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S,
                           const int64_t *first, const int32_t *count, int64_t K,
                           const double *rdelta, const double *workspace, double *delta);

/* The Levenberg-Marquardt step PER CHAIN, without the host looking at anything: the loop linearise -> relinearise the prior -> solve
 * -> retract -> cost -> accept closes on the device.  Replaces: the outer loop of GTSAM's
 * LevenbergMarquardtOptimizer (the error of the graph with its prior factor, the comparison of the trial's error with the current
 * one, the lambda update and the convergence test of checkConvergence), per chain instead of per graph.  GTSAM is absent from the
 * reference tree: PARITY UNPINNED; the three entries are checked against long-double restatements of the definitions below and, where
 * the summation order is fixed, bit for bit.  Out of scope: a gain-ratio (model-fidelity) acceptance rule, the minDiagonal /
 * maxDiagonal clamps, robust kernels, skipping the work of converged chains in the other sweeps.
 *
 * cpi_prior_relinearize_batch: the prior of P records at the current states, and its cost.
 *   idx     NULL or [P] DEVICE int32: record p belongs to state idx[p]; NULL: to state p, and P <= S is required.  A record whose index
 *           is outside [0, S) is skipped: it reads and writes nothing.  Duplicate indices are the caller's error (the contents are
 *           unspecified; no access goes out of bounds).
 *   states  [S][16];  anchor [P][16]: the state the prior was linearised at (x_lin of INTEGRATION.md 3o, or the centre of a Gaussian)
 *   prior0  [P][136]: [Lam eta0; . .] in the packing of prior; entry 135 is never read.  A row of cpi_chain_marginalize_batch goes in
 *           as it is; a Gaussian prior has eta0 = 0.
 * Per record, with s = idx[p]:
 *     xi    = localCoordinates(states[s], anchor[p])                 (the function of cpi_local_batch)
 *     eta_i = the fma chain k = 0 .. 14 ascending STARTING FROM eta0_i: acc = fma(Lam[i][k], xi[k], acc)
 *     t_i   = eta_i + eta0_i
 *     pcost = 0.5 * (the fma chain i = 0 .. 14 ascending from +0.0: acc = fma(xi[i], t_i, acc))
 *           = 0.5 xi^T Lam xi + eta0^T xi: the prior's cost up to the constant that marginalisation drops
 *   prior   NULL or [S][136]: row s receives the Lam bits copied, eta, and entry 135 as 0.0
 *   pcost   NULL or [S]: element s.  At least one of prior / pcost must be given.
 * Rows of states without a record are not written (the caller zeroes the arrays once).  eta is the negative gradient, the sign
 * convention of the solve; where states[s] and anchor[p] give xi = 0 the row is prior0 with entry 135 zeroed and pcost is 0.  NaN in
 * a record reaches that record's outputs only.  Refused: negative sizes, P > S with idx NULL, a NULL anchor / prior0 when
 * P > 0 (a NULL states when S > 0 too), prior and pcost both NULL, an output overlapping an input or the other output ("overlaps").  P == 0 is a no-op. */
int cpi_prior_relinearize_batch(cpi_ctx *ctx, int64_t S, int64_t P, const int32_t *idx,
                                const double *states, const double *anchor, const double *prior0,
                                double *prior, double *pcost);

/* cpi_chain_cost_batch: cost[c] = 0.5 sum_k chi2[ffirst_c + k] + sum_s pcost[first_c + s], the objective per chain.  C G S F first
 * count ffirst: those of cpi_chain_solve_batch, with the same defaults and clamps.  chi2 [F] (cpi_factor_cost_*; NULL only when
 * G == 1), pcost NULL (no priors) or [S], cost [C].  The reduction has a FIXED shape: sixteen slots q = 0 .. 15, a_q the plain sum from
 * +0.0 of the chain's chi2 at k = q, q + 16, ... ascending, b_q the same over pcost, v_q = 0.5 * a_q + b_q (the product and the sum
 * each rounded), then v_q = v_q + v_{q ^ 8}, ^ 4, ^ 2, ^ 1.  A chain without states gives +0.0; a chain whose factor rows leave
 * [0, F) (the solve's status -1 rule) gives NaN and reads nothing; NaN in any term gives NaN for that chain alone.
 * Refused: negative sizes, G < 1 or G > 2^31 - 1, a NULL cost, a NULL chi2 when G > 1, cost overlapping an input.  C == 0 is a no-op. */
int cpi_chain_cost_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                         const int64_t *first, const int32_t *count, const int64_t *ffirst,
                         const double *chi2, const double *pcost, double *cost);

/* cpi_chain_accept_batch: the decision.  params is a HOST pointer; NULL means { 0.1, 10, 0, 1e5, 1e-5, 1e-5 }: lambdaFactor 10 (down
 * by its inverse), lambdaLowerBound 0, lambdaUpperBound 1e5, absoluteErrorTol 1e-5, relativeErrorTol 1e-5 -- the defaults of GTSAM's
 * LevenbergMarquardtParams.  cost [C], states [S][16], lambda [C], phase [C] are in/out and required; chi2 [F] is in/out, or NULL
 * when the caller does not keep the current chi2; accepted is NULL or [C], out.  chi2_new / pcost_new / trial: the trial's.
 * Per chain (n_c: its clamped number of states):
 *     phase[c] != 0 on entry     -> nothing of the chain is written; accepted[c] = 0
 *     n_c == 0                   -> phase[c] = CPI_LM_CONVERGED, accepted[c] = 0, nothing else
 *     new = the value cpi_chain_cost_batch gives for (chi2_new, pcost_new), same bits;  cur = cost[c]
 *     new < cur (false for any NaN):
 *         the chain's rows of trial -> states and of chi2_new -> chi2, bit for bit; cost[c] = new
 *         lambda[c] = max(lambda[c] * lam_down, lam_min); accepted[c] = 1
 *         dec = cur - new; if dec <= abs_tol or dec <= rel_tol * |cur|: phase[c] = CPI_LM_CONVERGED
 *     otherwise (reject): states, chi2, cost untouched; accepted[c] = 0
 *         if |new - cur| <= max(abs_tol, rel_tol * |cur|): phase[c] = CPI_LM_CONVERGED (stalled inside the tolerance; lambda untouched)
 *         else l = lambda[c] * lam_up; if !(l <= lam_max): phase[c] = CPI_LM_GAVE_UP, lambda untouched; else lambda[c] = l
 * A failed solve (NaN delta, NaN trial, NaN cost) is a rejection with a larger lambda; a chain whose current cost is NaN climbs to
 * CPI_LM_GAVE_UP; neither disturbs another chain.  Rows of states that belong to no chain are not written.
 * Refused: the sizes as above; params outside 0 < lam_down <= 1 <= lam_up, 0 <= lam_min <= lam_max, a negative tolerance or a NaN in
 * any of them; a NULL cost / states / lambda / phase / trial, a NULL chi2_new when G > 1; trial / chi2_new / pcost_new or the
 * ranges overlapping an in/out array, or in/out arrays overlapping each other ("overlaps").  C == 0 is a no-op.
 *
 * Common to the three: every refusal is CPI_ERR_INVALID and comes before the context is looked at; the library allocates nothing;
 * one kernel on the context's stream, no host synchronisation: a capture is a chain without parallel branches.  A chain's or a
 * record's bits depend on its own data only, not on C, P or its position.  Alignment, for these three, cpi_state_fix_batch and every
 * other entry of the optimiser's loop (the factor sweeps, cpi_retract_batch, cpi_chain_solve / marginals / marginalize_batch): a
 * double array needs the alignment of a double (8 bytes) and no more -- [S][136] may be carved out of a workspace at an odd double
 * offset. */
typedef struct { double lam_down, lam_up, lam_min, lam_max, abs_tol, rel_tol; } cpi_lm_params;
enum { CPI_LM_RUNNING = 0, CPI_LM_CONVERGED = 1, CPI_LM_GAVE_UP = 2 };
int cpi_chain_accept_batch(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                           const int64_t *first, const int32_t *count, const int64_t *ffirst,
                           const cpi_lm_params *params,
                           const double *chi2_new, const double *pcost_new, const double *trial,
                           double *cost, double *states, double *chi2, double *lambda,
                           int32_t *phase, int32_t *accepted);

/* cpi_state_fix_batch: absolute measurements ("fixes") of states -- a GPS position, a zero-velocity update, an attitude, a mocap
 * pose -- added to the states' rows [Lam eta; . .] (the packing of prior: what cpi_chain_solve_batch takes) and to their cost (the
 * pcost of cpi_chain_cost_batch).  Replaces: GTSAM's PriorFactor<Point3 / Rot3 / Pose3> / GPSFactor linearised and summed into the
 * Hessian of a state, per state instead of per graph.  GTSAM is absent from the reference tree: PARITY UNPINNED; checked against a
 * long-double restatement of the definitions below and, where the summation order is fixed, bit for bit.  Out of scope: robust kernels
 * inside the library (weight is the caller's hook), measurements between non-adjacent states (the between-state measurements of
 * consecutive states are cpi_state_between_batch below), mixed kinds in one call (a second kind is
 * a second call), the exact right Jacobian of the rotation residual (it is taken flat, as cpi_prior_relinearize_batch takes it).
 *
 *   kind                 z row                              d   tangent rows sel (order theta bg v ba p)   residual e
 *   CPI_FIX_POSITION     [3] p                              3   12 13 14                                   z - x.p
 *   CPI_FIX_VELOCITY     [3] v                              3   6 7 8                                      z - x.v
 *   CPI_FIX_ORIENTATION  [4] JPL quaternion (a state's)     3   0 1 2                                      2 vec(qd), qd = quat_multiply(z, inv(x.q)),
 *                                                                                                          negated when qd.w < 0
 *   CPI_FIX_POSE         [7] q then p                       6   0 1 2 12 13 14                             the two above
 * e is the matching part of localCoordinates(x, x with z put in) -- the chart of every prior of the library -- with its Jacobian
 * taken flat (identity).  z and -z are one attitude and give the same e: the product is negated when its w is negative, which is
 * also what the library's localCoordinates (cpi_local_batch) does.  A zero-norm or NaN measurement gives NaN.
 *   mfirst  [S + 1] DEVICE int64: state s owns the fixes mfirst[s] .. mfirst[s + 1] - 1 (sorted by state, CSR).  Every range is
 *           clamped into [0, M] where it is read: a broken mfirst gives unspecified contents, no access out of bounds.
 *   states  [S][16];  z [M][3 | 3 | 4 | 7];  R [M][6 | 6 | 6 | 21]: the upper-triangular square-root information (R^T R = the inverse
 *           covariance of z) in the packing of R_tri, entry (i, k), i <= k, at i + k (k + 1) / 2;  weight NULL (1) or [M]
 *   base    NULL (zeros) or [S][136];  pcost_base NULL (zeros) or [S]
 * Per fix m of state s, in ascending m, with fma(a, b, c) one rounding of a b + c:
 *     wh_i  = the fma chain k = i .. d - 1 ascending from +0.0: acc = fma(R[i][k], e[k], acc)
 *     chi2  = (..(wh_0 wh_0 + wh_1 wh_1) + ..) + wh_{d-1} wh_{d-1}, every square rounded by itself
 *     u_a   = the fma chain i = 0 .. a ascending from +0.0: acc = fma(R[i][a], wh_i, acc)
 *     G_ab  = the fma chain i = 0 .. a ascending from +0.0: acc = fma(R[i][a], R[i][b], acc), a <= b
 *     Lam[sel_a][sel_b] = fma(w_m, G_ab, Lam[sel_a][sel_b]);  eta[sel_a] = fma(w_m, u_a, eta[sel_a]);  pcost = fma(0.5 w_m, chi2, pcost)
 *   out     NULL or [S][136]: for EVERY s in [0, S), out[s] = (base ? base[s] : 0) + the fixes of s; entry 135 is written as 0.0
 *   pcost   NULL or [S]: for every s, (pcost_base ? pcost_base[s] : 0) + sum 0.5 w chi2
 *   chi2    NULL or [M]: chi2[m] WITHOUT the weight, so that a gate does not depend on it
 * eta = Lam (z - x) is the negative gradient, the sign convention of the solve.  A state without fixes gets its base row and
 * pcost_base bit for bit (entry 135 aside), zeros when they are NULL.  The sweep is dense over S and never in place: a second
 * sensor is a second call with the first call's out / pcost as base / pcost_base, and the carried prior comes in as the base that
 * cpi_prior_relinearize_batch wrote; an in-place add would accumulate from one iteration of the loop to the next.  With out NULL
 * (the cost-only calls of an iteration) no row is read or written.  A NaN or zero-norm measurement makes that state's row and pcost
 * NaN and touches no other state; cpi_chain_cost_batch turns it into a rejection of that chain.
 * Refused (CPI_ERR_INVALID, before the context is looked at): negative sizes, an unknown kind, a NULL mfirst / states, a NULL z / R
 * when M > 0, out, pcost and chi2 all NULL, an output that overlaps an input or another output ("overlaps").  S == 0 is a no-op.
 * The library allocates nothing; one kernel on the context's stream, no host synchronisation: a capture is a chain
 * without parallel branches.  A state's bits depend on its own data only, not on S or its position. */
enum { CPI_FIX_POSITION = 0, CPI_FIX_VELOCITY = 1, CPI_FIX_ORIENTATION = 2, CPI_FIX_POSE = 3 };
int cpi_state_fix_batch(cpi_ctx *ctx, int64_t S, int64_t M, int32_t kind, const int64_t *mfirst,
                        const double *states, const double *z, const double *R,
                        const double *weight, const double *base,
                        const double *pcost_base, double *out,
                        double *pcost, double *chi2);

/* cpi_state_between_batch: measurements BETWEEN the two consecutive states x_i, x_j that IMU factor f joins -- a relative pose from
 * scan matching or visual odometry between two keyframes, a body-frame displacement from wheel odometry, a relative rotation --
 * added to the factor's augmented 31 x 31 row of cpi_factor_hessian_* ([G g; g^T f], hess [F][496]) and to its chi2
 * (cpi_factor_cost_*), so that cpi_chain_solve / marginals / marginalize / cost / accept_batch work as they are and the graph stays
 * block-tridiagonal.  Replaces: GTSAM's BetweenFactor<Pose3 / Rot3> (and a body-frame displacement factor) linearised and summed into
 * the Hessian of the pair, per factor instead of per graph.  GTSAM is absent from the reference tree: PARITY UNPINNED; checked against
 * a long-double restatement of the definitions below, central differences through a long-double retract and, where the summation
 * order is fixed, bit for bit.  Out of scope: measurements between non-adjacent states (loop closures, landmarks), robust kernels
 * inside the library (weight is the caller's hook), mixed kinds in one call, the exact right Jacobian of the rotation residual.
 *
 * With R_i = quat_2_Rot(x_i.q) (global to body i, JPL), R_ij = quat_2_Rot(x_j.q) R_i^T, y = R_i (p_j - p_i); tangent order theta bg v ba
 * p, state_i columns 0-14, state_j 15-29, the b column 30:
 *   kind                     z row                           d   residual e                                  touched columns of 31
 *   CPI_BETWEEN_POSITION     [3] position of j in body i     3   e_p = z - y                                  0 1 2 12 13 14 27 28 29 30       (55 of 496)
 *   CPI_BETWEEN_ORIENTATION  [4] JPL quaternion q_j (x) inv(q_i)  3   e_th = 2 vec(qd), qd = quat_multiply(z, inv(quat_multiply(x_j.q, inv(x_i.q)))),
 *                                                                negated when qd.w < 0                        0 1 2 15 16 17 30                (28 of 496)
 *   CPI_BETWEEN_POSE         [7] q then p                    6   the two above, rotation first                0 1 2 12 13 14 15 16 17 27 28 29 30  (91 of 496)
 * The Jacobian J [d][30], derivatives along cpi_retract_batch (the map every H1 / H2 of the library is a derivative along), checked
 * against central differences (tests/test_between_cpu.py):
 *   d e_p / d theta_i = -[y x]      d e_p / d p_i = R_i        d e_p / d p_j = -R_i
 *   d e_th / d theta_i = R_ij       d e_th / d theta_j = -I
 * The rotation residual's own right Jacobian is taken flat (identity), the rule of cpi_state_fix_batch and
 * cpi_prior_relinearize_batch: the rotation blocks are exact where e_th = 0; the position blocks are exact everywhere.  z and -z are
 * one rotation and give the same e.  A zero-norm or NaN z quaternion gives NaN.
 *   mfirst  [F + 1] DEVICE int64: factor f owns the measurements mfirst[f] .. mfirst[f + 1] - 1 (sorted by factor, CSR; the array
 *           Engine.fix_offsets builds).  Every range is clamped into [0, M] where it is read.
 *   states  [S][16];  idx_i / idx_j [F] int32 or NULL (f and f + 1: S >= F + 1) as in the factor sweeps, clamped into [0, S)
 *   z [M][3 | 4 | 7];  R [M][6 | 6 | 21]: the upper-triangular square-root information in the packing of R_tri, entry (r, k), r <= k,
 *           at r + k (k + 1) / 2;  weight NULL (1) or [M]
 *   hess_base NULL (zeros) or [F][496];  chi2_base NULL (zeros) or [F]
 * Per measurement m of factor f, in ascending m, with fma(a, b, c) one rounding of a b + c, b = -R e and [A | b] = [R J | -R e] over
 * the NC touched columns (structural zeros of J enter as +0.0):
 *     y_r    = the fma chain k = 0, 1, 2 from +0.0: acc = fma(R_i[r][k], (p_j - p_i)[k], acc);   e_p = z_p - y
 *     R_ij[a][b] = the fma chain k = 0, 1, 2 from +0.0: acc = fma(R_j[a][k], R_i[b][k], acc)
 *     wh_r   = the fma chain k = r .. d - 1 ascending from +0.0: acc = fma(R[r][k], e[k], acc)
 *     chi2_m = (..(wh_0 wh_0 + wh_1 wh_1) + ..) + wh_{d-1} wh_{d-1}, every square rounded by itself
 *     A_rc   = the fma chain k = r .. d - 1 ascending from +0.0: acc = fma(R[r][k], J[k][c], acc);  the b column: A_r = -wh_r
 *     P_ab   = the fma chain r = 0 .. d - 1 ascending from +0.0: acc = fma(A_ra, A_rb, acc), a <= b touched columns
 *     hess[f][(a, b)] = fma(w_m, P_ab, hess[f][(a, b)]);   chi2[f] = fma(w_m, chi2_m, chi2[f])
 * i.e. G += w A^T A, g += w A^T b (minus the gradient of 0.5 w chi2: the sign of cpi_factor_hessian_*), entry (30, 30) += w b^T b.
 *   hess    NULL or [F][496]: for EVERY f in [0, F), hess[f] = (hess_base ? hess_base[f] : 0) + the measurements of f; only the
 *           touched entries differ from the base.  NULL: the cost-only call of a trial step, no row is read or written
 *   chi2    NULL or [F]: for every f, (chi2_base ? chi2_base[f] : 0) + sum w chi2_m (cpi_chain_cost_batch halves the sum)
 *   chi2_m  NULL or [M]: |R e|^2 WITHOUT the weight, so that a gate does not depend on it
 * A factor without measurements gets its base row and base chi2 bit for bit, zeros when they are NULL.
 * IN PLACE: hess == hess_base and chi2 == chi2_base EXACTLY (the same pointer) are allowed and give the same bits as the out-of-place
 * call; then only the touched entries of factors with measurements are read and written.  This differs from cpi_state_fix_batch
 * deliberately: cpi_factor_hessian_* and cpi_factor_cost_* rewrite their arrays every iteration, so an in-place add does not
 * accumulate from one iteration to the next.  A second sensor is a second call.  A NaN or zero-norm measurement makes that factor's
 * row and chi2 NaN and touches no other factor.
 * Refused (CPI_ERR_INVALID, before the context is looked at): negative sizes, an unknown kind, a NULL mfirst / states, a NULL z / R
 * when M > 0, hess, chi2 and chi2_m all NULL, too few states, any other overlap of an output with an input or another output
 * ("overlaps").  F == 0 is a no-op.  The library allocates nothing; one kernel on the context's stream, no host synchronisation: a
 * capture is a chain without parallel branches.  A factor's bits depend on its own data only, not on F or its position.  A double
 * array needs the alignment of a double (8 bytes) and no more. */
enum { CPI_BETWEEN_POSITION = 0, CPI_BETWEEN_ORIENTATION = 1, CPI_BETWEEN_POSE = 2 };
int cpi_state_between_batch(cpi_ctx *ctx, int64_t F, int64_t M, int32_t kind, const int64_t *mfirst,
                            const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                            const double *z, const double *R, const double *weight,
                            const double *hess_base, const double *chi2_base,
                            double *hess, double *chi2, double *chi2_m);

/* ---- Device sets: the 8-GPU path of a single-process host (nothing in the reference, which is a
 * single-threaded CPU program).  Windows (and factors) are independent units: rank r of n owns the contiguous block
 * [lo, hi) = cpi_shard_bounds(W, r, n) (block size ceil(W / n); trailing ranks may be short or empty), runs the ordinary
 * entries above on cpi_group_ctx(g, r) with pointers into ITS device's memory, and the one exchange step is
 * cpi_group_gather: every peer sends its output slab straight to the root (ncclSend / ncclRecv inside one
 * ncclGroupStart / End, rccl/rccl.h:700-722,923-933 -- each peer has its own xGMI link to the root, so a direct gather
 * is link-parallel where a ring would be per-link bound), the root's own block is a device-to-device copy.
 * cpi_group_create makes one context + one non-blocking HIP stream per device and, for n > 1, one RCCL communicator per
 * device (ncclCommInitAll, rccl.h:236; librccl.so.1 -- or the path in the environment variable CPI_AMD_RCCL_LIB, read at
 * that moment only -- is bound then, never before; failure to bind it is CPI_ERR_RCCL).  devices NULL = 0 .. n-1.
 * All calls are asynchronous on the group's streams; cpi_group_synchronize waits for every device.
 * Multi-process hosts (one rank per GPU) use torch.distributed instead: cpi_amd/dist.py issues the same pattern. */
typedef struct cpi_group cpi_group;
int cpi_group_create(int n, const int *devices, cpi_group **out);
void cpi_group_destroy(cpi_group *g);
int cpi_group_size(const cpi_group *g);
cpi_ctx *cpi_group_ctx(cpi_group *g, int rank);                 /* borrowed; owned by the group */
const char *cpi_group_last_error(const cpi_group *g);           /* g may be NULL: last error of a failed create */
void cpi_shard_bounds(int64_t W, int rank, int n, int64_t *lo, int64_t *hi);
/* local[r] = the outputs of rank r's block (device pointers on device r, hi - lo windows each); root_out = arrays of W
 * windows on the root's device: rank r's block lands at window offset lo.  Every field that is non-NULL in root_out
 * must be non-NULL in every non-empty local[r].  local[root] may already point into root_out (no copy then).
 * When every peer's outputs are ONE SLAB (the wanted fields back to back, field-major over Wb >= hi - lo windows: what
 * cpi_outputs_bind_slab lays out) the exchange is ONE message per peer into a staging area on the root + one unpack
 * launch there; separately allocated fields cost one message per (peer, field), received in place.
 * cpi_group_last_gather_messages: messages per peer of the last gather (1 = slab path). */
int cpi_group_gather(cpi_group *g, int root, int64_t W, const cpi_outputs *local, const cpi_outputs *root_out);
int cpi_group_last_gather_messages(const cpi_group *g);
/* The exchange INSIDE one batch (ABI 3; DESIGN.md section 7 has the wire budget that asks for it: at configs[4]'s full-V1 outputs a
 * peer's slab is 1.4 - 2.2 GB over ONE xGMI link (18 - 29 ms at 76.8 GB/s one way), about as long as the 26 ms of kernels that produce it -- issued after them, all of it is
 * exposed).  Every rank's block is cut into `chunks` sub-blocks of cper = ceil(ceil(W / n) / chunks) windows
 * (cpi_shard_chunk_bounds: sub-block c of rank r = [lo_r + c cper, min(hi_r, lo_r + (c + 1) cper)); trailing ones may be short or
 * empty).  The host enqueues the ordinary entries for sub-block c on cpi_group_ctx(g, r) and then calls
 * cpi_group_gather_chunk(g, root, W, c, chunks, local_c, root_out): sub-block c of every rank travels to the root on the group's
 * EXCHANGE streams (a second non-blocking stream per device, made at the first use), behind everything that is enqueued on the
 * ranks' compute streams at the moment of the call -- and the compute streams stay free for sub-block c + 1, whose kernels
 * run while sub-block c is on the wire.  local_c[r] = the outputs of sub-block c of rank r, a slab of its own
 * (cpi_outputs_bind_slab over >= the sub-block's windows: ONE message per peer and chunk) or separately allocated fields;
 * root_out = arrays of W windows, as for cpi_group_gather.  The call with chunk == chunks - 1 JOINS: every rank's compute stream
 * waits for its exchange stream, so whatever is enqueued later on the contexts -- and cpi_group_synchronize, which also waits
 * for the exchange streams -- is ordered behind the whole exchange.  Buffers of sub-block c must not be rewritten before that
 * join (or a cpi_group_synchronize).  chunks == 1: cpi_group_gather, issued on the exchange streams. */
void cpi_shard_chunk_bounds(int64_t W, int rank, int n, int chunk, int chunks, int64_t *lo, int64_t *hi);
int cpi_group_gather_chunk(cpi_group *g, int root, int64_t W, int chunk, int chunks, const cpi_outputs *local_chunk,
                           const cpi_outputs *root_out);
/* Slab layout of an output set: the fields that are non-NULL in `mask`, back to back in the order of cpi_outputs (P_sym last:
 * a mask with P_sym instead of P makes the slab -- and the message a peer sends -- 840 bytes per window shorter), each over
 * Wb windows.  _slab_doubles: size of the slab; _bind_slab: *bound = mask's fields pointing into slab (others NULL). */
size_t cpi_outputs_slab_doubles(const cpi_outputs *mask, int64_t Wb);
int cpi_outputs_bind_slab(const cpi_outputs *mask, int64_t Wb, double *slab, cpi_outputs *bound);
int cpi_group_synchronize(cpi_group *g);

/* For host-side callers (the CpiV1-shaped C++ facade in cpi_amd/csrc/cpi_host.hpp): same as cpi_preintegrate_batch
 * but every pointer is a HOST pointer; stages through device memory owned by the context and returns when the outputs
 * are in host memory.  Dense batches (first == NULL) run as an upload / kernels / download pipeline over chunks of
 * <= 65536 windows: with PINNED host buffers (cpi_host_alloc, hipHostMalloc) the three overlap (PCIe is full duplex);
 * with pageable memory the result is the same, the copies serialise.  Lanes per window are chosen per chunk, so the
 * rounding of a window may differ from the device-pointer call on the whole batch (set prm->lanes_per_window to pin
 * it).  PCIe-inclusive, never the benchmarked path. */
int cpi_preintegrate_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                const double *knots, const int64_t *first, const int32_t *count,
                                int64_t n_knots, const double *lin, const double *q_k_lin,
                                const cpi_outputs *out);
/* cpi_preintegrate_running from host memory: every pointer a host pointer, n_knots as in cpi_preintegrate_batch_host; dense
 * batches run through the same upload / kernels / download pipeline, in chunks of <= 65536 rows. */
int cpi_preintegrate_running_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                  const double *knots, const int64_t *first, const int32_t *count,
                                  int64_t n_knots, const double *lin, const double *q_k_lin,
                                  const cpi_outputs *rows);
/* cpi_preintegrate_running_resume from host memory: every pointer a host pointer, n_knots as in cpi_preintegrate_batch_host.  Dense
 * batches run through the chunked pipeline of cpi_preintegrate_running_host (the records of a chunk go up and come down with
 * it; the rows and records do not depend on the chunking), ragged ones are staged whole. */
int cpi_preintegrate_running_resume_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                         const double *knots, const int64_t *first, const int32_t *count,
                                         int64_t n_knots, const double *lin, const double *q_k_lin,
                                         const double *carry_in, double *carry_out, const cpi_outputs *rows);
/* cpi_query_batch from host memory: every pointer a host pointer, n_knots as in cpi_preintegrate_batch_host, and NO rows
 * argument -- the windows are staged whole, the running means (and, for a Jacobian request, Jacobians) are computed into device
 * memory and stay there, the query kernel reads them and Q rows come down: the W * N rows never cross PCIe.  Validates what the
 * device form cannot, before anything is enqueued: every qwin[k] in [0, W), and finite non-decreasing stamps in every QUERIED
 * window (CPI_ERR_INVALID, the message names the window).  Bit for bit the device form on the same arguments. */
int cpi_query_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                         const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                         const double *lin, const double *q_k_lin,
                         int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);
/* cpi_query_cov_batch from host memory: the arguments, the staging and the validation of cpi_query_batch_host (its messages carry
 * this entry's name), with P / P_sym accepted in out.  The running rows stay in device staging, the covariance rows as P_sym (960 B
 * per row instead of 1 800): the staging need is W * N rows of 88 B (means) + 72 B per requested Jacobian field + 960 B when out
 * asks for P or P_sym, next to the windows and the Q output rows.  Bit for bit the device form on rows that hold P_sym. */
int cpi_query_cov_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                             const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                             const double *lin, const double *q_k_lin,
                             int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);
/* cpi_running_stj_batch from host memory: the arguments and the pipeline of cpi_preintegrate_running_host (its messages carry
 * this entry's name).  Bit for bit the device form on the same arguments and lanes_per_window. */
int cpi_running_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                               const double *knots, const int64_t *first, const int32_t *count,
                               int64_t n_knots, const double *lin, const double *q_k_lin,
                               const cpi_outputs *rows);
/* cpi_query_stj_batch from host memory: the arguments, the staging and the validation of cpi_query_cov_batch_host (its messages carry
 * this entry's name).  For a model-2 Jacobian request the W * N rows of all seven Jacobian fields (504 B per row) are computed by
 * cpi_running_stj_batch into device staging and stay there.  Bit for bit the device form on rows that hold P_sym. */
int cpi_query_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                             const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                             const double *lin, const double *q_k_lin,
                             int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);
/* cpi_running_resume_stj_batch from host memory: the arguments and the pipeline of cpi_preintegrate_running_resume_host (its
 * messages carry this entry's name).  Bit for bit the device form on the same arguments and lanes_per_window. */
int cpi_running_resume_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                      const double *knots, const int64_t *first, const int32_t *count,
                                      int64_t n_knots, const double *lin, const double *q_k_lin,
                                      const double *carry_in, double *carry_out, const cpi_outputs *rows);
/* cpi_query_open_batch from host memory, one chunk of a live loop in one call: host knots of the chunk (n_knots as in
 * cpi_preintegrate_batch_host), carry_in (NULL: the zero state) / carry_out in host memory, the queries and host outputs.  The base
 * rows are read out of carry_in (cpi_running_resume_stj_batch, N = 1, every count 0), the chunk's rows and carry_out come from
 * cpi_running_resume_stj_batch, then the device entry runs with base_N = 1; all rows stay in device staging, Q rows and the records
 * come down.  carry_in must hold what the request of out needs (covariance state for P / P_sym or model-2 Jacobians, analytic
 * Jacobians for model-1 Jacobians).  qwin and the stamps are validated as in cpi_query_batch_host.  Q == 0 still advances the
 * record.  Bit for bit the device composition on rows that hold P_sym. */
int cpi_query_open_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                              const double *knots, const int64_t *first, const int32_t *count, int64_t n_knots,
                              const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out,
                              int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out);
/* cpi_merge_batch from host memory: the same arguments, every array a host pointer; synchronous.  Only the fields of `in` that the
 * request reads are uploaded.  The dense layout (first == NULL) with every group inside in_rows runs through the chunked upload /
 * kernel / download pipeline of the other _host entries (the G operand rows of a group travel with it); a ragged layout is staged
 * whole.  Bit for bit the device form on the same arguments (a group's result does not depend on the chunking). */
int cpi_merge_batch_host(cpi_ctx *ctx, int32_t model, int64_t M, int32_t G, int64_t in_rows, const cpi_outputs *in,
                         const int64_t *first /*[M] or NULL*/, const int32_t *count /*[M] or NULL*/, const cpi_outputs *out);
/* cpi_preintegrate_resume from host memory: every pointer a host pointer, n_knots as in cpi_preintegrate_batch_host. */
int cpi_preintegrate_resume_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N,
                                 const double *knots, const int64_t *first, const int32_t *count,
                                 int64_t n_knots, const double *lin, const double *q_k_lin,
                                 const double *carry_in, double *carry_out, const cpi_outputs *out);
/* The tiled layout from HOST memory (tiles written by a host-side assembler), mean outputs only: same pipeline, chunks of
 * 1024 tiles. */
int cpi_preintegrate_tiled_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *tiles,
                                      const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *out);
/* page-locked host memory for the entries above (hipHostMalloc / hipHostFree); NULL when the allocation fails */
/* cpi_preintegrate_stream with HOST pointers -- what a caller shaped like GraphSolver::createimufactor_cpi_v1/v2
 * (GraphSolver_IMU.cpp:34-134) holds: its IMU deque as one array stream[K][7], the update times of the states it creates,
 * one linearisation point per window; the measurements of every window come back in host memory.  count (may be NULL)
 * receives the TRUE interval count of every window (> N: that window was truncated to N intervals).  The stream is uploaded
 * once, whole; the windows are cut on the device.  PCIe-inclusive, never the benchmarked path. */
int cpi_preintegrate_stream_host(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                 const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                 const cpi_outputs *out, int32_t *count);
/* cpi_preintegrate_streams with HOST pointers (pageable or pinned); count (may be NULL) receives the TRUE interval count of
 * every window.  The offsets ARE validated here: an array that does not start at 0, decreases or does not end at K /
 * U returns CPI_ERR_INVALID before anything is enqueued.  Uploads the runs once, whole; PCIe-inclusive, never the benchmarked
 * path. */
int cpi_preintegrate_streams_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                  const int64_t *stream_offsets, int64_t U, const double *update_times,
                                  const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                  const cpi_outputs *out, int32_t *count);
/* cpi_preintegrate_stream_running / cpi_preintegrate_streams_running with HOST pointers (pageable or pinned): the stream(s) are
 * uploaded once, whole, and cut on the device; rows holds U * N rows in host memory and comes back in chunks of whole windows,
 * never more than 2^18 rows each (N <= 65535: at least 4 windows), so that the device staging stays bounded whatever N is -- the
 * rows do not depend on the chunking.  count (may be NULL)
 * receives the TRUE interval count of every window.  The multi-stream form validates the offsets as
 * cpi_preintegrate_streams_host does.  PCIe-inclusive, never the benchmarked path. */
int cpi_preintegrate_stream_running_host(cpi_ctx *ctx, const cpi_params *prm, int64_t K, const double *stream, int64_t U,
                                         const double *update_times, int32_t N, const double *lin, const double *q_k_lin,
                                         const cpi_outputs *rows, int32_t *count);
int cpi_preintegrate_streams_running_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                          const int64_t *stream_offsets, int64_t U, const double *update_times,
                                          const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                          const cpi_outputs *rows, int32_t *count);
/* cpi_stream_running_stj_batch with HOST pointers: the staging and chunking of cpi_preintegrate_stream[s]_running_host (its
 * messages carry this entry's name).  Bit for bit the device form. */
int cpi_stream_running_stj_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                      const int64_t *stream_offsets, int64_t U, const double *update_times,
                                      const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                      const cpi_outputs *rows, int32_t *count);
/* cpi_query_stream_batch from host memory: stream, offsets, update times, lin, q_k_lin, qrun and qtime are host pointers, and there
 * is no rows and no workspace argument -- the stream(s) are staged whole, cpi_stream_running_stj_batch computes the rows into device
 * staging (the covariance rows as P_sym), Q rows and qwin_out (may be NULL) come down.  Validates what the device form cannot,
 * before anything is enqueued: the offsets, and every qrun[k] in [0, R).  Bit for bit the device form on rows that hold P_sym. */
int cpi_query_stream_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t R, int64_t K, const double *stream,
                                const int64_t *stream_offsets, int64_t U, const double *update_times,
                                const int64_t *update_offsets, int32_t N, const double *lin, const double *q_k_lin,
                                int64_t Q, const int32_t *qrun, const double *qtime, int32_t *qwin_out, const cpi_outputs *out);
void *cpi_host_alloc(size_t bytes);
void cpi_host_free(void *p);
int cpi_factor_eval_batch_host(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                               const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                               const double *states, int64_t S, const int32_t *idx_i,
                               const int32_t *idx_j, double *err, double *H1, double *H2);

/* cpi_retract_batch / cpi_local_batch from host memory: every pointer a host pointer, synchronous, the same rules (states_out may
 * equal states_in); the device forms' bits. */
int cpi_retract_batch_host(cpi_ctx *ctx, int64_t S, const double *states_in, const double *delta, double *states_out);
int cpi_local_batch_host(cpi_ctx *ctx, int64_t S, const double *x, const double *other, double *xi);
/* GTSAM's factor.error(values) for F factors in ONE call, from host memory: the covariance of each measurement -- meas->P_sym when
 * set, else the dense meas->P, whose upper triangle is packed first -- is factorised on the device
 * (cpi_sqrt_information_packed_batch) and cpi_factor_cost_tri_batch runs on the result.  idx_i / idx_j are validated as
 * cpi_factor_eval_batch_host validates them.  chi2 [F] required, werr [F][15] or NULL, total [1] or NULL (0.5 * sum chi2; no
 * workspace: the staging holds it).  Synchronous. */
int cpi_factor_cost_batch_host(cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F,
                               const cpi_outputs *meas, const double *lin, const double *q_k_lin,
                               const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                               double *chi2, double *werr, double *total);

/* cpi_chain_solve_batch from host memory: every pointer a host pointer (lambda too), no workspace, synchronous; the device form's
 * bits.  Every chain's state range and factor range is validated first: a chain whose states leave [0, S) or whose factor rows
 * leave [0, F) is CPI_ERR_INVALID, the text names the chain.  Rows of delta that belong to no chain keep the caller's values. */
int cpi_chain_solve_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                               const int64_t *first, const int32_t *count, const int64_t *ffirst,
                               const double *hess, const double *prior, const double *lambda, int32_t damping,
                               double *delta, int32_t *status);

/* cpi_chain_marginals_batch from host memory: every pointer a host pointer, synchronous.  The UNDAMPED system of hess and prior
 * (the arguments of cpi_chain_solve_batch_host with lambda = NULL) is factorised on the device by the solve, the marginals kernel
 * runs on its workspace, and cov [S][120], cross (NULL or [S][225]) and status (NULL or [C], the solve's codes) come back: the device
 * forms' bits.  A chain that failed has NaN rows whether status is given or not.  Every chain's state range and factor range is
 * validated first as in cpi_chain_solve_batch_host, and the text names the chain.  Rows of cov / cross that are not written keep the
 * caller's values. */
int cpi_chain_marginals_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                   const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                   const double *hess, const double *prior,
                                   double *cov, double *cross, int32_t *status);

/* cpi_chain_marginalize_batch from host memory: every pointer a host pointer (drop too), synchronous; the device form's bits.
 * Every chain's state range and factor range is validated first as in cpi_chain_solve_batch_host, and so is its m_c: a chain with
 * states whose m_c is outside [0, n_c) is CPI_ERR_INVALID, the text names the chain.  (A chain without states is not an error
 * here: it gets status -1 and a NaN row, as in the device form.) */
int cpi_chain_marginalize_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                     const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                     const double *hess, const double *prior,
                                     int32_t M, const int32_t *drop,
                                     double *out, int32_t *status);

/* cpi_chain_condense_batch and cpi_chain_expand_batch from host memory: every pointer a host pointer, synchronous; the device forms'
 * bits.  Every chain's state range (condense: and factor range) is validated first as in cpi_chain_solve_batch_host, and the text
 * names the chain.  The workspace is a HOST array too: workspace_out (NULL: not wanted) receives the records the condense left, and
 * the expand form takes that array.  Rows that are not written keep the caller's values. */
int cpi_chain_condense_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                  const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                  const double *hess, const double *prior, const double *lambda, int32_t damping, int64_t K,
                                  double *rhess, double *rprior, int32_t *rcount,
                                  int32_t *status, double *workspace_out);
int cpi_chain_expand_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S,
                                const int64_t *first, const int32_t *count, int64_t K,
                                const double *rdelta, const double *workspace, double *delta);

/* cpi_prior_relinearize_batch, cpi_chain_cost_batch and cpi_chain_accept_batch from host memory: every pointer a host pointer (idx
 * too), synchronous; the device forms' bits.  The outputs and in/out arrays travel up before the kernel, so that what nobody writes
 * comes back as the caller left it.  The two chain entries validate every chain's state range and factor range first as
 * cpi_chain_solve_batch_host does, and the text names the chain. */
int cpi_prior_relinearize_batch_host(cpi_ctx *ctx, int64_t S, int64_t P, const int32_t *idx,
                                     const double *states, const double *anchor, const double *prior0,
                                     double *prior, double *pcost);
int cpi_chain_cost_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                              const int64_t *first, const int32_t *count, const int64_t *ffirst,
                              const double *chi2, const double *pcost, double *cost);
int cpi_chain_accept_batch_host(cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F,
                                const int64_t *first, const int32_t *count, const int64_t *ffirst,
                                const cpi_lm_params *params,
                                const double *chi2_new, const double *pcost_new, const double *trial,
                                double *cost, double *states, double *chi2, double *lambda,
                                int32_t *phase, int32_t *accepted);

/* cpi_state_fix_batch from host memory: every pointer a host pointer (mfirst too), synchronous; the device form's bits.  mfirst is
 * validated first -- non-decreasing and inside [0, M] -- and the text names the state. */
int cpi_state_fix_batch_host(cpi_ctx *ctx, int64_t S, int64_t M, int32_t kind, const int64_t *mfirst,
                             const double *states, const double *z, const double *R,
                             const double *weight, const double *base,
                             const double *pcost_base, double *out,
                             double *pcost, double *chi2);

/* cpi_state_between_batch from host memory: every pointer a host pointer (mfirst and the indices too), synchronous; the device form's
 * bits, the in-place forms included.  mfirst -- non-decreasing and inside [0, M] -- and the state indices are validated first, and
 * the text names the factor. */
int cpi_state_between_batch_host(cpi_ctx *ctx, int64_t F, int64_t M, int32_t kind, const int64_t *mfirst,
                                 const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j,
                                 const double *z, const double *R, const double *weight,
                                 const double *hess_base, const double *chi2_base,
                                 double *hess, double *chi2, double *chi2_m);

#ifdef __cplusplus
}
#endif
#endif /* CPI_AMD_H */
