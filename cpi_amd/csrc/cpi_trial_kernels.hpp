// cpi_trial_kernels.hpp -- the optimiser's trial step: batched retract / localCoordinates of JPLNavState and the whitened cost of
// the IMU factors at trial states (0.5 |R e|^2: GTSAM's NoiseModelFactor::error), with its deterministic total.
// Part of the translation unit cpi_trial.hip (included there after cpi_math.hpp / cpi_device_util.hpp / cpi_factor_kernels.hpp; not a
// stand-alone header).  From cpi_factor_kernels.hpp it takes the record layout (fin::), factor_fetch_inputs, factor_meas_of and, out
// of cpi_math.hpp, factor_shared_core -- unchanged, so the residual is the one cpi_factor_eval_batch computes.
#pragma once

namespace {

// ============================================================================================
// retract / localCoordinates: copies with a little arithmetic in them (248 bytes in, 128 out per state; 256 in, 120 out), moved the
// way cpi_predict_kernel moves its records: one wavefront per 64 states, ONE burst of fully coalesced pieces -- the states as
// 16-byte pieces, eight lanes per state; the deltas as consecutive doubles -- all requested before the first is used, parked in
// LDS record-major at an odd pitch (the per-lane record reads hit distinct banks), one lane per state for the arithmetic, and the
// results leave through the same area as consecutive 16-byte non-temporal stores.
// In place (states_out == states_in): a wavefront has read all of its 64 records before it stores the first result, and no other
// wavefront touches them.
// ============================================================================================
constexpr int RETR_IN_D = 31, RETR_OUT_D = 17;    // state 16 + delta 15 (odd); result 16 (+1: odd)
constexpr int LOCAL_IN_D = 33, LOCAL_OUT_D = 15;  // x 16 + other 16 (+1: odd); xi 15: the stage IS the output layout

struct __attribute__((packed, aligned(8))) trial_d2u { double a, b; };

// 64 state records of one array -> LDS (record fl at sRec + fl * pitch + off): piece p = lane + 64 r is part p & 7 of record p >> 3
struct StateBurst {
    trial_d2u st[8];
    __device__ __forceinline__ void load(const double *states, long long f0, int nf, int lane) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const long long ff = f0 + min((lane >> 3) + 8 * r, nf - 1);
            st[r] = *reinterpret_cast<const trial_d2u *>(states + ff * 16 + 2 * (lane & 7));
        }
    }
    __device__ __forceinline__ void store(double *sRec, int pitch, int off, int lane) const {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            double *d = sRec + ((lane >> 3) + 8 * r) * pitch + off + 2 * (lane & 7);
            d[0] = st[r].a; d[1] = st[r].b;
        }
    }
};
__device__ __forceinline__ void state_to_stage(double *d, const NavState &o) {
    d[0] = o.q.x; d[1] = o.q.y; d[2] = o.q.z; d[3] = o.q.w;
    stv3(d + 4, o.bg); stv3(d + 7, o.v); stv3(d + 10, o.ba); stv3(d + 13, o.p);
}

__global__ __launch_bounds__(64) void cpi_retract_kernel(long long S, const double *states_in, const double *delta, double *states_out) {
    constexpr int FPW = 64;
    __shared__ __attribute__((aligned(16))) double sRec[FPW * RETR_IN_D];
    static_assert(FPW * RETR_OUT_D <= FPW * RETR_IN_D, "the results re-use the record area");
    const int lane = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
    const int nf = (int)min((long long)FPW, S - f0);
    StateBurst sb;
    FieldFetch<FPW, 15> fd;
    sb.load(states_in, f0, nf, lane);
    fd.load(delta, f0, nf, lane);
    sb.store(sRec, RETR_IN_D, 0, lane);
    fd.store(sRec, RETR_IN_D, 16, lane);
    wave_lds_fence();
    // ---- lane = state (lanes past the last state redo it: same values, and they do not store)
    NavState o;
    {
        const double *rec = sRec + min(lane, nf - 1) * RETR_IN_D;
        double d[15];
#pragma unroll
        for (int i = 0; i < 15; i++) d[i] = rec[16 + i];
        o = retract_state(ld_state(rec), d);
    }
    wave_lds_fence();   // every record is read (in-order DS) before the area becomes the output stage
    state_to_stage(sRec + lane * RETR_OUT_D, o);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int fl = (lane >> 3) + 8 * r;
        const double *src = sRec + fl * RETR_OUT_D + 2 * (lane & 7);
        if (fl < nf) st16_nt(states_out + (f0 + fl) * 16 + 2 * (lane & 7), src[0], src[1]);
    }
}

__global__ __launch_bounds__(64) void cpi_local_kernel(long long S, const double *x, const double *other, double *xi) {
    constexpr int FPW = 64;
    __shared__ __attribute__((aligned(16))) double sRec[FPW * LOCAL_IN_D];
    const int lane = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * FPW;
    const int nf = (int)min((long long)FPW, S - f0);
    StateBurst sx, so;
    sx.load(x, f0, nf, lane);
    so.load(other, f0, nf, lane);
    sx.store(sRec, LOCAL_IN_D, 0, lane);
    so.store(sRec, LOCAL_IN_D, 16, lane);
    wave_lds_fence();
    double out[15];
    {
        const double *rec = sRec + min(lane, nf - 1) * LOCAL_IN_D;
        local_coordinates(ld_state(rec), ld_state(rec + 16), out);
    }
    wave_lds_fence();   // every record is read before the area becomes the output stage
#pragma unroll
    for (int i = 0; i < 15; i++) sRec[lane * LOCAL_OUT_D + i] = out[i];
    wave_lds_fence();
    // the nf rows of xi are one contiguous run of the output: consecutive lanes = consecutive 16-byte pieces
    const int n = nf * LOCAL_OUT_D, n2 = n >> 1;
    double *dst = xi + f0 * LOCAL_OUT_D;
    for (int i = lane; i < n2; i += 64) st16_nt(dst + 2 * i, sRec[2 * i], sRec[2 * i + 1]);
    if ((n & 1) && lane == 0) dst[n - 1] = sRec[n - 1];
}

// ============================================================================================
// cost of a factor at the current states: werr = R e (e: the residual of cpi_factor_eval_batch), chi2 = |werr|^2.
// LPF lanes per factor, FPW = 64 / LPF factors per wavefront.
//   fetch     factor_fetch_inputs<MODEL, FPW, true, RD>: de-duplicated, cooperative, every load issued before the first LDS write;
//             state indices clamped into [0, S); R dense [225] or the packed triangle [120] (TRI) beside the records in LDS
//   core      lane 0 of a factor runs factor_shared_core<MODEL> and leaves the fifteen residual entries in the stage (the other
//             lanes sit it out: the same instructions for the wavefront, 1 / LPF of the FP64 lanes switching)
//   werr      lane q owns rows q, q + LPF, ...: whiten_row (cpi_math.hpp) -- row i accumulates R[i][k] e[k] over k = i .. 14
//             ascending as one fma chain from zero, the loop of cpi_factor_kernel's whitening, so werr is bit for bit the err of
//             cpi_factor_eval_whitened[_tri]_batch
//   chi2      lane l < nf sums the fifteen squares of factor f0 + l: chi2_of (cpi_math.hpp) -- every square rounded by itself,
//             added in ascending order, left to right: chi2 = (..((w0 w0 + w1 w1) + w2 w2) + ..) + w14 w14
//   stores    chi2: consecutive lanes = consecutive doubles; werr (optional): the wavefront's FPW x 15 doubles are one contiguous
//             run, consecutive lanes = consecutive 16-byte pieces.  Nothing is written past F.
// There is no store-shaping reason for sixteen lanes here (8 or 128 bytes per factor leave, not 3.7 KB); what LPF trades is LDS per
// wavefront (records + R: 1.9 KB per factor with R packed) against idle lanes during the core.  The launcher's choice and the
// measurement behind it: cpi_abi.hip, cost_lanes() (profiles/trial_step.md).
// ============================================================================================
struct CostOut { double *chi2; double *werr; };

// __launch_bounds__ asks for 4 / 2 / 1 wavefronts per SIMD (16 / 8 / 4 lanes): what the LDS of the DENSE instances allows (11.4 /
// 22.8 / 45.6 KB per wavefront; resource_usage_trial.txt shows occupancy 4 / 2 / 1 for them).  The packed instances (8.0 / 16.1 /
// 32.1 KB) reach 5 / 3 / 2, more than the bound asks for: a bound is a minimum, and the registers (64 .. 198, no scratch) are far
// from limiting either.
template <int MODEL, bool TRI, int LPF>
__global__ __launch_bounds__(64, LPF == 16 ? 4 : (LPF == 8 ? 2 : 1)) void cpi_factor_cost_kernel(FactorArgs A, CostOut O) {
    constexpr int FPW = 64 / LPF;
    constexpr int CPL = (15 + LPF - 1) / LPF;          // rows per lane
    constexpr int RD = TRI ? CPI_TRI_DOUBLES : 225;
    constexpr int IN_D = fin::IN_D;
    __shared__ __attribute__((aligned(16))) double sIn[FPW * IN_D];
    __shared__ __attribute__((aligned(16))) double sR[FPW * RD];
    __shared__ __attribute__((aligned(16))) double se[FPW * 15 + 1];
    const int lane = threadIdx.x;
    const int q = lane % LPF, fl = lane / LPF;
    const long long f0 = (long long)blockIdx.x * FPW;
    const int nf = (int)min((long long)FPW, A.F - f0);

    factor_fetch_inputs<MODEL, FPW, true, RD>(A, f0, nf, lane, sIn, sR);
    __syncthreads();
    if (q == 0) {
        const FactorMeas m = factor_meas_of(sIn + fl * IN_D, A.grav);
        FactorShared S;
        V3 e5[5];
        factor_shared_core<MODEL>(m, S, e5);
#pragma unroll
        for (int a = 0; a < 5; a++) put3(se + fl * 15 + 3 * a, e5[a]);
    }
    wave_lds_fence();
    const double *Rf = sR + fl * RD;
    double acc[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) acc[k] = whiten_row<TRI>(Rf, se + fl * 15, min(q + LPF * k, 14));
    wave_lds_fence();   // every lane has read the residual before werr takes its place
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const int c = q + LPF * k;
        if (c < 15) se[fl * 15 + c] = acc[k];
    }
    wave_lds_fence();
    if (lane < nf) O.chi2[f0 + lane] = chi2_of(se + lane * 15);
    if (O.werr) {
        const int n = nf * 15, n2 = n >> 1;
        double *dst = O.werr + f0 * 15;
        for (int i = lane; i < n2; i += 64) st16_nt(dst + 2 * i, se[2 * i], se[2 * i + 1]);
        if ((n & 1) && lane == 0) dst[n - 1] = se[n - 1];
    }
}

// ============================================================================================
// total = 0.5 sum_f chi2[f]: a reduction of FIXED shape, no floating-point atomics -- the same inputs give the same bits on every run.
//   cpi_cost_partial_kernel   workgroup b sums chi2[b * COST_CHUNK .. + COST_CHUNK): thread t adds its elements t, t + 256, ... in
//                             ascending order, then a binary tree over the 256 threads in LDS (stride 128, 64, ..., 1)
//   cpi_cost_final_kernel     ONE workgroup sums n values the same way (thread t: t, t + 256, ...; the same tree) and writes
//                             scale * sum to dst[0]
// F <= COST_DIRECT: the final kernel alone, on chi2.  Larger: partial sums into workspace[1 ..], then the final kernel over them.
// An element past the end contributes +0.0 (chi2 >= 0: the sum is unchanged bit for bit); a NaN anywhere makes the total NaN.
// ============================================================================================
constexpr int COST_CHUNK = 4096, COST_DIRECT = 32768;
__device__ __forceinline__ double cost_block_sum(double v, double *sRed) {
    const int t = threadIdx.x;
    sRed[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) sRed[t] = sRed[t] + sRed[t + s];
        __syncthreads();
    }
    return sRed[0];
}
__global__ __launch_bounds__(256) void cpi_cost_partial_kernel(long long n, const double *src, double *partial) {
    __shared__ double sRed[256];
    const long long base = (long long)blockIdx.x * COST_CHUNK;
    const int m = (int)min((long long)COST_CHUNK, n - base);
    double v = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) v = v + src[base + i];
    const double s = cost_block_sum(v, sRed);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void cpi_cost_final_kernel(long long n, const double *src, double scale, double *dst) {
    __shared__ double sRed[256];
    double v = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) v = v + src[i];
    const double s = cost_block_sum(v, sRed);
    if (threadIdx.x == 0) dst[0] = scale * s;
}

}  // namespace
