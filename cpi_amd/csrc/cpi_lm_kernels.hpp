// cpi_lm_kernels.hpp -- the Levenberg-Marquardt step per chain: cpi_lm_prior_kernel (cpi_prior_relinearize_batch: the prior at the
// current states and its cost), cpi_lm_cost_kernel (cpi_chain_cost_batch: the objective per chain) and cpi_lm_accept_kernel
// (cpi_chain_accept_batch: accept or reject, copy, lambda, phase).  The arithmetic: cpi_math.hpp, chn::prior_eta_row / prior_cost,
// chain_cost_slot and its butterfly, lm_decide.  Part of the translation unit cpi_lm.hip (included there after cpi_math.hpp /
// cpi_device_util.hpp / cpi_factor_kernels.hpp -- ld_state -- and cpi_chain_util.hpp -- chain_range; not a stand-alone header).
#pragma once

namespace {

// a 16-byte piece of a row on its way through a lane (the rows are 8-byte aligned)
struct __attribute__((packed, aligned(8))) lm_d2u { double a, b; };

// ============================================================================================
// cpi_lm_prior_kernel: cpi_local_kernel's shape (cpi_trial_kernels.hpp) with SIXTEEN lanes per record, four records per wavefront,
// one wavefront per workgroup.
//   fetch     lanes 0 .. 7 of a record one 16-byte piece of its state each, lanes 8 .. 15 of its anchor, and every lane pieces j,
//             j + 16, ... of the 68 of its prior0 row: six loads per lane, all requested before the first LDS write.  A record that
//             is skipped (past P, or its index outside [0, S)) loads nothing.
//   LDS       record-major [state 16 | anchor 16 | prior0 136] at pitch 169 (odd): 5.4 KB per wavefront, plus the 64 doubles of t
//   xi        every lane of a record runs local_coordinates on the record's two states (one quaternion product and twelve
//             differences: cheaper than an exchange), so xi sits in registers where the chains want it
//   eta, t    lane i < 15 owns row i: chn::prior_eta_row over the packed row in LDS (lane 15 redoes row 14 and stores nothing of it)
//   pcost     lane 0 of a record runs chn::prior_cost over the fifteen t it reads back from LDS
//   stores    eta takes the place of eta0 in the staged row, entry 135 becomes 0.0, and the row leaves as 68 contiguous 16-byte
//             non-temporal stores, lane j pieces j, j + 16, ...; pcost is one double per record
// Sixteen lanes rather than one per record: a lane that walked 120 doubles of Lam alone would need 64 x 169 doubles of LDS per
// wavefront (86 KB) and leave the rows as 64 scattered streams; sixteen keep a row's fetch and its stores whole cache lines and the
// fifteen chains independent.  74 VGPRs, no scratch, 5920 bytes of LDS, six wavefronts per SIMD (resource_usage_lm.txt).
// ============================================================================================
constexpr int LMP_D = 16 + 16 + chn::PRIOR_D + 1, LMP_NP = chn::PRIOR_D / 2, LMP_NR = (LMP_NP + 15) / 16;

__global__ __launch_bounds__(64) void cpi_lm_prior_kernel(LmPriorArgs A) {
    __shared__ __attribute__((aligned(16))) double sRec[4 * LMP_D];
    __shared__ double sT[64];
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4;
    const long long p = (long long)blockIdx.x * 4 + fl;
    long long s = -1;
    if (p < A.P) s = A.idx ? (long long)A.idx[p] : p;
    const bool live = s >= 0 && s < A.S;
    lm_d2u x = {0.0, 0.0}, pr[LMP_NR];
#pragma unroll
    for (int r = 0; r < LMP_NR; r++) pr[r] = x;
    if (live) {
        x = *reinterpret_cast<const lm_d2u *>((j < 8) ? A.states + s * 16 + 2 * j : A.anchor + p * 16 + 2 * (j - 8));
#pragma unroll
        for (int r = 0; r < LMP_NR; r++)
            pr[r] = *reinterpret_cast<const lm_d2u *>(A.prior0 + p * chn::PRIOR_D + 2 * min(j + 16 * r, LMP_NP - 1));
    }
    double *rec = sRec + fl * LMP_D, *P0 = rec + 32;
    rec[2 * j] = x.a; rec[2 * j + 1] = x.b;
#pragma unroll
    for (int r = 0; r < LMP_NR; r++) {
        const int i = min(j + 16 * r, LMP_NP - 1);     // the lanes past piece 67 write piece 67 again: the same values
        P0[2 * i] = pr[r].a; P0[2 * i + 1] = pr[r].b;
    }
    wave_lds_fence();
    double xi[15];
    local_coordinates(ld_state(rec), ld_state(rec + 16), xi);
    const int i = min(j, 14);
    const double eta = chn::prior_eta_row(P0, xi, i);
    const double t = eta + P0[chn::tri(15) + i];
    wave_lds_fence();                                  // every row is read before eta takes the place of eta0
    if (j < 15) P0[chn::tri(15) + j] = eta; else P0[chn::PRIOR_D - 1] = 0.0;
    sT[lane] = t;
    wave_lds_fence();
    if (!live) return;
    if (A.pcost && j == 0) A.pcost[s] = chn::prior_cost(xi, sT + 16 * fl);
    if (A.prior) {
        double *dst = A.prior + s * chn::PRIOR_D;
#pragma unroll
        for (int r = 0; r < LMP_NR; r++) {
            const int k = j + 16 * r;
            if (k < LMP_NP) st16_nt(dst + 2 * k, P0[2 * k], P0[2 * k + 1]);
        }
    }
}

// ============================================================================================
// The objective of a chain: 16 lanes (slots) per chain, 4 chains per wavefront, the mapping of the solver family.  Lane q sums its
// slot of the chain's chi2 and pcost rows (chn::chain_cost_slot: consecutive lanes read consecutive doubles), then the butterfly
// over the sixteen lanes with __shfl_xor 8, 4, 2, 1: every lane of a chain ends with the same bits.  Every lane of the wavefront
// takes part in the exchanges, chains past C and chains without states included (they sum nothing: +0.0).  A chain whose factor rows
// leave [0, F) (chain_range: bad) reads nothing and gets NaN.
// ============================================================================================
__device__ __forceinline__ double lm_chain_cost(const LmCostArgs &A, const ChainRange &cs, int q) {
    const int n = cs.bad ? 0 : cs.n;
    const double *x2 = (A.chi2 && n > 1) ? A.chi2 + cs.ff : nullptr, *pc = (A.pcost && n > 0) ? A.pcost + cs.f : nullptr;
    double v = chn::chain_cost_slot(n, x2, pc, q);
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) v = v + __shfl_xor(v, s);
    return cs.bad ? __builtin_nan("") : v;
}

// 18 VGPRs, no scratch, no LDS
__global__ __launch_bounds__(64) void cpi_lm_cost_kernel(LmCostArgs A) {
    const int lane = threadIdx.x, q = lane & 15, fl = lane >> 4;
    const long long c = (long long)blockIdx.x * 4 + fl;
    const ChainRange cs = chain_range(A, c);
    const double v = lm_chain_cost(A, cs, q);
    if (c < A.C && q == 0) A.cost[c] = v;
}

// ============================================================================================
// cpi_lm_accept_kernel: the trial's objective as cpi_lm_cost_kernel computes it, then chn::lm_decide.  Lane 0 of a chain reads
// phase, cost and lambda and decides; the decision reaches the other fifteen lanes through __shfl BEFORE anything is written, so no
// lane reads a value a mate has already replaced.  An accepted chain's sixteen lanes copy its rows of trial -> states as 16-byte
// pieces, lane q pieces q, q + 16, ... (eight loads in flight per lane per trip), and its chi2 rows; lane 0 writes cost, lambda, phase
// and accepted.  A chain that is not running (phase != 0) writes nothing but accepted = 0.  72 VGPRs, no LDS, no scratch.
// ============================================================================================
__global__ __launch_bounds__(64) void cpi_lm_accept_kernel(LmCostArgs A, LmAcceptArgs B) {
    const int lane = threadIdx.x, q = lane & 15, fl = lane >> 4;
    const long long c = (long long)blockIdx.x * 4 + fl;
    const ChainRange cs = chain_range(A, c);
    const double nw = lm_chain_cost(A, cs, q);
    const bool mine = c < A.C && q == 0;
    int rule = 0, ph = 0, acc = 0;                     // rule: 0 the chain is frozen, 1 it ran through lm_decide, 2 it has no states
    double lam = 0.0;
    if (mine && B.phase[c] == 0) {
        if (cs.n > 0) {
            chn::LmParams P;
            P.lam_down = B.p.lam_down; P.lam_up = B.p.lam_up; P.lam_min = B.p.lam_min; P.lam_max = B.p.lam_max;
            P.abs_tol = B.p.abs_tol; P.rel_tol = B.p.rel_tol;
            lam = B.lambda[c];
            acc = chn::lm_decide(A.cost[c], nw, P, lam, ph);
            rule = 1;
        } else {
            rule = 2;
        }
    }
    const int copy = __shfl(acc, lane & 48);
    if (copy) {                                        // cs.n > 0 and the chain is not bad (a bad chain's cost is NaN: never accepted)
        const long long np = (long long)cs.n * 8;               // 16-byte pieces: past 2^31 for a chain of 2^28 states
        const double *src = B.trial + cs.f * 16;
        double *dst = B.states + cs.f * 16;
        for (long long i0 = q; i0 < np; i0 += 128) {
            cpi_d2v v[8];
#pragma unroll
            for (int r = 0; r < 8; r++) v[r] = *reinterpret_cast<const cpi_d2v *>(src + 2 * min(i0 + 16 * r, np - 1ll));
#pragma unroll
            for (int r = 0; r < 8; r++)
                if (i0 + 16 * r < np) *reinterpret_cast<cpi_d2v *>(dst + 2 * (i0 + 16 * r)) = v[r];
        }
        if (B.chi2)
            for (int k = q; k < cs.n - 1; k += 16) B.chi2[cs.ff + k] = A.chi2[cs.ff + k];
    }
    if (!mine) return;
    if (B.accepted) B.accepted[c] = acc;
    if (rule == 1) {
        if (acc) A.cost[c] = nw;
        B.lambda[c] = lam;                             // the bits it had where the rule leaves it alone
        if (ph) B.phase[c] = ph;
    } else if (rule == 2) {
        B.phase[c] = 1;
    }
}

}  // namespace
