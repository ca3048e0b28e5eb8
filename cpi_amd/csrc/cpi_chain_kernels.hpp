// cpi_chain_kernels.hpp -- cpi_chain_solve_kernel: the damped block-tridiagonal solve of chains of IMU factors (cpi_chain_solve_batch;
// the arithmetic and the workspace record: cpi_math.hpp, namespace chn, whose lane-mapped form this is).
// Part of the translation unit cpi_chain.hip (included there after cpi_math.hpp / cpi_device_util.hpp / cpi_factor_kernels.hpp, from
// which it takes dpp_fnmac, and after cpi_chain_util.hpp, which holds what one elimination step shares with cpi_marginalize_kernel:
// chain_range, the staged pieces, chain_pick, chain_pivot_step, chain_w, chain_schur; not a stand-alone header).
//
// 16 lanes (one DPP row) per chain, 4 chains per wavefront, one wavefront per workgroup.  Lane j < 15 keeps column j of the working
// block in registers -- the FULL symmetric column, so the multiplier of its own trailing update is a static register --, lane 15
// the right-hand side as a sixteenth column.  Everything a lane needs of another lane's column is the broadcast operand of a
// double-precision DPP multiply-add:
//   pivots   step k: lane k runs pivot_rsqrt on its a[k], the result is broadcast; a[i] += bcast_k(a[i]) * ca, i > k
//   W        column c of L^-1 U in lane c: L[i][k] = R[k][i] is register a[k] of lane i
//   Schur    nxt[i] -= bcast_i(w[k]) * w[k]: lambda_row_dpp's pattern with a full matrix; lane 15's w holds y
//   back     lane k owns row k: t -= bcast_c(delta_next) * W[k][c], then t -= bcast_m(x) * R[k][m], m = 14 .. 0
// No LDS and no shuffle in the arithmetic.  LDS stages the four hess rows of a step (4 x 496 doubles, whole 16-byte pieces, every
// lane of the wavefront loading for every chain) when the step begins: a single buffer, 15.5 KB.  The kernel fits 253 registers
// without scratch, so two wavefronts per SIMD hide each other's fetches (resource_usage_chain.txt).  Requesting the rows one step
// ahead into registers was measured and is not here: 64 more registers mean one wavefront per SIMD, for the same time within 1.6 %
// (profiles/chain_solve.md).  The forward pass leaves [R y] and W of every state in the caller's workspace, the same wavefront reads
// them back in reverse.
// The arithmetic is namespace chn of cpi_math.hpp term by term and in its order; the bits are not the host's: a pivot's reciprocal
// square root is the Newton sequence of pivot_rsqrt here and 1 / sqrt there, and both are gated against the longdouble reference.
// Lanes of a chain that has ended -- or does not exist, or is refused -- keep executing on valid addresses with their stores
// predicated off: a DPP source must be an active lane, so no 16-lane group leaves early; the trip count of a wavefront is the
// longest of its four chains.  One long chain therefore runs on 16 lanes: there is no parallelism ALONG a chain here.
#pragma once

namespace {

// compile-time loops over a DPP control: chain_for (ascending) is cpi_chain_util.hpp's
template <int I, class F>
__device__ __forceinline__ void chain_for_down(F &&f) {
    if constexpr (I >= 0) { f(std::integral_constant<int, I>()); chain_for_down<I - 1>(f); }
}

__global__ __launch_bounds__(64, 2) void cpi_chain_solve_kernel(ChainArgs A) {
    constexpr int HD = chn::HESS_D, NP = HD / 2, NR = (NP + 63) / 64;   // 248 pieces of 16 bytes per row, 4 per lane
    __shared__ __attribute__((aligned(16))) double sH[4 * HD];
    static_assert(chain_reads_stay_in_rows(), "a read at a constant offset from a lane's base stays inside the row");
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4, jc = min(j, 14);
    const long long c = (long long)blockIdx.x * 4 + fl;
    const ChainRange cr = chain_range(A, c);
    const int n = cr.n;
    const int nmax = wave_max(n);
    const double lam = (A.lambda && c < A.C) ? A.lambda[c] : 0.0;
    const double qnan = __builtin_nan("");
    if (nmax == 0) {                                   // the whole wavefront: nothing to solve
        if (A.status && j == 0 && c < A.C) A.status[c] = 0;
        return;
    }
    // rows this lane's group uses while it has none of its own: state 0 / factor 0 exist (nmax > 0; F > 0 is checked where hess is read)
    const long long f = (n > 0) ? cr.f : 0;
    const long long Fm1 = A.F - 1;
    const int cj = (j < 15) ? j : 30, bj = (j < 15) ? 15 + j : 30;
    const double *Hq = sH + fl * HD;

    double pfa[4 * NR], pfb[4 * NR];
    // The hess rows of step s, all four chains, into registers: every lane loads for every chain.  A chain without a factor at this step
    // re-reads row 0 (F > 0 here; the L2 has it) rather than skipping: a conditional load would keep the sixteen pieces of the
    // PREVIOUS step alive through the whole trip, 64 registers the factorisation does not have.
    auto fetch = [&](int s) {
        const bool hasf = !cr.bad && s < n - 1;
        long long row = cr.ff + s;
        row = (row < 0 || !hasf) ? 0 : ((row > Fm1) ? Fm1 : row);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const chain_d2u *src = reinterpret_cast<const chain_d2u *>(A.hess + readlane64(row, 16 * q) * HD);
#pragma unroll
            for (int r = 0; r < NR; r++) {
                chain_d2u v; v.a = 0.0; v.b = 0.0;
                if (A.F > 0) v = src[min(lane + 64 * r, NP - 1)];
                pfa[q * NR + r] = v.a; pfb[q * NR + r] = v.b;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int i = min(lane + 64 * r, NP - 1);
                sH[q * HD + 2 * i] = pfa[q * NR + r]; sH[q * HD + 2 * i + 1] = pfb[q * NR + r];
            }
    };

    double nxt[15], rawd = 0.0;
    int st = 0;
#pragma unroll
    for (int i = 0; i < 15; i++) nxt[i] = 0.0;
    // ================================================================ forward
    for (int s = 0; s < nmax; s++) {
        const bool act = s < n, hasf = act && !cr.bad && s < n - 1 && A.F > 0;
        const long long srow = f + ((n > 0) ? min(s, n - 1) : 0);
        fetch(s);
        stage();
        wave_lds_fence();
        double a[15], pd = 0.0;
        if (A.prior) {
            const double *Pr = A.prior + srow * chn::PRIOR_D;
            const double *colp = Pr + chn::tri(j), *rowp = Pr + j;
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = chain_pick(i <= j, colp[i], rowp[chn::tri(i)]);
            pd = Pr[chn::tri(jc) + jc];
        } else {
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = 0.0;
        }
        chain_read_fence();                            // one group of reads at a time: all of them at once is 150 doubles in flight
        double u[15];
        {
            const double *colp = Hq + chn::tri(cj), *rowp = Hq + cj;
            double curd = Hq[chn::tri(jc) + jc];
            curd = hasf ? curd : 0.0;
#pragma unroll
            for (int i = 0; i < 15; i++) {
                double cur = chain_pick(i <= cj, colp[i], rowp[chn::tri(i)]);
                cur = hasf ? cur : 0.0;
                a[i] = (nxt[i] + cur) + a[i];
            }
            chain_read_fence();
            // damping: the diagonal of the three sums without the Schur term
            const double d = (rawd + curd) + pd;
#pragma unroll
            for (int i = 0; i < 15; i++) {
                const double damped = A.diagonal ? fma(lam, d, a[i]) : a[i] + lam;
                a[i] = (i == j) ? damped : a[i];
            }
            chain_read_fence();
            // U = rows 0 .. 14 of packed column 15 + j; the carried block of the next state: rows 15 .. 29 of column 15 + j (30: g)
            const double *ucol = Hq + chn::tri(15 + jc);
            const double *bcol = Hq + chn::tri(bj) + 15, *brow = Hq + bj;
#pragma unroll
            for (int i = 0; i < 15; i++) {
                const double uu = ucol[i];
                u[i] = hasf ? uu : 0.0;
            }
            chain_read_fence();
#pragma unroll
            for (int i = 0; i < 15; i++) {
                const double bb = chain_pick(15 + i <= bj, bcol[i], brow[chn::tri(15 + i)]);
                nxt[i] = hasf ? bb : 0.0;
            }
            const double rd = Hq[chn::tri(15 + jc) + 15 + jc];
            rawd = hasf ? rd : 0.0;
        }
        wave_lds_fence();                              // the stage is read: the next trip may write over it
        bool fail = false;
        chain_pivot_step<0>(a, j, fail);
        {
            const unsigned long long bal = __ballot(fail && j < 15);
            if (act && st == 0 && ((bal >> (16 * fl)) & 0xffffull)) st = s + 1;
        }
        chain_w(a, u);
        double *rec = A.workspace + srow * chn::WS_D;
        if (act) {
#pragma unroll
            for (int k = 0; k < 15; k++)
                if (j >= k) rec[chn::row_off(k) + j - k] = a[k];
            if (hasf && j < 15) {
#pragma unroll
                for (int k = 0; k < 15; k++) rec[chn::WS_R + k * 15 + j] = u[k];
            }
        }
        // lane 15: its w becomes y, and the Schur update carries the right-hand side along
#pragma unroll
        for (int k = 0; k < 15; k++) u[k] = (j == 15) ? a[k] : u[k];
        chain_settle(u);
        __builtin_amdgcn_sched_barrier(0);
        chain_schur(nxt, u);
    }
    // the records are read back by OTHER lanes of this wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // ================================================================ back: lane k owns row k (lane 15 redoes row 14)
    const bool poison = cr.bad || st != 0;
    double dn = 0.0;
    for (int s = nmax - 1; s >= 0; s--) {
        const bool act = s < n, hasw = act && !cr.bad && s < n - 1 && A.F > 0;
        const long long srow = f + ((n > 0) ? min(s, n - 1) : 0);
        const double *rec = A.workspace + srow * chn::WS_D;
        // row jc of [R y] starts at column jc: rrow[m] is R[jc][m] for m >= jc and, below that, an entry of an earlier row that no
        // product of this lane's result takes (row_off(k) >= k: still inside the record)
        const double *rrow = rec + (chn::row_off(jc) - jc), *wr = rec + chn::WS_R + jc * 15;
        double rr[15], wrow[15];
#pragma unroll
        for (int m = 0; m < 15; m++) { rr[m] = rrow[m]; wrow[m] = wr[m]; }
        const double inv = rec[chn::row_off(jc)], y = rrow[15];
        double t = y, tw = y;
        chain_settle(dn);
        chain_for<0, 15>([&](auto Cc) {
            constexpr int Cn = decltype(Cc)::value;
            dpp_fnmac<Cn>(tw, dn, wrow[Cn]);
        });
        t = hasw ? tw : t;
        double x = 0.0;
        chain_for_down<14>([&](auto Mc) {
            constexpr int M = decltype(Mc)::value;
            double xc = t * inv;
            x = (j == M) ? xc : x;
            chain_settle(xc);
            dpp_fnmac<M>(t, xc, rr[M]);
            __builtin_amdgcn_sched_barrier(0);
        });
        dn = act ? x : dn;
        if (act && j < 15) A.delta[srow * 15 + j] = poison ? qnan : x;
    }
    if (A.status && j == 0 && c < A.C) A.status[c] = cr.bad ? -1 : st;
}

}  // namespace
