// cpi_marginalize_kernels.hpp -- cpi_marginalize_kernel: the leading states of every chain of IMU factors eliminated into the
// prior row of the first state that stays (cpi_chain_marginalize_batch; the arithmetic: cpi_math.hpp, chn::marginalize_chain, whose
// lane-mapped form this is).  Part of the translation unit cpi_marginalize.hip (included there after cpi_math.hpp /
// cpi_device_util.hpp / cpi_factor_kernels.hpp, and after cpi_chain_util.hpp, which holds what one elimination step shares with
// cpi_chain_solve_kernel: chain_range, the staged pieces, chain_pick, chain_pivot_step, chain_w, chain_schur; not a stand-alone header).
//
// The mapping of cpi_chain_solve_kernel (cpi_chain_kernels.hpp): 16 lanes (one DPP row) per chain, 4 chains per wavefront, one
// wavefront per workgroup.  Lane j < 15 keeps the FULL symmetric column j of the working block, lane 15 the right-hand side as a
// sixteenth column; pivots, W = L^-1 U and the Schur update are the solve's DPP patterns (cpi_chain_util.hpp), without damping.  LDS
// stages the four hess rows of a trip (4 x 496 doubles, whole 16-byte pieces).  Nothing is written but out and status: no workspace,
// no fence, no back pass.
//
// What differs from the solve is where a chain stops.  The trip count of a wavefront is its largest m; a chain with a smaller m
// FREEZES its carried block from its trip m on (a select per register) and goes on executing on valid addresses -- a DPP source must
// be an active lane.  In those trips it re-reads its last eliminated hess row (row 0 of hess if it eliminates nothing) and the prior
// row of state m, and every value fetched is discarded by a select, never multiplied by zero: rows of hess at factor index >= m and
// rows of prior at states > m are not fetched at all.  After the last trip every chain adds the prior row of its state m and lane
// j <= 14 stores rows i <= j of its column, lane 15 eta and the zero of entry 135.  A chain with m = 0 never enters a trip as an
// active chain: its row is (0 + 0) + Pr_0.  A chain that is refused (m outside [0, n), factor rows outside hess) or whose
// eliminated block failed stores NaN.
#pragma once

namespace {

__global__ __launch_bounds__(64, 2) void cpi_marginalize_kernel(MarginalizeArgs A) {
    constexpr int HD = chn::HESS_D, PD = chn::PRIOR_D, NP = HD / 2, NR = (NP + 63) / 64;   // 248 pieces of 16 bytes per row, 4 per lane
    __shared__ __attribute__((aligned(16))) double sH[4 * HD];
    static_assert(chain_reads_stay_in_rows(), "a read at a constant offset from a lane's base stays inside the row");
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4, jc = min(j, 14);
    const long long c = (long long)blockIdx.x * 4 + fl;
    const ChainRange cs = chain_range(A, c);           // the states and the factors: the solve's rule, over the whole chain
    const int n = cs.n;
    const long long ff = cs.ff;
    const int mraw = A.drop ? A.drop[cs.cc] : A.M;
    const bool ok = c < A.C && !cs.bad && mraw >= 0 && mraw < n;               // n = 0: no m is inside [0, n)
    const int m = ok ? mraw : 0;
    const int mmax = wave_max(m);
    const double qnan = __builtin_nan("");
    // A trip is entered only when a chain of this wavefront eliminates a state: that chain has two states and a factor row inside hess,
    // so S > 0 and F > 0 in every trip, and row 0 of hess and of prior exist for the groups that have no rows of their own.
    const long long f = ok ? cs.f : 0;
    const int cj = (j < 15) ? j : 30, bj = (j < 15) ? 15 + j : 30;
    const double *Hq = sH + fl * HD;

    double nxt[15];
    int st = 0;
#pragma unroll
    for (int i = 0; i < 15; i++) nxt[i] = 0.0;
    for (int s = 0; s < mmax; s++) {
        const bool act = s < m;                        // m <= n - 1: factor s exists wherever act holds
        // the hess rows of this trip, all four chains: every lane loads for every chain; a frozen chain re-reads a row it has read
        {
            const long long row = (m > 0) ? ff + min(s, m - 1) : 0;    // m = 0: ff may be anything (a chain of one state)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const chain_d2u *src = reinterpret_cast<const chain_d2u *>(A.hess + readlane64(row, 16 * q) * HD);
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const int i = min(lane + 64 * r, NP - 1);
                    const chain_d2u v = src[i];
                    sH[q * HD + 2 * i] = v.a; sH[q * HD + 2 * i + 1] = v.b;
                }
            }
        }
        wave_lds_fence();
        double a[15];
        if (A.prior) {
            const double *Pr = A.prior + (f + min(s, m)) * PD;
            const double *colp = Pr + chn::tri(j), *rowp = Pr + j;
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = chain_pick(i <= j, colp[i], rowp[chn::tri(i)]);
        } else {
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = 0.0;
        }
        chain_read_fence();                            // one group of reads at a time
        double u[15], nb[15];
        {
            const double *colp = Hq + chn::tri(cj), *rowp = Hq + cj;
#pragma unroll
            for (int i = 0; i < 15; i++) {
                double cur = chain_pick(i <= cj, colp[i], rowp[chn::tri(i)]);
                cur = act ? cur : 0.0;
                a[i] = (nxt[i] + cur) + a[i];
            }
            chain_read_fence();
            // U = rows 0 .. 14 of packed column 15 + j; the carried block of the next state: rows 15 .. 29 of column 15 + j (30: g)
            const double *ucol = Hq + chn::tri(15 + jc);
            const double *bcol = Hq + chn::tri(bj) + 15, *brow = Hq + bj;
#pragma unroll
            for (int i = 0; i < 15; i++) {
                const double uu = ucol[i];
                u[i] = act ? uu : 0.0;
            }
            chain_read_fence();
#pragma unroll
            for (int i = 0; i < 15; i++) {
                const double bb = chain_pick(15 + i <= bj, bcol[i], brow[chn::tri(15 + i)]);
                nb[i] = act ? bb : 0.0;
            }
        }
        wave_lds_fence();                              // the stage is read: the next trip may write over it
        bool fail = false;
        chain_pivot_step<0>(a, j, fail);
        {
            const unsigned long long bal = __ballot(fail && j < 15);
            if (act && st == 0 && ((bal >> (16 * fl)) & 0xffffull)) st = s + 1;
        }
        chain_w(a, u);
        // lane 15: its w becomes y, and the Schur update carries the right-hand side along
#pragma unroll
        for (int k = 0; k < 15; k++) u[k] = (j == 15) ? a[k] : u[k];
        chain_settle(u);
        __builtin_amdgcn_sched_barrier(0);
        chain_schur(nb, u);
        // a chain past its m keeps the block it carried at its trip m
#pragma unroll
        for (int i = 0; i < 15; i++) nxt[i] = act ? nb[i] : nxt[i];
    }
    if (c >= A.C) return;                              // no DPP from here on
    const bool good = ok && st == 0;
    double pr[15];
#pragma unroll
    for (int i = 0; i < 15; i++) pr[i] = 0.0;
    if (good && A.prior) {
        const double *colp = A.prior + (cs.f + m) * PD + chn::tri(j);       // rows i <= j of column j (j = 15: eta) are contiguous
#pragma unroll
        for (int i = 0; i < 15; i++)
            if (i <= j) pr[i] = colp[i];
    }
    double *o = A.out + c * PD + chn::tri(j);
#pragma unroll
    for (int i = 0; i < 15; i++)
        if (i <= j) o[i] = good ? (nxt[i] + 0.0) + pr[i] : qnan;
    if (j == 15) o[15] = good ? 0.0 : qnan;
    if (A.status && j == 0) A.status[c] = ok ? st : -1;
}

}  // namespace
