// cpi_condense_kernels.hpp -- cpi_condense_kernel and cpi_expand_kernel: chains of IMU factors cut into segments of K factors, the
// states between the two ends of every segment eliminated (cpi_chain_condense_batch), and the solution of the short chain of segment
// ends substituted back into them (cpi_chain_expand_batch).  The arithmetic and the workspace record: cpi_math.hpp, namespace chn
// (condense_segment, condense_separator, expand_segment), whose lane-mapped forms these are.  Part of the translation unit
// cpi_condense.hip (included there after cpi_math.hpp / cpi_device_util.hpp / cpi_factor_kernels.hpp, and after cpi_chain_util.hpp,
// which holds what one elimination step shares with cpi_chain_solve_kernel and cpi_marginalize_kernel; not a stand-alone header).
//
// 16 lanes (one DPP row) per SEGMENT, 4 segments per wavefront, one wavefront per workgroup: group q = 4 blockIdx + lane / 16 is
// segment q % P of chain q / P, P = max(Gr - 1, 1) the segment slots of a chain.  A chain of 549 states at K = 23 is 24 groups of 22
// trips, where cpi_chain_solve_kernel walks 549 states on 16 lanes: this is the parallelism ALONG a chain.
//
// Condense.  What a segment carries is the 31 x 31 factor between its left end a and the state t it has reached, in five pieces:
//   aa   M_aa, column j in lane j < 15 and m_a in lane 15 -- in LDS (4 x 15 x 16 doubles, slot [i][lane]: a lane reads and writes its own
//        slots only, no fence): it is only ever accumulated into, once per trip, and 30 registers are what the pivots need
//   v    M_at: lane j < 15 holds ROW j (a-index j), v[k] = M_at[j][k], which is column j of M_at^T -- the second right-hand block
//        that goes through the same L^-1 as U (chain_w); registers
//   nxt  M_tt, column j in lane j < 15 and m_t in lane 15: the solve's carried block; registers
//   c, rawd  the scalar of lane 15, and the raw diagonal of the trailing block for diagonal damping
// A trip eliminates one interior state with the solve's forward step (the staged hess row, chain_pick, chain_pivot_step, chain_w,
// chain_schur) plus chain_w on v, chain_schur on aa and the product M_a,t+1 = -Wa^T Wn (225 DPP multiply-adds each), and leaves
// [R y], Wn and Wa of the state in its workspace record.  Lane 15 carries y through all of them as in the solve.
// The trip count of a wavefront is the largest number of interiors of its four groups.  A group with fewer STORES its row in the trip
// it is done (s == ni) and goes on executing on valid addresses with every later store predicated off -- a DPP source must be an
// active lane --, so nothing has to be frozen: what it computes afterwards is discarded.
// Separators are not factorised: the group of a segment writes the damped prior row of its left end (chn::condense_separator), the
// last segment of a chain also that of the chain's last state, segment slot 0 the row of a chain of one state and rcount.
//
// Expand.  The same mapping; the solve's back-substitution with two broadcast sources, delta_a (fixed) and delta_{t+1}, from the
// segment's right end down to its first interior.  A group copies the reduced solve's row of its left end (the last segment: of both
// ends) into delta.
// Registers, LDS and occupancy: resource_usage_condense.txt (cpi_amd/build.py); no scratch.
#pragma once

namespace {

template <int I, class F>
__device__ __forceinline__ void condense_for_down(F &&f) {
    if constexpr (I >= 0) { f(std::integral_constant<int, I>()); condense_for_down<I - 1>(f); }
}

// Which segment a 16-lane group works on.  n: the chain's clamped states; m: its reduced states; seg: the group has a segment (slot sj
// < m - 1); a0: chain-local index of the left end; ni: interiors of the segment (factors - 1); last: the chain's last segment.
struct CondenseSlot { long long c; int sj, m, a0, ni; bool inq, seg, last; };
__device__ __forceinline__ CondenseSlot condense_slot(long long C, int Gr, int K, int n, long long q) {
    CondenseSlot r;
    const int P = (Gr > 1) ? Gr - 1 : 1;
    r.c = q / P; r.sj = (int)(q - r.c * P);
    r.inq = r.c < C;
    r.m = (n >= 2) ? (n - 2) / K + 2 : n;
    r.seg = r.inq && r.sj < r.m - 1;
    r.last = r.seg && r.sj == r.m - 2;
    r.a0 = r.seg ? r.sj * K : 0;                           // sj < m - 1 <= (n - 2) / K + 1: a0 <= n - 2, no overflow
    const int b0 = r.seg ? ((n - 1 - r.a0 < K) ? n - 1 : r.a0 + K) : 0;
    r.ni = r.seg ? b0 - r.a0 - 1 : 0;
    return r;
}

__global__ __launch_bounds__(64, 2) void cpi_condense_kernel(CondenseArgs A) {
    constexpr int HD = chn::HESS_D, PD = chn::PRIOR_D, NP = HD / 2, NR = (NP + 63) / 64;   // 248 pieces of 16 bytes per row, 4 per lane
    __shared__ __attribute__((aligned(16))) double sH[4 * HD];
    __shared__ double sA[4 * 15 * 16];
    static_assert(chain_reads_stay_in_rows(), "a read at a constant offset from a lane's base stays inside the row");
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4, jc = min(j, 14);
    const long long q = (long long)blockIdx.x * 4 + fl;
    const int P = (A.Gr > 1) ? A.Gr - 1 : 1;
    const ChainRange cr = chain_range(A, q / P);           // a group past the last chain: no states
    const int n = cr.n;
    const CondenseSlot sl = condense_slot(A.C, A.Gr, A.K, n, q);
    const long long c = sl.c;
    const bool work = sl.seg && !cr.bad;                   // n > 1 and the chain's factor rows lie inside [0, F): F > 0
    const int ni = work ? sl.ni : 0;
    const int tmax = wave_max(ni);
    const double lam = (A.lambda && sl.inq) ? A.lambda[cr.cc] : 0.0;
    const double qnan = __builtin_nan("");
    const int cj = (j < 15) ? j : 30, bj = (j < 15) ? 15 + j : 30;
    const double *Hq = sH + fl * HD;
    double *Aq = sA + fl * 240 + j;

    if (sl.inq && j == 0) {
        if (sl.sj == 0) A.rcount[c] = sl.m;
        if (A.status && A.Gr > 1 && !sl.seg) A.status[c * (A.Gr - 1) + sl.sj] = 0;          // a slot without a segment
    }
    // ---------------------------------------------------------------- the separators' prior rows (no DPP: predicated)
    {
        const bool one = sl.inq && sl.sj == 0 && n == 1;   // a chain of one state: its only reduced state
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const bool on = e == 0 ? (sl.seg || one) : sl.last;
            if (on) {
                const int s = e == 0 ? sl.a0 : n - 1;
                const long long srow = cr.f + s;
                double rawd = 0.0, curd = 0.0, pd = 0.0;
                if (!cr.bad && s > 0) rawd = A.hess[(cr.ff + s - 1) * HD + chn::tri(15 + jc) + 15 + jc];
                if (!cr.bad && s < n - 1) curd = A.hess[(cr.ff + s) * HD + chn::tri(jc) + jc];
                if (A.prior) pd = A.prior[srow * PD + chn::tri(jc) + jc];
                const double d = (rawd + curd) + pd;
                const double *colp = A.prior ? A.prior + srow * PD + chn::tri(j) : nullptr;  // rows i <= j of column j (15: eta) are contiguous
                double *o = A.rprior + (c * A.Gr + sl.sj + e) * PD + chn::tri(j);
#pragma unroll
                for (int i = 0; i < 15; i++)
                    if (i <= j) {
                        double x = colp ? colp[i] : 0.0;
                        if (A.lambda && i == j) x = A.diagonal ? fma(lam, d, x) : x + lam;
                        o[i] = x;
                    }
                if (j == 15) o[15] = 0.0;
            }
        }
    }
    // the hess rows of a trip, all four groups: every lane loads for every group.  Entered only when a group of this wavefront has work:
    // F > 0 then, and row 0 exists for the groups that have no row of their own.
    auto stage = [&](long long row) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const chain_d2u *src = reinterpret_cast<const chain_d2u *>(A.hess + readlane64(row, 16 * g) * HD);
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int i = min(lane + 64 * r, NP - 1);
                const chain_d2u v = src[i];
                sH[g * HD + 2 * i] = v.a; sH[g * HD + 2 * i + 1] = v.b;
            }
        }
    };
    if (__ballot(work) == 0ull) {                          // the whole wavefront: no segment to condense
        if (sl.seg) {                                      // a refused chain's segments
            double *rh = A.rhess + (c * (A.Gr - 1) + sl.sj) * HD;
            for (int i = j; i < HD; i += 16) rh[i] = qnan;
            if (A.status && j == 0) A.status[c * (A.Gr - 1) + sl.sj] = -1;
        }
        return;
    }
    // ---------------------------------------------------------------- M = H_a
    const long long frow = work ? cr.ff + sl.a0 : 0;       // the factor row of the left end
    const long long srow0 = work ? cr.f + sl.a0 : 0;       // its state
    stage(frow);
    wave_lds_fence();
    double v[15], nxt[15], cst, rawd;
    {
        const double *colp = Hq + chn::tri(cj), *rowp = Hq + cj;
#pragma unroll
        for (int i = 0; i < 15; i++) Aq[16 * i] = chain_pick(i <= cj, colp[i], rowp[chn::tri(i)]);
#pragma unroll
        for (int k = 0; k < 15; k++) v[k] = Hq[chn::tri(15 + k) + jc];
        const double *bcol = Hq + chn::tri(bj) + 15, *brow = Hq + bj;
#pragma unroll
        for (int i = 0; i < 15; i++) nxt[i] = chain_pick(15 + i <= bj, bcol[i], brow[chn::tri(15 + i)]);
        cst = Hq[chn::tri(30) + 30];
        rawd = Hq[chn::tri(15 + jc) + 15 + jc];
    }
    wave_lds_fence();                                      // the stage is read: the first trip may write over it
    int st = 0;
    for (int s = 0;; s++) {
        if (s == ni && sl.seg) {                           // this group's segment is condensed: its row (no DPP inside)
            const bool good = work && st == 0;
            double *rh = A.rhess + (c * (A.Gr - 1) + sl.sj) * HD;
            if (j < 15) {
#pragma unroll
                for (int i = 0; i < 15; i++)
                    if (i <= j) rh[chn::tri(j) + i] = good ? Aq[16 * i] : qnan;
#pragma unroll
                for (int k = 0; k < 15; k++) rh[chn::tri(15 + k) + j] = good ? v[k] : qnan;
#pragma unroll
                for (int i = 0; i < 15; i++)
                    if (i <= j) rh[chn::tri(15 + j) + 15 + i] = good ? nxt[i] : qnan;
            } else {
#pragma unroll
                for (int i = 0; i < 15; i++) {
                    rh[chn::tri(30) + i] = good ? Aq[16 * i] : qnan;
                    rh[chn::tri(30) + 15 + i] = good ? nxt[i] : qnan;
                }
                rh[chn::tri(30) + 30] = good ? cst : qnan;
            }
            if (A.status && j == 0) A.status[c * (A.Gr - 1) + sl.sj] = work ? st : -1;
        }
        if (s >= tmax) break;
        const bool act = s < ni;
        const int t = (ni > 0) ? min(s, ni - 1) + 1 : 0;   // the interior of this trip, from the left end; a group that is done re-reads
        stage(frow + t);
        wave_lds_fence();
        const long long srow = srow0 + t;
        double a[15], pd = 0.0;
        if (A.prior) {
            const double *Pr = A.prior + srow * PD;
            const double *colp = Pr + chn::tri(j), *rowp = Pr + j;
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = chain_pick(i <= j, colp[i], rowp[chn::tri(i)]);
            pd = Pr[chn::tri(jc) + jc];
        } else {
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = 0.0;
        }
        chain_read_fence();                                // one group of reads at a time
        double u[15];
        {
            const double *colp = Hq + chn::tri(cj), *rowp = Hq + cj;
            const double curd = Hq[chn::tri(jc) + jc];
#pragma unroll
            for (int i = 0; i < 15; i++) a[i] = (nxt[i] + chain_pick(i <= cj, colp[i], rowp[chn::tri(i)])) + a[i];
            chain_read_fence();
            // damping: the diagonal of the three sums without the Schur term, the solve's rule
            const double d = (rawd + curd) + pd;
#pragma unroll
            for (int i = 0; i < 15; i++) {
                const double damped = A.diagonal ? fma(lam, d, a[i]) : a[i] + lam;
                a[i] = (i == j) ? damped : a[i];
            }
            const double *ucol = Hq + chn::tri(15 + jc);
#pragma unroll
            for (int i = 0; i < 15; i++) u[i] = ucol[i];
            chain_read_fence();
        }
        bool fail = false;
        chain_pivot_step<0>(a, j, fail);
        {
            const unsigned long long bal = __ballot(fail && j < 15);
            if (act && st == 0 && ((bal >> (16 * fl)) & 0xffffull)) st = sl.a0 + t + 1;
        }
        chain_settle(a);                                   // the select that ends a pivot step must not sink to the DPP read of chain_w
        chain_w(a, u);                                     // Wn = L^-1 U
        chain_w(a, v);                                     // Wa = L^-1 M_at^T
        if (act) {
            double *rec = A.workspace + srow * chn::CS_D;
#pragma unroll
            for (int k = 0; k < 15; k++)
                if (j >= k) rec[chn::row_off(k) + j - k] = a[k];
            if (j < 15) {
#pragma unroll
                for (int k = 0; k < 15; k++) { rec[chn::WS_R + k * 15 + j] = u[k]; rec[chn::CS_A + k * 15 + j] = v[k]; }
            }
        }
        // lane 15: both of its w become y, and the updates carry the right-hand sides along
        cst = cst + Hq[chn::tri(30) + 30];
#pragma unroll
        for (int k = 0; k < 15; k++) {
            u[k] = (j == 15) ? a[k] : u[k];
            v[k] = (j == 15) ? a[k] : v[k];
            cst = fma(-a[k], a[k], cst);                   // lane 15's a[k] is y_k; the other lanes' cst is never stored
        }
        {
            const double *bcol = Hq + chn::tri(bj) + 15, *brow = Hq + bj;
#pragma unroll
            for (int i = 0; i < 15; i++) nxt[i] = chain_pick(15 + i <= bj, bcol[i], brow[chn::tri(15 + i)]);
            rawd = Hq[chn::tri(15 + jc) + 15 + jc];
        }
        wave_lds_fence();                                  // the stage is read: the next trip may write over it
        chain_settle(u);
        chain_settle(v);
        __builtin_amdgcn_sched_barrier(0);
        chain_schur(nxt, u);                               // M_t+1,t+1 = H_t[15:30, 15:30 | 30] - Wn^T [Wn y]
        // M_aa -= Wa^T [Wa y], five rows at a time through LDS
        chain_for<0, 3>([&](auto Bc) {
            constexpr int I0 = 5 * decltype(Bc)::value;
            double x[5];
#pragma unroll
            for (int i = 0; i < 5; i++) x[i] = Aq[16 * (I0 + i)];
            chain_for<0, 5>([&](auto Ic) {
                constexpr int I = decltype(Ic)::value;
                chain_for<0, 15>([&](auto Kc) {
                    constexpr int Kk = decltype(Kc)::value;
                    dpp_fnmac<I0 + I>(x[I], v[Kk], v[Kk]);
                });
            });
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 5; i++) Aq[16 * (I0 + i)] = x[i];
        });
        // M_a,t+1 = -Wa^T Wn: entry k of row j is -sum over r of bcast_k(Wn[r]) Wa[r] (lane 15: Wn^T y over again, never stored)
        double vn[15];
        chain_for<0, 15>([&](auto Kc) {
            constexpr int Kk = decltype(Kc)::value;
            vn[Kk] = 0.0;
            chain_for<0, 15>([&](auto Rc) {
                constexpr int R = decltype(Rc)::value;
                dpp_fnmac<Kk>(vn[Kk], u[R], v[R]);
            });
        });
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 15; k++) v[k] = vn[k];
    }
}

__global__ __launch_bounds__(64, 2) void cpi_expand_kernel(ExpandArgs A) {
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4, jc = min(j, 14);
    const long long q = (long long)blockIdx.x * 4 + fl;
    const int P = (A.Gr > 1) ? A.Gr - 1 : 1;
    const ChainStates cs = chain_states(A.C, A.G, A.S, A.first, A.count, q / P);
    const int n = cs.n;
    const CondenseSlot sl = condense_slot(A.C, A.Gr, A.K, n, q);
    const int ni = sl.ni;
    const int tmax = wave_max(ni);
    const double *ra = A.rdelta + (sl.c * A.Gr + sl.sj) * 15;
    const bool one = sl.inq && sl.sj == 0 && n == 1;
    double da = 0.0, dn = 0.0;
    if (sl.seg || one) da = ra[jc];
    if (sl.seg) dn = ra[15 + jc];
    if (j < 15) {
        if (sl.seg || one) A.delta[(cs.f + sl.a0) * 15 + j] = da;
        if (sl.last) A.delta[(cs.f + n - 1) * 15 + j] = dn;
    }
    // a trip is entered only when a group of this wavefront has an interior: S > 0 then, and record 0 exists for the groups without one
    const long long srow0 = (ni > 0) ? cs.f + sl.a0 : 0;
    chain_settle(da);
    for (int s = 0; s < tmax; s++) {
        const bool act = s < ni;
        const long long srow = srow0 + ((ni > 0) ? ni - min(s, ni - 1) : 0);     // interiors from the right end down
        const double *rec = A.workspace + srow * chn::CS_D;
        // row jc of [R y] starts at column jc: rrow[m] is R[jc][m] for m >= jc and, below that, an entry of an earlier row that no
        // product of this lane's result takes (row_off(k) >= k: still inside the record)
        const double *rrow = rec + (chn::row_off(jc) - jc), *wn = rec + chn::WS_R + jc * 15, *wa = rec + chn::CS_A + jc * 15;
        double rr[15], wnrow[15], warow[15];
#pragma unroll
        for (int m = 0; m < 15; m++) { rr[m] = rrow[m]; wnrow[m] = wn[m]; warow[m] = wa[m]; }
        const double inv = rec[chn::row_off(jc)];
        double t = rrow[15];
        chain_settle(dn);
        chain_for<0, 15>([&](auto Cc) {
            constexpr int Cn = decltype(Cc)::value;
            dpp_fnmac<Cn>(t, da, warow[Cn]);
        });
        chain_for<0, 15>([&](auto Cc) {
            constexpr int Cn = decltype(Cc)::value;
            dpp_fnmac<Cn>(t, dn, wnrow[Cn]);
        });
        double x = 0.0;
        condense_for_down<14>([&](auto Mc) {
            constexpr int M = decltype(Mc)::value;
            double xc = t * inv;
            x = (j == M) ? xc : x;
            chain_settle(xc);
            dpp_fnmac<M>(t, xc, rr[M]);
            __builtin_amdgcn_sched_barrier(0);
        });
        dn = act ? x : dn;
        if (act && j < 15) A.delta[srow * 15 + j] = x;
    }
}

}  // namespace
