// cpi_chain_util.hpp -- what the kernels that walk chains of states share: cpi_chain_solve_kernel (cpi_chain_kernels.hpp),
// cpi_marginals_kernel (cpi_marginals_kernels.hpp) and cpi_marginalize_kernel (cpi_marginalize_kernels.hpp).  For all three: the
// compile-time loop over a DPP control, the wait states in front of a DPP read, and the ONE statement of how first / count are clamped
// into the state rows (include/cpi_amd.h: cpi_chain_solve_batch).  For the two that eliminate states along a chain (the solve and the
// marginalize): the factor range of a chain, the staged 16-byte pieces, the both-candidates read of a packed symmetric entry, and the
// three DPP patterns of one elimination -- the pivot steps, W = L^-1 U and the Schur update.
// Included after cpi_args.hpp / cpi_device_util.hpp / cpi_factor_kernels.hpp (row_share, dpp_fmac / dpp_fnmac / dpp_mul, pivot_rsqrt)
// inside a kernel translation unit; no kernel is defined here.
#pragma once

namespace {

// compile-time loops over a DPP control (the broadcast lane is an immediate)
template <int I, int N, class F>
__device__ __forceinline__ void chain_for(F &&f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>()); chain_for<I + 1, N>(f); }
}
// a VALU result that is read as a DPP source next: two wait states, tied to the register so that nothing moves across
__device__ __forceinline__ void chain_settle(double &v) { asm volatile("s_nop 1" : "+v"(v)); }
__device__ __forceinline__ void chain_settle(double (&v)[15]) {
    asm volatile("s_nop 1" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                             "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]));
}

// The states of chain c: first clamped into [0, S], count into [0, G] and into what is left of S; a chain past C has none.  cc is
// the index the per-chain arrays are read at (c clamped into [0, C)).
struct ChainStates { long long f, cc; int n; };
__device__ __forceinline__ ChainStates chain_states(long long C, int G, long long S, const long long *first, const int *count, long long c) {
    ChainStates r;
    const long long cc = (c < C) ? c : C - 1;
    long long f = first ? first[cc] : cc * (long long)G;
    int n = count ? count[cc] : G;
    n = (n < 0) ? 0 : ((n > G) ? G : n);
    f = (f < 0) ? 0 : ((f > S) ? S : f);
    if (S - f < (long long)n) n = (int)(S - f);
    if (c >= C) n = 0;
    r.f = f; r.n = n; r.cc = cc;
    return r;
}

// The factors of chain c (ChainArgs / MarginalizeArgs: ffirst, F): ff is the row of hess that joins states 0 and 1 of the chain.  A
// chain of more than one state whose n - 1 factor rows do not lie inside [0, F) is refused (bad).
struct ChainRange { long long f, ff, cc; int n; bool bad; };
template <class Args>
__device__ __forceinline__ ChainRange chain_range(const Args &A, long long c) {
    ChainRange r;
    const ChainStates cs = chain_states(A.C, A.G, A.S, A.first, A.count, c);
    r.f = cs.f; r.n = cs.n; r.cc = cs.cc;
    r.ff = A.ffirst ? A.ffirst[cs.cc] : cs.f - cs.cc;
    r.bad = cs.n > 1 && (r.ff < 0 || r.ff > A.F - (long long)(cs.n - 1));
    return r;
}

// a 16-byte piece of a hess row on its way into the LDS stage (the rows are 8-byte aligned)
struct __attribute__((packed, aligned(8))) chain_d2u { double a, b; };

__device__ __forceinline__ long long readlane64(long long v, int l) {
    return ((long long)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), l);
}
// Entry (i, d) of a packed symmetric matrix sits at T(d) + i or at T(i) + d.  BOTH are read -- each a lane's base plus a constant the
// instruction carries -- and one is kept: an address per entry, picked first, is a register per entry that the compiler computes
// once and holds through the whole chain (75 of them).  The one not kept lies inside the same row: every kernel that picks asserts
// chain_reads_stay_in_rows().
__device__ __forceinline__ double chain_pick(bool first, double x, double y) { return first ? x : y; }
// the furthest entries chain_pick and the column reads touch, kept or not, lie inside a hess row / a prior row
constexpr bool chain_reads_stay_in_rows() {
    return chn::tri(30) + 29 < chn::HESS_D && 30 + chn::tri(29) < chn::HESS_D && chn::tri(15) + 14 < chn::PRIOR_D && 15 + chn::tri(14) < chn::PRIOR_D;
}
// keeps the reads of one group from being issued with the next group's (instruction selection orders memory operations along it)
__device__ __forceinline__ void chain_read_fence() { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }

// pivot step K of the augmented block (chn::factor_block); a[K] becomes R[K][j] (1 / R[K][K] in lane K)
// No "finished lane" select in the trailing update: lanes j <= K go on updating rows of columns that are never read again (the
// broadcasts of the later steps come from lanes > K, and a lane's a[k], k <= K, is already final), as in cpi_sqrt_info_kernel.
template <int K>
__device__ __forceinline__ void chain_pivot_step(double (&a)[15], int j, bool &fail) {
    if constexpr (K < 15) {
        double mine = a[K];
        if (j == K) {
            if (!(mine > 0.0)) fail = true;
            mine = pivot_rsqrt(mine);
        }
        chain_settle(mine);
        const double inv = row_share<K>(mine);
        const double r = a[K] * inv, ca = -inv * r;
        a[K] = (j == K) ? inv : r;
#pragma unroll
        for (int i = K + 1; i < 15; i++) dpp_fmac<K>(a[i], a[i], ca);   // rows ascend: a[K + 1], the next pivot, is the oldest write
        asm volatile("s_nop 1");
        __builtin_amdgcn_sched_barrier(0);
        chain_pivot_step<K + 1>(a, j, fail);
    }
}

// W = L^-1 U: column min(j, 14) in this lane (lane 15 redoes column 14); L[i][k] = R[k][i] is register a[k] of lane i
__device__ __forceinline__ void chain_w(const double (&a)[15], double (&u)[15]) {
    chain_for<0, 15>([&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        u[K] = dpp_mul<K>(a[K], u[K]);
        chain_for<K + 1, 15>([&](auto Ic) {
            constexpr int I = decltype(Ic)::value;
            dpp_fnmac<I>(u[I], a[K], u[K]);
        });
    });
    __builtin_amdgcn_sched_barrier(0);
}

// The Schur update of the carried block: nb[i] -= bcast_i(w[k]) * w[k].  Lane 15's w holds y, so the right-hand side is carried
// along; w has settled (chain_settle) when this is called.
__device__ __forceinline__ void chain_schur(double (&nb)[15], const double (&w)[15]) {
    chain_for<0, 15>([&](auto Ic) {
        constexpr int I = decltype(Ic)::value;
        chain_for<0, 15>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
            dpp_fnmac<I>(nb[I], w[K], w[K]);
        });
    });
    __builtin_amdgcn_sched_barrier(0);
}

}  // namespace
