// cpi_chain_util.hpp -- what the kernels that walk chains of states share: cpi_chain_solve_kernel (cpi_chain_kernels.hpp) and
// cpi_marginals_kernel (cpi_marginals_kernels.hpp).  The compile-time loop over a DPP control, the wait states in front of a DPP
// read, and the ONE statement of how first / count are clamped into the state rows (include/cpi_amd.h: cpi_chain_solve_batch).
// Included after cpi_args.hpp / cpi_device_util.hpp inside a kernel translation unit; no kernel is defined here.
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

}  // namespace
