// cpi_fix_kernels.hpp -- cpi_fix_kernel<kind> (cpi_state_fix_batch): absolute measurements of states added to their rows and to their
// cost.  The arithmetic: cpi_math.hpp, chn::Fix / fix_residual / fix_vectors / fix_term (chn::state_fix is the same statement one
// state at a time).  Part of the translation unit cpi_fix.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a
// stand-alone header).
#pragma once

namespace {

// a 16-byte piece of a row on its way through a lane (the rows are 8-byte aligned)
struct __attribute__((packed, aligned(8))) fix_d2u { double a, b; };

// ============================================================================================
// cpi_fix_kernel<K>: the mapping of the chain family -- SIXTEEN lanes per state, four states per wavefront, one wavefront per workgroup.
//   ranges    every lane of a state reads mfirst[s], mfirst[s + 1] and clamps them into [0, M] (m1 >= m0): a broken mfirst reads
//             other fixes, never outside z / R / weight / chi2
//   fetch     with rows (out != NULL): the 68 sixteen-byte pieces of the base row, lane j pieces j, j + 16, ...: five loads per lane,
//             all requested before the first LDS write; zeros where base is NULL.  Without rows nothing of base or out is touched.
//   LDS       state-major [136] at pitch 137 (odd): 4384 bytes per wavefront.  The flush reads 8 bytes at dword 274 fl + 4 j + 64 r:
//             within a group of 32 lanes (two states) the banks 4 j, 4 j + 1 and 4 j + 18, 4 j + 19 are all distinct, where the even
//             pitch 136 would put state 1 on the banks of state 0 (272 mod 64 = 16).
//   entries   a kind touches NT = d (d + 1) / 2 + d entries of the row (9, or 27 for the pose); lane j owns t = j and t = j + 16 and
//             keeps them in two registers from the base value to the last fix (lanes past NT redo the last entry and store nothing)
//   fixes     m ascending.  Every lane of the state loads z_m and R_m (one address for sixteen lanes: a broadcast), and computes e,
//             wh, chi2 and u in registers -- at most a 6 x 6 triangle, cheaper than an exchange; its own entries G_ab come from
//             chn::fix_term, which reads R_m at the lane's (a, b) from memory (the line is in the L1 after the broadcast load):
//             no register array is indexed at run time, so nothing spills to scratch
//   stores    the two entries go back to the staged row, entry 135 becomes 0.0, and the row leaves as 68 contiguous 16-byte
//             non-temporal stores; pcost is one double per state and chi2 one per fix, from lane 0 of the state
// A state's bits depend on its own data only.  The kernel is bound by its row traffic: 1088 bytes in and 1088 out per state against
// 128 of state and 80 (position) to 232 (pose) per fix; the cost-only call moves none of the rows.
// ============================================================================================
constexpr int FIX_NP = chn::PRIOR_D / 2, FIX_NR = (FIX_NP + 15) / 16, FIX_PITCH = chn::PRIOR_D + 1;

template <int K>
__global__ __launch_bounds__(64) void cpi_fix_kernel(FixArgs A) {
    typedef chn::Fix<K> T;
    __shared__ double sRow[4 * FIX_PITCH];
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4;
    const long long s = (long long)blockIdx.x * 4 + fl;
    const bool live = s < A.S, rows = A.out != nullptr;
    long long m0 = 0, m1 = 0;
    if (live) {
        m0 = min(max(A.mfirst[s], 0ll), A.M);
        m1 = max(min(max(A.mfirst[s + 1], 0ll), A.M), m0);
    }
    double *row = sRow + fl * FIX_PITCH;
    const int t0 = min(j, T::NT - 1), t1 = min(j + 16, T::NT - 1);
    const int slot0 = T::slot(t0), slot1 = T::slot(t1);
    double acc0 = 0.0, acc1 = 0.0;
    if (rows) {
        fix_d2u pr[FIX_NR];
#pragma unroll
        for (int r = 0; r < FIX_NR; r++) { pr[r].a = 0.0; pr[r].b = 0.0; }
        if (live && A.base) {
#pragma unroll
            for (int r = 0; r < FIX_NR; r++)
                pr[r] = *reinterpret_cast<const fix_d2u *>(A.base + s * chn::PRIOR_D + 2 * min(j + 16 * r, FIX_NP - 1));
        }
#pragma unroll
        for (int r = 0; r < FIX_NR; r++) {
            const int i = min(j + 16 * r, FIX_NP - 1);         // the lanes past piece 67 write piece 67 again: the same values
            row[2 * i] = pr[r].a; row[2 * i + 1] = pr[r].b;
        }
        wave_lds_fence();
        acc0 = row[slot0]; acc1 = row[slot1];
    }
    double pc = (live && A.pcost_base) ? A.pcost_base[s] : 0.0;
    if (m1 > m0) {
        const double *xs = A.states + s * 16;
        NavState x;
        x.q = ldq4(xs); x.bg = mk(0.0, 0.0, 0.0); x.v = ldv3(xs + 7); x.ba = x.bg; x.p = ldv3(xs + 13);
        for (long long m = m0; m < m1; m++) {
            const double *zp = A.z + m * T::ZN, *Rm = A.R + m * T::RN;
            double z[T::ZN], R[T::RN], e[T::D], wh[T::D], u[T::D];
#pragma unroll
            for (int i = 0; i < T::ZN; i++) z[i] = zp[i];
#pragma unroll
            for (int i = 0; i < T::RN; i++) R[i] = Rm[i];
            const double w = A.weight ? A.weight[m] : 1.0;
            chn::fix_residual<K>(x, z, e);
            const double c2 = chn::fix_vectors<T::D>(R, e, wh, u);
            pc = fma(0.5 * w, c2, pc);
            if (A.chi2 && j == 0) A.chi2[m] = c2;
            if (rows) {
                acc0 = fma(w, chn::fix_term<T::D>(Rm, u, t0), acc0);
                if (T::NT > 16) acc1 = fma(w, chn::fix_term<T::D>(Rm, u, t1), acc1);
            }
        }
    }
    if (live && A.pcost && j == 0) A.pcost[s] = pc;
    if (!rows) return;
    if (j < T::NT) row[slot0] = acc0;
    if (j + 16 < T::NT) row[slot1] = acc1;
    if (j == 15) row[chn::PRIOR_D - 1] = 0.0;
    wave_lds_fence();
    if (!live) return;
    double *dst = A.out + s * chn::PRIOR_D;
#pragma unroll
    for (int r = 0; r < FIX_NR; r++) {
        const int k = j + 16 * r;
        if (k < FIX_NP) st16_nt(dst + 2 * k, row[2 * k], row[2 * k + 1]);
    }
}

}  // namespace
