// cpi_between_kernels.hpp -- cpi_between_kernel<kind> (cpi_state_between_batch): measurements between the two states of an IMU factor
// added to the factor's 31 x 31 row and to its chi2.  The arithmetic: cpi_math.hpp, chn::Between / between_geometry / between_residual /
// between_jcol / between_acol / between_term (chn::factor_between is the same statement one factor at a time).  Part of the translation
// unit cpi_between.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

// a 16-byte piece of a row on its way through a lane (the rows are 8-byte aligned)
struct __attribute__((packed, aligned(8))) btw_d2u { double a, b; };

// ============================================================================================
// cpi_between_kernel<K>: the mapping of the chain family -- SIXTEEN lanes per factor, four factors per wavefront, one wavefront per
// workgroup.
//   ranges    every lane of a factor reads mfirst[f], mfirst[f + 1] and clamps them into [0, M] (m1 >= m0); the two state indices are
//             clamped into [0, S): a broken mfirst or index reads other measurements or states, never outside an array
//   entries   a kind touches NT = NC (NC + 1) / 2 entries of the row (28, 55, or 91 for the pose); lane j owns t = j + 16 r,
//             r < NE = 2 | 4 | 6, and keeps them in registers from the base value to the last measurement (the slots past NT redo the
//             last entry and store nothing)
//   rows      OUT OF PLACE (hess != hess_base): the 248 sixteen-byte pieces of the base row, lane j pieces j, j + 16, ...: sixteen
//             loads per lane, all requested before the first LDS write; zeros where hess_base is NULL.  LDS factor-major [496] at pitch
//             497 (odd): the flush reads 8 bytes at dword 994 fl + 4 j + 64 r, so within a group of 32 lanes (two factors) the banks
//             4 j, 4 j + 1 and 4 j + 34, 4 j + 35 are all distinct, where the even pitch 496 would put factor 1 on the banks of factor 0
//             (992 mod 64 = 32).  The entries go back to the staged row and the row leaves as 248 contiguous 16-byte non-temporal stores.
//             IN PLACE (hess == hess_base): no staging -- a lane loads its own NE entries of a factor that has measurements, and
//             stores them; a factor without measurements is not touched.  The same kernel body: the branch is uniform over the launch.
//             Without rows (hess NULL) nothing of hess_base or hess is touched.
//   columns   J depends on the two states alone: lane j < NC - 1 builds column j of it once per factor (chn::between_jcol, selects on
//             registers).  Per measurement, m ascending: every lane of the factor loads z_m and R_m (one address for sixteen lanes: a
//             broadcast) and computes e, wh and chi2 in registers; lane j whitens ITS column (lane NC - 1 holds -wh) and puts its d
//             values into the factor's [d][16] tile of LDS; the lane's entries (a, b) are then the fma chains over the columns a and b
//             read back from the tile.  No register array is indexed at run time, so nothing spills to scratch.
//   cost      chi2[f] is one double per factor and chi2_m one per measurement, from lane 0 of the factor
// A factor's bits depend on its own data only.  Traffic per factor: 3968 bytes in and 3968 out out of place; in place the 8 NT bytes
// of the touched entries each way, for factors with measurements only; 256 of the two states and 80 (position) to 232 (pose) per
// measurement in every form.
// ============================================================================================
constexpr int BTW_ROW = 496, BTW_NP = BTW_ROW / 2, BTW_NR = (BTW_NP + 15) / 16, BTW_PITCH = BTW_ROW + 1;

template <int K>
__global__ __launch_bounds__(64) void cpi_between_kernel(BetweenArgs A) {
    typedef chn::Between<K> T;
    constexpr int NE = (T::NT + 15) / 16;
    __shared__ double sRow[4 * BTW_PITCH];
    __shared__ double sCol[4 * T::D * 16];
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4;
    const long long f = (long long)blockIdx.x * 4 + fl;
    const bool live = f < A.F, rows = A.hess != nullptr, inplace = rows && A.hess == A.hess_base;
    long long m0 = 0, m1 = 0;
    if (live) {
        m0 = min(max(A.mfirst[f], 0ll), A.M);
        m1 = max(min(max(A.mfirst[f + 1], 0ll), A.M), m0);
    }
    double *row = sRow + fl * BTW_PITCH, *tile = sCol + fl * T::D * 16;
    int slot[NE], ca[NE], cb[NE];
    double acc[NE];
#pragma unroll
    for (int r = 0; r < NE; r++) {
        const int t = min(j + 16 * r, T::NT - 1);
        T::ab(t, ca[r], cb[r]);
        slot[r] = chn::tri(T::col(cb[r])) + T::col(ca[r]);
        acc[r] = 0.0;
    }
    if (inplace) {
        if (m1 > m0) {
#pragma unroll
            for (int r = 0; r < NE; r++) acc[r] = A.hess_base[f * BTW_ROW + slot[r]];
        }
    } else if (rows) {
        btw_d2u pr[BTW_NR];
#pragma unroll
        for (int r = 0; r < BTW_NR; r++) { pr[r].a = 0.0; pr[r].b = 0.0; }
        if (live && A.hess_base) {
#pragma unroll
            for (int r = 0; r < BTW_NR; r++)
                pr[r] = *reinterpret_cast<const btw_d2u *>(A.hess_base + f * BTW_ROW + 2 * min(j + 16 * r, BTW_NP - 1));
        }
#pragma unroll
        for (int r = 0; r < BTW_NR; r++) {
            const int i = min(j + 16 * r, BTW_NP - 1);         // the lanes past piece 247 write piece 247 again: the same values
            row[2 * i] = pr[r].a; row[2 * i + 1] = pr[r].b;
        }
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < NE; r++) acc[r] = row[slot[r]];
    }
    double c2sum = (live && A.chi2_base) ? A.chi2_base[f] : 0.0;
    if (m1 > m0) {
        const long long si = min(max(A.idx_i ? (long long)A.idx_i[f] : f, 0ll), A.S - 1);
        const long long sj = min(max(A.idx_j ? (long long)A.idx_j[f] : f + 1, 0ll), A.S - 1);
        const double *pi = A.states + si * 16, *pj = A.states + sj * 16;
        NavState xi, xj;
        xi.q = ldq4(pi); xi.bg = mk(0.0, 0.0, 0.0); xi.v = xi.bg; xi.ba = xi.bg; xi.p = ldv3(pi + 13);
        xj.q = ldq4(pj); xj.bg = xi.bg; xj.v = xi.bg; xj.ba = xi.bg; xj.p = ldv3(pj + 13);
        const chn::BetweenGeo g = chn::between_geometry<K>(xi, xj);
        double Jc[T::D];
        chn::between_jcol<K>(g, min(j, T::NC - 2), Jc);
        for (long long m = m0; m < m1; m++) {
            const double *zp = A.z + m * T::ZN, *Rm = A.R + m * T::RN;
            double z[T::ZN], R[T::RN], e[T::D], wh[T::D], u[T::D], Ac[T::D];
#pragma unroll
            for (int i = 0; i < T::ZN; i++) z[i] = zp[i];
#pragma unroll
            for (int i = 0; i < T::RN; i++) R[i] = Rm[i];
            const double w = A.weight ? A.weight[m] : 1.0;
            chn::between_residual<K>(g, z, e);
            const double c2 = chn::fix_vectors<T::D>(R, e, wh, u);
            c2sum = fma(w, c2, c2sum);
            if (A.chi2_m && j == 0) A.chi2_m[m] = c2;
            if (rows) {
                chn::between_acol<T::D>(R, Jc, Ac);
#pragma unroll
                for (int r = 0; r < T::D; r++) tile[r * 16 + j] = (j == T::NC - 1) ? -wh[r] : Ac[r];
                wave_lds_fence();
#pragma unroll
                for (int r = 0; r < NE; r++) acc[r] = fma(w, chn::between_term<T::D>(tile + ca[r], tile + cb[r], 16), acc[r]);
                wave_lds_fence();
            }
        }
    }
    if (live && A.chi2 && j == 0) A.chi2[f] = c2sum;
    if (!rows) return;
    if (inplace) {
        if (m1 > m0) {
#pragma unroll
            for (int r = 0; r < NE; r++)
                if (j + 16 * r < T::NT) A.hess[f * BTW_ROW + slot[r]] = acc[r];
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < NE; r++)
        if (j + 16 * r < T::NT) row[slot[r]] = acc[r];
    wave_lds_fence();
    if (!live) return;
    double *dst = A.hess + f * BTW_ROW;
#pragma unroll
    for (int r = 0; r < BTW_NR; r++) {
        const int k = j + 16 * r;
        if (k < BTW_NP) st16_nt(dst + 2 * k, row[2 * k], row[2 * k + 1]);
    }
}

}  // namespace
