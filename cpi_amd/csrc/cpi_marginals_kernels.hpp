// cpi_marginals_kernels.hpp -- cpi_marginals_kernel: the diagonal and first off-diagonal blocks of the inverse of the block-tridiagonal
// matrix that cpi_chain_solve_batch factorised, from the factor it left in the caller's workspace (cpi_chain_marginals_batch; the
// arithmetic: cpi_math.hpp, chn::marginals_chain, whose lane-mapped form this is).
// Part of the translation unit cpi_marginals.hip (included there after cpi_math.hpp / cpi_device_util.hpp / cpi_factor_kernels.hpp,
// from which it takes dpp_fmac / dpp_fnmac / dpp_mul, and cpi_chain_util.hpp; not a stand-alone header).
//
// 16 lanes (one DPP row) per chain, 4 chains per wavefront, one wavefront per workgroup, s from the chain's last state down to 0.
// Everything is kept by COLUMNS, lane j < 15 owning column j, so that every product is "the broadcast of another lane's register
// times my own" -- one double-precision DPP multiply-add -- and nothing is ever transposed between lanes:
//   Z   = R_s^-T     column j: forward substitution on e_j; R[m][k] is register rr[k] of lane m (lane m loads ROW m of R, as the
//                    solve's back pass does), 1 / R[m][m] its rr[m]
//   KT  = K_s^T = W_s^T Z            KT[c][j] += bcast_k(w[c]) z[k]: lane k loads row k of W, fifteen consecutive doubles
//   Sig = Z^T Z  (= R^-1 R^-T)       Sig[i][j] += bcast_i(z[k]) z[k], k >= i: the pattern of the solve's Schur update
//   T   = P KT,  P = Sigma[s+1][s+1] T[i][j] += bcast_k(p[i]) kt[k]: P is symmetric, column k of it is lane k's
//   Sig += K T                       Sig[i][j] += bcast_i(kt[k]) t[k]
// and Sigma[s][s+1] = -K P = -T^T: lane i writes entry (i, c) of the column-major cross row from its t[c], consecutive lanes to
// consecutive doubles.  Lane j's part of the upper triangle of Sig (rows i <= j) goes to LDS in the packing of the output; from
// there the wavefront writes the cov row in consecutive doubles, and the next trip reads the FULL column j back, the part below the
// diagonal from the mirrored position: Sigma[s][s] is symmetric by construction, one triangle computed and mirrored (480 doubles
// of LDS for the four chains).  At a chain's last state W and P are replaced by zeros: the same instructions, Sig = Z^T Z exactly,
// and the W record that the solve does not write there is fetched (a valid address) but never used.
// The rows R / W of the NEXT trip are requested as soon as Z and KT have consumed this trip's, into the same registers.
// Lanes of a chain that has ended, has not begun (the trip count is the wavefront's longest chain), does not exist or is refused keep
// executing on valid addresses with their stores predicated off: a DPP source must be an active lane.  Lane 15 redoes lane 14.
#pragma once

namespace {

__global__ __launch_bounds__(64, 2) void cpi_marginals_kernel(MarginalsArgs A) {
    constexpr int TD = chn::tri(15);                  // 120: a packed block
    __shared__ __attribute__((aligned(16))) double sP[4 * TD];
    // the furthest entries the column read touches, kept or not, lie inside the chain's block; a row of R read from its start lies
    // inside the record
    static_assert(chn::tri(14) + 14 < TD && 14 + chn::tri(14) < TD && chn::row_off(14) < chn::WS_R && chn::WS_R + 15 * 15 == chn::WS_D,
                  "a read at a constant offset from a lane's base stays inside the block / the record");
    const int lane = threadIdx.x, j = lane & 15, fl = lane >> 4, jc = min(j, 14);
    const long long c = (long long)blockIdx.x * 4 + fl;
    const ChainStates cs = chain_states(A.C, A.G, A.S, A.first, A.count, c);
    const int n = cs.n;
    const int nmax = wave_max(n);
    if (nmax == 0) return;                             // the whole wavefront: nothing to write
    const bool poison = A.status && A.status[cs.cc] != 0;
    const double qnan = __builtin_nan("");
    // the record this lane's group uses while it has none of its own: state 0 exists (nmax > 0)
    const long long f = (n > 0) ? cs.f : 0;
    double *Pq = sP + fl * TD;
    const double *colp = Pq + chn::tri(jc), *rowp = Pq + jc;

    double rr[15], w[15];
    // row jc of R from its start (rr[m] is R[jc][m] for m >= jc, 1 / R[jc][jc] at m == jc and, below that, an entry of an earlier row
    // that no product takes: row_off(k) >= k, still inside the record), row jc of W
    auto fetch = [&](int s) {
        const long long srow = f + ((n > 0) ? min(s, n - 1) : 0);
        const double *rec = A.workspace + srow * chn::WS_D;
        const double *rrow = rec + (chn::row_off(jc) - jc), *wr = rec + chn::WS_R + jc * 15;
#pragma unroll
        for (int m = 0; m < 15; m++) { rr[m] = rrow[m]; w[m] = wr[m]; }
    };
    fetch(nmax - 1);
    for (int s = nmax - 1; s >= 0; s--) {
        const bool act = s < n, hasw = act && s < n - 1;
        const long long srow = f + ((n > 0) ? min(s, n - 1) : 0);
        // ---- Z = R^-T, column jc: t = e_jc; m ascending: z[m] = t[m] / R[m][m]; t[k] -= R[m][k] z[m], k > m
        double z[15];
#pragma unroll
        for (int k = 0; k < 15; k++) z[k] = (k == jc) ? 1.0 : 0.0;
        chain_for<0, 15>([&](auto Mc) {
            constexpr int M = decltype(Mc)::value;
            z[M] = dpp_mul<M>(rr[M], z[M]);
            chain_for<M + 1, 15>([&](auto Kc) {
                constexpr int K = decltype(Kc)::value;
                dpp_fnmac<M>(z[K], rr[K], z[M]);
            });
        });
        chain_settle(z);                               // read as DPP sources below
        __builtin_amdgcn_sched_barrier(0);
        // ---- KT = W^T Z (zeros at the chain's last state), column jc
        double kt[15];
#pragma unroll
        for (int m = 0; m < 15; m++) w[m] = hasw ? w[m] : 0.0;
        chain_settle(w);
        chain_for<0, 15>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
            chain_for<0, 15>([&](auto Cc) {
                constexpr int Cn = decltype(Cc)::value;
                if constexpr (K == 0) kt[Cn] = dpp_mul<K>(w[Cn], z[K]);
                else dpp_fmac<K>(kt[Cn], w[Cn], z[K]);
            });
        });
        chain_settle(kt);
        __builtin_amdgcn_sched_barrier(0);
        // ---- Sig = Z^T Z, column jc
        double sg[15];
        chain_for<0, 15>([&](auto Ic) {
            constexpr int I = decltype(Ic)::value;
            sg[I] = dpp_mul<I>(z[I], z[I]);
            chain_for<I + 1, 15>([&](auto Kc) {
                constexpr int K = decltype(Kc)::value;
                dpp_fmac<I>(sg[I], z[K], z[K]);
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        // rr, w and z are done: the next trip's rows (trip 0 re-reads its own)
        fetch(max(s - 1, 0));
        // ---- T = P KT, column jc: P = the block of state s + 1 as the previous trip left it in LDS, the full symmetric column
        double p[15], t[15];
#pragma unroll
        for (int i = 0; i < 15; i++) {
            const double up = colp[i], lo = rowp[chn::tri(i)];
            const double v = (i <= jc) ? up : lo;
            p[i] = hasw ? v : 0.0;
        }
        chain_settle(p);
        chain_for<0, 15>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
            chain_for<0, 15>([&](auto Ic) {
                constexpr int I = decltype(Ic)::value;
                if constexpr (K == 0) t[I] = dpp_mul<K>(p[I], kt[K]);
                else dpp_fmac<K>(t[I], p[I], kt[K]);
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        // ---- Sig += K T
        chain_for<0, 15>([&](auto Ic) {
            constexpr int I = decltype(Ic)::value;
            chain_for<0, 15>([&](auto Kc) {
                constexpr int K = decltype(Kc)::value;
                dpp_fmac<I>(sg[I], kt[K], t[K]);
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        // ---- Sigma[s][s + 1] = -T^T, column-major: entry (j, k) from t[k]
        if (A.cross && hasw && j < 15) {
            double *x = A.cross + srow * 225 + j;
#pragma unroll
            for (int k = 0; k < 15; k++) x[15 * k] = poison ? qnan : -t[k];
        }
        // ---- the upper triangle to LDS (every read of P is done), the cov row from there, and P of the next trip
        wave_lds_fence();
        if (j < 15) {
#pragma unroll
            for (int i = 0; i < 15; i++)
                if (i <= j) Pq[chn::tri(j) + i] = sg[i];
        }
        wave_lds_fence();
        if (act) {
            double *o = A.cov + srow * TD;
#pragma unroll
            for (int r = 0; r < (TD + 15) / 16; r++) {
                const int e = j + 16 * r;
                if (e < TD) o[e] = poison ? qnan : Pq[e];
            }
        }
    }
}

}  // namespace
