// cpi_mean_kernels.hpp -- the mean (+ analytic Jacobian) recursion: cpi_mean_kernel (dense / ragged layouts) and cpi_mean_tiled_kernel (tiled layout).
// Part of the translation unit cpi_mean.hip (included there after cpi_math.hpp / cpi_device_util.hpp; not a stand-alone header).
#pragma once

namespace {

// Number of knots with stamp <= T (stamps non-decreasing).  An IMU stream is sampled almost uniformly, so the answer lies
// within a few knots of the linear interpolation between the stream's ends: gallop from that guess until T is bracketed,
// then bisect the bracket -- typically 3-5 probes inside one or two cache lines, where a plain bisection of a 50 M-knot
// stream takes 26 probes of which the last ten are private to the window (measured: 2.4 KB of extra HBM traffic per window).
__device__ __forceinline__ long long knots_not_after(const double *stream, long long K, double T) {
    const double t0 = stream[0], t1 = stream[(K - 1) * 7];
    if (!(T >= t0)) return 0;
    if (T >= t1) return K;
    long long g = (long long)((T - t0) / (t1 - t0) * (double)(K - 1));
    g = min(max(g, 0ll), K - 1);
    long long lo, hi;                       // invariant: stream[lo - 1] <= T (or lo == 0), stream[hi] > T (or hi == K)
    if (stream[g * 7] <= T) {
        lo = g + 1; hi = K;
        for (long long step = 1; lo < K; step <<= 1) {
            const long long p = min(g + step, K - 1);
            if (stream[p * 7] <= T) { lo = p + 1; if (p == K - 1) break; } else { hi = p; break; }
        }
    } else {
        hi = g; lo = 0;
        for (long long step = 1; hi > 0; step <<= 1) {
            const long long p = max(g - step, 0ll);
            if (stream[p * 7] <= T) { lo = p + 1; break; } else { hi = p; if (p == 0) break; }
        }
    }
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (stream[mid * 7] <= T) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The same count with ONE memory round trip in the common case: the four stamps around the interpolation guess are requested
// together (one or two cache lines) and resolved with compares; only a guess that does not bracket T (a stream with gaps)
// falls back to the gallop above.  The answer is unique for non-decreasing stamps, so both routes return the same number.
// Used by the fused cut in the prologue of cpi_mean_kernel<..., CUT = 2>, where every dependent round trip is exposed
// latency of a whole wavefront.  t0 / t1: stamps of the first / last reading.
__device__ __forceinline__ long long knots_not_after_near(const double *stream, long long K, double t0, double t1, double T,
                                                          double &last_stamp) {
    // last_stamp: the stamp of knot (result - 1) when result > 0 -- one of the probes in the common case, so the caller's
    // "stamp of the front reading" costs no further round trip
    last_stamp = t0;
    if (!(T >= t0)) return 0;
    if (T >= t1) { last_stamp = t1; return K; }
    long long g = (long long)((T - t0) / (t1 - t0) * (double)(K - 1));
    g = min(max(g, 1ll), K - 3);          // probes g - 1 .. g + 2 (K >= 4 is checked by the caller)
    const double pa = stream[(g - 1) * 7], pb = stream[g * 7], pc = stream[(g + 1) * 7], pd = stream[(g + 2) * 7];
    if (pa <= T && T < pd) {              // #{t <= T} = (g - 1) + 1 + [pb <= T] + [pc <= T]
        last_stamp = (pc <= T) ? pc : ((pb <= T) ? pb : pa);
        return g + (pb <= T ? 1 : 0) + (pc <= T ? 1 : 0);
    }
    const long long r = knots_not_after(stream, K, T);
    last_stamp = stream[max(r - 1, 0ll) * 7];
    return r;
}

// ---- many streams in one call (cpi_preintegrate_streams; RunArgs: cpi_args.hpp)
// The run that owns window u: the last r with uoff[r] <= u, by bisection over uoff[1 .. R - 1] -- whatever the offsets hold
// (they live in device memory), the result lies in [0, R - 1].  log2(R) dependent loads of one small array.
__device__ __forceinline__ int run_of(const RunArgs &RA, long long u) {
    int lo = 0, hi = RA.R;                // the run lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);   // (lo + hi overflows an int for R > 2^30)
        if (RA.uoff[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}
// knots_not_after_near for the n readings of one run, which may hold fewer than the four it probes
__device__ __forceinline__ long long knots_in_run(const double *s, long long n, double t0, double t1, double T, double &last_stamp) {
    if (n >= 4) return knots_not_after_near(s, n, t0, t1, T, last_stamp);
    long long c = 0;
    while (c < n && s[c * 7] <= T) c++;
    last_stamp = c > 0 ? s[(c - 1) * 7] : t0;
    return c;
}
// Window u of run r, cut the way cpi_cut_windows_kernel cuts window u - uoff[r] of a stream holding that run's readings alone
// (its first window starts at the run's first reading).  The offsets are clamped into [0, K] (knots) and [0, u] (the run's
// first window); a run without readings yields a window of 0 intervals based on a knot that exists (K >= 1: the entry
// refuses an empty stream), so the kernels that read it stay inside the stream.
struct RunWindow {
    long long k0;      // the front reading (global knot index)
    int cnt;           // TRUE intervals (whole + tail)
    double t_start;    // stamp of the front reading
    bool tail;         // the last interval is [stamp of the last real knot, T]
};
__device__ __forceinline__ RunWindow run_window(const double *stream, long long K, const double *update, const RunArgs &RA, int r, long long u) {
    const long long kb = min(max(RA.soff[r], 0ll), K);
    const long long kn = min(max(RA.soff[r + 1], kb), K) - kb;
    // the run's first window -- or an offset past u, treated as one.  Window 0 is always a first window, whatever uoff[r] holds
    // (a negative offset must not send it to update[-1]): every other window has a predecessor in update[].
    const bool head = u <= max(RA.uoff[r], 0ll);
    const double *rs = stream + kb * 7;
    const double t0 = kn > 0 ? rs[0] : 0.0, t1 = kn > 0 ? rs[(kn - 1) * 7] : 0.0;
    const double T = update[u], Tp = update[head ? u : u - 1];
    double stT, stP;
    const long long cT = knots_in_run(rs, kn, t0, t1, T, stT);
    const long long cP = knots_in_run(rs, kn, t0, t1, Tp, stP);
    const long long fp = head ? 0ll : max(cP - 1, 0ll);
    RunWindow o;
    o.t_start = head ? t0 : fmax(Tp, t0);
    const long long fu = max(max(cT - 1, 0ll), fp);
    const int m = (int)min(fu - fp, (long long)0x3fffffff);
    const double front_t = (m > 0) ? stT : o.t_start;                   // m > 0: fu = cT - 1, whose stamp the search returned
    o.tail = kn > 0 && (T - front_t) > 0;
    o.cnt = m + (o.tail ? 1 : 0);
    o.k0 = kn > 0 ? kb + fp : min(kb, K - 1);
    return o;
}

// ============================================================================================
// mean (+ analytic Jacobian) kernel
// ============================================================================================
#ifndef CPI_MEAN_WPS
#define CPI_MEAN_WPS 1
#endif
#ifndef CPI_MEAN_C
#define CPI_MEAN_C 2      // knots per chunk of the staged kernels with several intervals per lane (3 measured: see below)
#endif
#ifndef CPI_MEAN_BIG_C
#define CPI_MEAN_BIG_C 3  // knots per chunk of the BIG instantiations (round 6, short windows: 2 and 5 measured at N = 10 / 20, profiles/r06_short_windows.md)
#endif

// CUT: the windows are cut out of one stream in flight (cpi_preintegrate_stream) -- a template parameter, so that the
// plain-knot instantiations carry none of it (the 10 k-window headline launch is issue-bound: a few extra live registers
// and selects per interval cost it 3-4 %).  1: the cut was made by cpi_cut_windows_kernel (PreArgs::first / count / tstart /
// tend: the workspace route, shared with the covariance kernels); 2: FUSED -- the wavefront cuts its own windows in its
// prologue from PreArgs::update (mean-only requests: no cut kernel, no 56 bytes of workspace traffic per window, and the
// search probes land on the lines the window reads anyway).
// BIG (one lane per window, mean-only, batches that fill the chip many times over): THREE knots per chunk instead of two.
// 21 staged doubles per lane do not fit beside round 3's per-element bookkeeping (a 64-bit pointer, a 32-bit fast-path offset,
// the last valid chunk and the LDS slot per element: 266 registers, one wavefront per SIMD -- which cut the HBM traffic of a 1 M
// launch from 1.26 x to 1.08 x algorithmic but not its time, profiles/r04_mean_chunk_ab.md part B), so BIG keeps ONE 32-bit byte
// offset per element, relative to the wavefront's lowest knot (a wave-uniform base in SGPRs), for the fast path (constant) and
// the per-element path (advanced per chunk) alike, and its LDS tile is flat (pitch 21 doubles: element e of lane i sits at
// 64 e + i, an immediate offset) -- two wavefronts per SIMD again, 2-3 % faster than the two-knot kernel on large batches and 7 %
// on ragged stream windows; the over-fetch at that occupancy is back at 1.37-1.48 x (it is an L2-capacity effect: part D).  The
// launcher admits BIG only where every lane-segment of a wavefront lies within 2^32 bytes above the lowest one: stream windows of
// a stream of < 2^26 readings, or the dense layout (cpi_mean.hip: launch_mean_L).  5 knots per chunk, and two chunks fetched
// back to back per trip, are slower.
// CARRY (cpi_mean_carry_kernel, cpi_preintegrate_resume): lane 0 of a window -- the earliest segment -- starts from the
// window's carry record instead of the zero state, so the ordered tree below composes "carried state o this call's
// intervals" unchanged.  That holds for the model-2 segments with a gravity response (GSEG) too: lane 0 integrates with the
// carried rotation, i.e. in the window-start frame, and its gravity response starts at zero because the carried means
// already contain the gravity of the intervals before.  The window's final state is written back to the record.
// CUT = 3 (cpi_mean_runs_kernel, mean-only requests of cpi_preintegrate_streams): CUT = 2 for windows of many runs -- the
// prologue first finds the run of its window (RunArgs), then cuts the window out of that run's readings; everything after the
// prologue is the CUT = 2 path on the whole stream.
// Kernel-argument preloading (gfx950 delivers the first kernel-argument dwords in SGPRs when the wave is dispatched; build.py
// passes the backend's preload count): only leading scalar / pointer parameters are preloaded, never the fields of a by-value
// aggregate, so what the prologue reads before its first vector load travels as leading plain parameters, in order of first use
// (12 dwords), and the body reads these names instead of the copies in PreArgs, which follows unchanged.
#define CPI_MEAN_LEAD_PARAMS const double *knots, const double *lin, long long W, int N, const long long *first, const int *count
#define CPI_MEAN_LEAD(a) (a).knots, (a).lin, (a).W, (a).N, (a).first, (a).count
// the same for cpi_mean_tiled_kernel (TiledArgs; 14 dwords)
#define CPI_TILED_LEAD_PARAMS const double *tiles, long long ts, long long ss, long long W, int N, const int *count, const double *lin
#define CPI_TILED_LEAD(a) (a).tiles, (a).ts, (a).ss, (a).W, (a).N, (a).count, (a).lin
template <int MODEL, bool JAC, bool AVG, int L, int CUT, bool BIG = false>
__global__ __launch_bounds__(64, BIG ? 2 : (((MODEL == 2 && !JAC) || (MODEL == 1 && JAC)) && L == 1 ? 2 : CPI_MEAN_WPS)) void cpi_mean_kernel(CPI_MEAN_LEAD_PARAMS, PreArgs A) {
    constexpr bool CARRY = false;
    [[maybe_unused]] const CarryArgs CA = {};
    [[maybe_unused]] const RunArgs RA = {};
#include "cpi_mean_body.inc"
}
// cpi_preintegrate_resume: the plain-knot path of cpi_mean_kernel<MODEL, JAC, AVG, L, 0> from and to carry records
template <int MODEL, bool JAC, bool AVG, int L>
__global__ __launch_bounds__(64, (((MODEL == 2 && !JAC) || (MODEL == 1 && JAC)) && L == 1 ? 2 : CPI_MEAN_WPS)) void cpi_mean_carry_kernel(CPI_MEAN_LEAD_PARAMS, PreArgs A, CarryArgs CA) {
    constexpr bool CARRY = true;
    constexpr int CUT = 0;
    constexpr bool BIG = false;
    [[maybe_unused]] const RunArgs RA = {};
#include "cpi_mean_body.inc"
}
// cpi_preintegrate_streams, mean-only: cpi_mean_kernel<MODEL, false, AVG, L, 3, BIG> -- its own __global__ only because the run
// offsets travel as a second argument (RunArgs) instead of growing PreArgs
template <int MODEL, bool AVG, int L, bool BIG>
__global__ __launch_bounds__(64, BIG ? 2 : ((MODEL == 2 && L == 1) ? 2 : CPI_MEAN_WPS)) void cpi_mean_runs_kernel(CPI_MEAN_LEAD_PARAMS, PreArgs A, RunArgs RA) {
    constexpr bool JAC = false;
    constexpr int CUT = 3;
    constexpr bool CARRY = false;
    [[maybe_unused]] const CarryArgs CA = {};
#include "cpi_mean_body.inc"
}

// ============================================================================================
// mean kernel on the TILED layout: knots of 64 windows interleaved per step (cpi_preintegrate_tiled_batch)
// ============================================================================================
// tiles[b][s][k][i] = field k (t, w, a) of knot s of window 64 b + i.  A wavefront owns tile b, lane i window 64 b + i, and
// step s reads seven fully coalesced 512-byte rows: the whole batch is ONE linear stream per wavefront, every byte
// fetched once, no LDS, no staging, ~100 registers (4 wavefronts per SIMD) -- the layout the recursion wants on this
// memory system, for producers that can write it (a batch assembler that places knot s of window w at its tile slot instead of
// at w (N+1) + s costs nothing extra).  Knots are prefetched three steps ahead in registers.
// (TiledArgs: cpi_args.hpp)
#ifndef CPI_TILED_OCC
#define CPI_TILED_OCC (MODEL == 2 ? 2 : 3)
#endif
#ifndef CPI_TILED_BUFS
#define CPI_TILED_BUFS 5
#endif

// SPLIT (small batches: fewer tiles than the chip has SIMDs): a workgroup of S = blockDim.x / 64 wavefronts owns the
// tile; wavefront j integrates the steps [j per, (j + 1) per) of all 64 windows from the identity (model 2: from the raw
// specific force, with the segment's gravity response -- cpi_math.hpp mean_step_v2seg), parks its segment in LDS, and
// wavefront 0 composes the S segments in order (mean_combine / grav_combine: the composition cpi_mean_kernel uses
// across the lanes of a window).  Each wavefront still reads one linear stream.
template <int MODEL, bool AVG, bool COUNTED, bool SPLIT>
__global__ __launch_bounds__(SPLIT ? 512 : 64, SPLIT ? 1 : CPI_TILED_OCC) void cpi_mean_tiled_kernel(CPI_TILED_LEAD_PARAMS, TiledArgs A) {
    constexpr bool GSEG = SPLIT && MODEL == 2;
    constexpr int NF = GSEG ? 34 : 16;            // doubles of a parked segment
    extern __shared__ double seg[];               // [S - 1][NF][64]
    const int lane = threadIdx.x & 63;
    const int j = SPLIT ? (int)(threadIdx.x >> 6) : 0, S = SPLIT ? (int)(blockDim.x >> 6) : 1;
    const long long w = (long long)blockIdx.x * 64 + lane;
    const bool valid = w < W;
    const long long wc = valid ? w : W - 1;
    const int n = valid ? (COUNTED ? min(max(count[wc], 0), N) : N) : 0;
    const int nmax = COUNTED ? __builtin_amdgcn_readfirstlane(wave_max(n)) : N;
    const int per = SPLIT ? (N + S - 1) / S : N;
    const int sb = __builtin_amdgcn_readfirstlane(j * per), se = min(sb + per, nmax);   // this wavefront's steps
    const double *tb = tiles + (long long)blockIdx.x * ts + lane;   // a step of a tile: 448 doubles = 7 fields x 64 windows
    const V3 bw = ldv3(lin + wc * 6), ba = ldv3(lin + wc * 6 + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2 && j == 0) gk = mul(quat_2_Rot(ldq4(A.qk + wc * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));
    auto load = [&](double (&k)[7], int s) {
        // COUNTED: past its own last knot a lane re-reads that knot (dt = 0) -- what lies behind it in the column is
        // never read.  Otherwise the row offset is wave-uniform (scalar address arithmetic).
        const double *p = tb + (long long)(COUNTED ? min(s, n) : min(s, N)) * ss;
        // non-temporal: every byte of a tile is read exactly once, by one wavefront (round 4, same-box A/B: 1 M x 50 582-588 ->
        // 565-569 us, model 2 561-576 -> 540 us, 100 k 60.5 -> 56 us; the same hint on the dense layout's staged loads, whose
        // 128-byte lines ARE touched again by the next chunk, costs 35 %: 619 -> 840-874 us)
#pragma unroll
        for (int f = 0; f < 7; f++) k[f] = __builtin_nontemporal_load(p + f * 64);
    };
    MeanState<false> st;
    mean_init(st);
    GravAcc ga;
    if (GSEG) grav_init(ga);
    // the knot buffers rotate by NAME over one unrolled trip (a rolled loop spends 28 v_mov_b64 per step on it)
#define CPI_TSTEP(a, b, e, S_)                                                                                        \
    load(e, (S_) + CPI_TILED_BUFS - 1);                                                                               \
    if constexpr (GSEG)                                                                                               \
        mean_step_v2seg<AVG>(st, ga, a[0], b[0], mk(a[1], a[2], a[3]), mk(a[4], a[5], a[6]), mk(b[1], b[2], b[3]),    \
                             mk(b[4], b[5], b[6]), bw, ba, (S_) < n);                                                 \
    else                                                                                                              \
        mean_step<MODEL, false, AVG>(st, a[0], b[0], mk(a[1], a[2], a[3]), mk(a[4], a[5], a[6]), mk(b[1], b[2], b[3]), \
                                     mk(b[4], b[5], b[6]), bw, ba, gk, (S_) < n)
#if CPI_TILED_BUFS == 5
    double k0[7], k1[7], k2[7], k3[7], k4[7];
    load(k0, sb); load(k1, sb + 1); load(k2, sb + 2); load(k3, sb + 3);
    for (int s = sb; s < se; s += 5) {
        CPI_TSTEP(k0, k1, k4, s);
        if (s + 1 >= se) break;
        CPI_TSTEP(k1, k2, k0, s + 1);
        if (s + 2 >= se) break;
        CPI_TSTEP(k2, k3, k1, s + 2);
        if (s + 3 >= se) break;
        CPI_TSTEP(k3, k4, k2, s + 3);
        if (s + 4 >= se) break;
        CPI_TSTEP(k4, k0, k3, s + 4);
    }
#elif CPI_TILED_BUFS == 4
    double k0[7], k1[7], k2[7], k3[7];
    load(k0, sb); load(k1, sb + 1); load(k2, sb + 2);
    for (int s = sb; s < se; s += 4) {
        CPI_TSTEP(k0, k1, k3, s);
        if (s + 1 >= se) break;
        CPI_TSTEP(k1, k2, k0, s + 1);
        if (s + 2 >= se) break;
        CPI_TSTEP(k2, k3, k1, s + 2);
        if (s + 3 >= se) break;
        CPI_TSTEP(k3, k0, k2, s + 3);
    }
#else
    double k0[7], k1[7], k2[7];
    load(k0, sb); load(k1, sb + 1);
    for (int s = sb; s < se; s += 3) {
        CPI_TSTEP(k0, k1, k2, s);
        if (s + 1 >= se) break;
        CPI_TSTEP(k1, k2, k0, s + 1);
        if (s + 2 >= se) break;
        CPI_TSTEP(k2, k0, k1, s + 2);
    }
#endif
#undef CPI_TSTEP
    if constexpr (SPLIT) {
        auto park = [&](int f, double v) { seg[((j - 1) * NF + f) * 64 + lane] = v; };
        if (j > 0) {
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) park(r * 3 + c, st.R.m[r][c]);
            park(9, st.alpha.x); park(10, st.alpha.y); park(11, st.alpha.z);
            park(12, st.beta.x); park(13, st.beta.y); park(14, st.beta.z); park(15, st.DT);
            if constexpr (GSEG) {
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) { park(16 + r * 3 + c, ga.Gam.m[r][c]); park(25 + r * 3 + c, ga.Lam.m[r][c]); }
            }
        }
        __syncthreads();
        if (j > 0) return;
        for (int jj = 1; jj < S; ++jj) {        // earlier o later, in order
            const double *sp = seg + (jj - 1) * NF * 64 + lane;
            MeanState<false> B;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) B.R.m[r][c] = sp[(r * 3 + c) * 64];
            B.alpha = mk(sp[9 * 64], sp[10 * 64], sp[11 * 64]);
            B.beta = mk(sp[12 * 64], sp[13 * 64], sp[14 * 64]);
            B.DT = sp[15 * 64];
            if constexpr (GSEG) {
                GravAcc gB;
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) { gB.Gam.m[r][c] = sp[(16 + r * 3 + c) * 64]; gB.Lam.m[r][c] = sp[(25 + r * 3 + c) * 64]; }
                grav_combine(ga, st, gB, B);    // before mean_combine: needs st.R and B.DT as they are
            }
            mean_combine(st, B);
        }
        if constexpr (GSEG) grav_apply(st, ga, gk);
    }
    if (!valid) return;
    if (A.out.DT) A.out.DT[w] = st.DT;
    if (A.out.alpha) stv3(A.out.alpha + w * 3, st.alpha);
    if (A.out.beta) stv3(A.out.beta + w * 3, st.beta);
    if (A.out.q) {
        const Q4 q = rot_2_quat(st.R);
        double *p = A.out.q + w * 4;
        p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
    }
}
#ifdef CPI_EXPERIMENTS
// measurement only (CPI_AMD_BLK_MODE=1): the tiled stream alone -- the same loads, one add per value
__global__ __launch_bounds__(64, 3) void cpi_tiled_fetch_probe_kernel(TiledArgs A) {
    const int lane = threadIdx.x;
    const long long w = (long long)blockIdx.x * 64 + lane;
    const double *tb = A.tiles + (long long)blockIdx.x * A.ts + lane;
    auto load = [&](double (&k)[7], int s) {
        const double *p = tb + (long long)min(s, A.N) * A.ss;
#pragma unroll
        for (int f = 0; f < 7; f++) k[f] = p[f * 64];
    };
    double k0[7], k1[7], k2[7], k3[7], acc = 0;
    load(k0, 0); load(k1, 1); load(k2, 2); load(k3, 3);
    for (int s = 0; s < A.N; ++s) {
        double k4[7];
        load(k4, s + 4);
#pragma unroll
        for (int f = 0; f < 7; f++) { acc += k0[f]; k0[f] = k1[f]; k1[f] = k2[f]; k2[f] = k3[f]; k3[f] = k4[f]; }
    }
    if (w < A.W && A.out.DT) A.out.DT[w] = acc;
}
#endif
// knots[W][N+1][7] (first == NULL) or a shared stream indexed by first[W] / count[W] (the ragged layout of
// cpi_preintegrate_batch) -> tiles[ceil(W/64)][N+1][7][64].  Rows past a window's last knot repeat that knot and columns
// past W repeat window W - 1: finite padding the kernels never integrate.
__global__ __launch_bounds__(256) void cpi_tile_knots_kernel(long long W, int N, const double *knots, const long long *first,
                                                             const int *count, double *tiles, long long ts, long long ss) {
    const long long total = ((W + 63) / 64) * (long long)(N + 1) * 448;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const int i = (int)(o & 63);
        const long long r = o >> 6;
        const int f = (int)(r % 7);
        const long long bs = r / 7;
        const int sidx = (int)(bs % (N + 1));
        const long long b = bs / (N + 1);
        const long long w = min(b * 64 + i, W - 1);
        const long long k0 = first ? first[w] : w * (long long)(N + 1);
        const int n = count ? min(max(count[w], 0), N) : N;
        tiles[b * ts + sidx * ss + f * 64 + i] = knots[(k0 + min(sidx, n)) * 7 + f];
    }
}

// Window assembly on the device, straight into the tiled layout (cpi_assemble_tiles): ONE IMU stream cut at successive
// update times with the semantics of GraphSolver::createimufactor_cpi_v1/v2 (GraphSolver_IMU.cpp:50-69) -- whole
// intervals while imu_times[1] <= updatetime, then the partial tail interval with the front reading repeated, after which
// the front stamp is overwritten by the update time.  The reference walks a deque, i.e. window u starts where window
// u - 1 stopped; for a stream whose stamps are non-decreasing (and update times likewise) that state is a pure function of
// the previous update time, so every window is independent here:
//     front(T)  = max(#{knots with t <= T} - 1, 0)          (the deque's front index after the window ending at T)
//     stamp(T)  = max(T, t_0)                               (the front stamp after that window)
// One wavefront per tile, one lane per window; a row of the tile is seven coalesced 512-byte stores.
// The same cut WITHOUT moving a knot (cpi_preintegrate_stream): per window the front reading's index, the interval count
// (whole + tail), the start stamp and the update time of a tail interval (NaN: none) -- 28 bytes per window; the
// preintegration kernels then read the stream in place (PreArgs::tstart / tend).
__global__ __launch_bounds__(256) void cpi_cut_windows_kernel(long long K, const double *stream, long long U, const double *update,
                                                              long long *first, int *count, double *tstart, double *tend) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    const double t0 = stream[0], t1 = stream[(K - 1) * 7], T = update[u];
    const bool near_ok = K >= 4;          // one round trip per search in the common case (knots_not_after_near)
    long long fp = 0;
    double start_t = t0, stT = t0, stP;
    const long long cT = near_ok ? knots_not_after_near(stream, K, t0, t1, T, stT) : knots_not_after(stream, K, T);
    if (u > 0) {
        const double Tp = update[u - 1];
        fp = max((near_ok ? knots_not_after_near(stream, K, t0, t1, Tp, stP) : knots_not_after(stream, K, Tp)) - 1, 0ll);
        start_t = fmax(Tp, t0);
    }
    const long long fu = max(max(cT - 1, 0ll), fp);
    const int m = (int)min(fu - fp, (long long)0x3fffffff);
    const double front_t = (m > 0) ? (near_ok ? stT : stream[fu * 7]) : start_t;
    const bool tail = (T - front_t) > 0;
    first[u] = fp; count[u] = m + (tail ? 1 : 0); tstart[u] = start_t;
    tend[u] = tail ? T : __builtin_nan("");
}
// The same 28 bytes per window for the windows of many runs (cpi_preintegrate_streams): first[u] indexes the whole stream, so
// the covariance, Forster and analytic-Jacobian kernels read multi-run windows through their CUT = 1 path unchanged.
__global__ __launch_bounds__(256) void cpi_cut_runs_kernel(long long K, const double *stream, long long U, const double *update, RunArgs RA,
                                                           long long *first, int *count, double *tstart, double *tend) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    const RunWindow c = run_window(stream, K, update, RA, run_of(RA, u), u);
    first[u] = c.k0; count[u] = c.cnt; tstart[u] = c.t_start;
    tend[u] = c.tail ? update[u] : __builtin_nan("");
}
// Rows leave as coalesced 512-byte stores (lane = window).  It is a copy with a transposition in it; designs measured on the
// 1 M x 50 batch (profiles/r04_assembler.md):
//   * round 3: lane i loads its own window's knots (8 B per lane and instruction, 64 different 128-byte lines per instruction):
//     1.46-1.48 ms = 3.9 TB/s of read + write;
//   * SHIPPED: the RB = 8 rows of a trip travel as LDS-DMA (glds16) -- one instruction fetches the 448 contiguous bytes of TWO
//     windows (28 lanes x 16 B each), 32 instructions fill a 33-KB image of the trip's 64 x 8 knots, no staging registers, 8
//     lines per instruction instead of 64 --, and lane i then reads ITS window's values out of the image (pitch 1040 B per
//     instruction image: 2-way bank conflicts, the minimum of this placement) for the row stores: 1.16-1.21 ms = 4.7-4.9 TB/s
//     algorithmic, 5.96 TB/s of real traffic (the 8-byte aligned pieces over-fetch 1.49 x on the read side);
//   * 16-byte stores / 4 rows per trip (9 wavefronts per CU): 1.20 / 1.27 ms -- neither store issue nor occupancy paces it;
//   * every line once: a wavefront owning 16 whole windows (128-byte row pieces: 1.79 ms -- small write pieces stream at half
//     rate), line-aligned 512-byte trips with a carry for the straddling knot, rows stored out of step (reads 1.14 x, writes
//     + 29 %: 1.40 ms) or in step with a 320-byte carry (traffic 1.05 x in total, but 54 KB of LDS = 3 wavefronts per CU:
//     1.34 ms).  Commit "experiment (not shipped): line-aligned assembler" holds the last of them.
//   * round 5: the next trip's LDS-DMA issued under the current trip's row stores (4 rows per trip, two 17-KB images, the landing
//     waited for as vmcnt(28) on exact store counts): reads 1.36 x -> 1.16 x, latency hidden, 1.13-1.16 ms -- the SAME time
//     (profiles/r05_assembler.md; commit "experiment (not shipped): assembler with the next trip's DMA under the row stores").
//     5.0 TB/s of algorithmic read + write is what a 1 : 1 copy of 448-byte pieces into 512-byte rows gets on this memory system.
// The DMA route needs the wavefront's windows within 2^24 knots above the first one and K >= RB (wave-uniform test); any
// other wavefront takes the per-lane loads of round 3.
#ifndef CPI_ASM_RB
#define CPI_ASM_RB 8
#endif
__global__ __launch_bounds__(64) void cpi_assemble_tiles_kernel(AssembleArgs A) {
    constexpr int RB = CPI_ASM_RB;              // rows per trip
    constexpr int PPW = RB * 56 / 16;           // 16-byte pieces of a window's trip: 28
    constexpr int WPI = 64 / PPW;               // windows per DMA instruction: 2
    constexpr int NI = 64 / WPI;                // DMA instructions per trip: 32
    constexpr int IMG = (RB == 8) ? 1040 : 1072;   // bytes between instruction images: 2-way (RB = 8) / 3-way (RB = 4) read conflicts, the minima of these placements
    static_assert((RB == 8 && WPI == 2) || (RB == 4 && WPI == 4), "RB = 8: two windows per instruction; RB = 4: four");
    __shared__ __attribute__((aligned(1024))) char img[NI * IMG];
    __shared__ int srel[64];
    const int lane = threadIdx.x;
    const long long u = (long long)blockIdx.x * 64 + lane;
    const bool valid = u < A.U;
    const long long uc = valid ? u : A.U - 1;
    const double t0 = A.stream[0], tl_ = A.stream[(A.K - 1) * 7];
    const double T = A.update[uc];
    long long fp = 0;
    double start_t = t0;
    double stT, stP;
    const bool near_ok = A.K >= 4;
    const long long cT = near_ok ? knots_not_after_near(A.stream, A.K, t0, tl_, T, stT) : knots_not_after(A.stream, A.K, T);
    if (uc > 0) {
        const double Tp = A.update[uc - 1];
        const long long cP = near_ok ? knots_not_after_near(A.stream, A.K, t0, tl_, Tp, stP) : knots_not_after(A.stream, A.K, Tp);
        fp = max(cP - 1, 0ll);
        start_t = fmax(Tp, t0);
    }
    const long long fu = max(max(cT - 1, 0ll), fp);
    const int m = (int)min(fu - fp, (long long)0x3fffffff);          // whole intervals
    const double front_t = (m > 0) ? (near_ok ? stT : A.stream[fu * 7]) : start_t;   // m > 0: fu = cT - 1, whose stamp the search returned
    const bool tail = (T - front_t) > 0;
    const int cnt = m + (tail ? 1 : 0);
    if (valid) A.count[u] = cnt;                                      // the TRUE count: a caller can check max(count) <= N
    const int rows = min(cnt, A.N);                                   // rows 0 .. rows exist in the tile
    const int rmax = __builtin_amdgcn_readfirstlane(wave_max(rows));
    double *tb = A.tiles + (long long)blockIdx.x * A.ts + lane;

    const long long base = min(readfirstlane64(fp), A.K - RB);        // wave-uniform; the DMA offsets are relative to it
    const bool dma = __all((A.K >= RB) && (fp >= readfirstlane64(fp)) && (fp + (long long)m - base < (1ll << 24)));
    if (dma) {
        const char *sbase = reinterpret_cast<const char *>(A.stream + base * 7);
        const int dw = min(lane / PPW, WPI - 1);                      // lanes 56..63 re-fetch a piece of the second window
        const int dp = (lane < PPW * WPI) ? lane - dw * PPW : 0;
        const unsigned img_base = (unsigned)(size_t)((__attribute__((address_space(3))) char *)img);
        const char *mine = img + (lane / WPI) * IMG + (lane % WPI) * (PPW * 16);   // this lane's window in the image
        for (int r0 = 0; r0 <= rmax; r0 += RB) {
            // the trip's RB knots of window i start at knot fp + min(r0, m) (rows past m repeat knot m: the tail row is knot
            // m's reading under the update time), pulled back so that the piece stays inside the stream
            const long long st = min(fp + (long long)min(r0, m), A.K - RB);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the previous trip's image reads have retired
            srel[lane] = (int)(st - base);
            wave_lds_fence();
            unsigned so[NI];                                          // all offsets first: one LDS round trip, then 32 DMA issues
#pragma unroll
            for (int j = 0; j < NI; ++j) so[j] = (unsigned)srel[j * WPI + dw];
#pragma unroll
            for (int j = 0; j < NI; ++j) glds16(so[j] * 56u + (unsigned)dp * 16u, sbase, img_base + j * IMG);
            wait_vmcnt<0>();
            wave_lds_fence();
#pragma unroll
            for (int i = 0; i < RB; i++) {
                const int r = r0 + i;
                const int jj = (int)(fp + (long long)min(r, m) - st);             // 0 .. RB - 1 for every row that is stored
                const double *src = reinterpret_cast<const double *>(mine + min(max(jj, 0), RB - 1) * 56);
                double v[7];
#pragma unroll
                for (int k = 0; k < 7; k++) v[k] = src[k];
                if (r == 0) v[0] = start_t;
                if (tail && r == m + 1) v[0] = T;
                if (r <= rows) {
                    // non-temporal row stores: 1.17-1.21 -> 1.13 ms per 1 M x 50 (the same hint on the LDS-DMA reads, whose pieces
                    // share lines with the next trip: 1.20 -> 1.35 ms)
#pragma unroll
                    for (int k = 0; k < 7; k++) __builtin_nontemporal_store(v[k], tb + (long long)r * A.ss + k * 64);
                }
            }
        }
        return;
    }
    // per-lane loads (round 3): RB rows per trip, a lane consumes RB x 56 contiguous bytes of the stream while its 128-byte
    // lines are in flight / fresh in the L1
    for (int r0 = 0; r0 <= rmax; r0 += RB) {
        double v[RB][7];
#pragma unroll
        for (int i = 0; i < RB; i++) {
            // row r of this window: r == 0 the front reading under the window's start stamp; 1 .. m stream knots; m + 1 the tail
            const int rr = min(r0 + i, rows);
            const double *kp = A.stream + (fp + min(rr, m)) * 7;
#pragma unroll
            for (int k = 0; k < 7; k++) v[i][k] = kp[k];
            if (rr == 0) v[i][0] = start_t;
            if (tail && rr == m + 1) v[i][0] = T;
        }
#pragma unroll
        for (int i = 0; i < RB; i++) {
            const int r = r0 + i;
            if (r <= rows) {
#pragma unroll
                for (int k = 0; k < 7; k++) tb[(long long)r * A.ss + k * 64] = v[i][k];
            }
        }
    }
}


}  // namespace
