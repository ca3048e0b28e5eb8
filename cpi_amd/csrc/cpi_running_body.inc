// cpi_running_body.inc -- the body of cpi_mean_running_kernel and cpi_mean_stream_running_kernel (cpi_running_kernels.hpp),
// included inside both.  Shared as text rather than through a device function, as cpi_mean_body.inc is: the plain-knot kernel
// compiles to exactly the code it had before the stream form existed.  In scope where it is included: MODEL, JAC, AVG, MULTI,
// CUT (the windows are cut out of a stream in flight), CARRY (cpi_mean_running_carry_kernel: the window continues from / is left
// in a carry record), the kernel arguments A (PreArgs), CA (CarryArgs; read when CARRY only) and L_arg.
    static_assert(!(JAC && MODEL == 2), "model 2's Jacobians are read out of the state transition matrix");
    constexpr int T = CPI_RUN_T;
    constexpr int P1 = T | 1, P3 = (3 * T) | 1, P4 = (4 * T) | 1;   // odd pitches: a lane's slots start in distinct banks
    constexpr bool GSEG = MULTI && MODEL == 2;
    __shared__ double sDT[64 * P1], sAl[64 * P3], sBe[64 * P3], sQ[64 * P4];
    __shared__ long long s_rowbase[64];
    __shared__ int s_lo[64], s_hi[64];

    const int lane = threadIdx.x;
    const int L = MULTI ? L_arg : 1;
    const int WPB = 64 / L;
    const int grp = lane / L, l = lane - grp * L;
    long long w = (long long)blockIdx.x * WPB + grp;
    const bool valid = (w < A.W) && (grp < WPB);       // L not a power of two leaves 64 - WPB L idle lanes
    if (grp >= WPB) w = (long long)blockIdx.x * WPB;
    if (w >= A.W) w = A.W - 1;
    int n;
    long long k0;
    // CUT: knot 0 of the window takes the stamp t_start; a partial tail interval has NO closing knot in memory -- it is the last
    // real knot's reading held until t_end (cpi_mean_body.inc, CUT = 1).  nlast: the window's last knot that exists in memory.
    double t_start = 0.0, t_end = 0.0;
    bool tail = false;
    int nlast;
    if constexpr (CUT) {
        const int c = A.count[w];                                        // the TRUE count: may exceed N
        n = min(max(c, 0), A.N);
        t_start = A.tstart[w]; t_end = A.tend[w];
        tail = (t_end == t_end) && (c <= A.N) && (n > 0);                // NaN = no tail; a truncated window has lost it
        // whatever the workspace holds, every read stays inside the K readings of the stream: the virtual tail knot of a window
        // that ends on the stream's last reading would lie one reading behind the caller's buffer
        k0 = min(max(A.first[w], 0ll), A.K - 1);
        nlast = (int)min((long long)(n - (tail ? 1 : 0)), A.K - 1 - k0);
    } else {
        n = A.count ? min(max(A.count[w], 0), A.N) : A.N;
        k0 = A.first ? A.first[w] : w * (long long)(A.N + 1);
        nlast = n;
    }
    const int per = (A.N + L - 1) / L;                 // rows per lane: wave-uniform
    const int r0 = min(A.N, l * per);
    const int nrows = valid ? min(A.N - r0, per) : 0;
    // knot i of the window, never past its last one (what lies behind belongs to the caller; the repeated knot gives dt = 0)
    auto knot = [&](int i) { return A.knots + (k0 + min(i, nlast)) * 7; };
    // CUT: knot i as the host assembler would have written it -- the tail knot (and its repeats past the window's end, which
    // keep the rows past count exact no-ops) is {t_end, reading of the last real knot}, which is what knot() has just fetched
    auto patch = [&](double *k, int i) {
        const int j = min(i, n);
        k[0] = (tail && j == n) ? t_end : (j == 0 ? t_start : k[0]);
    };

    const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));

    MeanState<JAC> st;
    mean_init(st);
    // CARRY: lane 0 of the window -- the earliest rows -- starts from the record, in pass 1 (so that the scan hands every later
    // lane carried o everything before it) and in the walk.  The record is read straight from memory where it is needed and
    // never kept in a second set of registers: the Jacobian variant has 61 doubles of live state already.
    constexpr int CD = carry::doubles(MODEL);
    bool cbad = false;    // the record does not hold what this call continues: every row and the record left behind become NaN
    bool chead = false;   // the window continues from a record
    int owner = lane;     // the lane whose walked state is the window's final state (the state of row N - 1)
    if constexpr (CARRY) {
        if (CA.in) {
            cbad = !carry_tag_ok(CA.in[w * CD + carry::TAG], CA.need);
            chead = !cbad;
            if (chead && l == 0) carry_load_mean<MODEL, JAC>(st, CA.in + w * CD, A.write_jac != 0);
        }
    }
    int lead = 0;        // leading rows of this lane before its first integrated interval (held back for the fix-up)
    int src = -1;        // the wavefront lane whose last row those rows repeat (-1: none -- the scanned state is exact)
    if constexpr (MULTI) {
        GravAcc ga;
        grav_init(ga);
        double pk[7], nx[7];
        {
            const double *a = knot(r0), *b = knot(r0 + 1);
#pragma unroll
            for (int i = 0; i < 7; i++) { pk[i] = a[i]; nx[i] = b[i]; }
            if constexpr (CUT) { patch(pk, r0); patch(nx, r0 + 1); }
        }
        bool seen = false;
        for (int t = 0; t < per; ++t) {
            double q[7];
#pragma unroll
            for (int i = 0; i < 7; i++) q[i] = nx[i];
            {
                const double *b = knot(r0 + t + 2);
#pragma unroll
                for (int i = 0; i < 7; i++) nx[i] = b[i];
                if constexpr (CUT) patch(nx, r0 + t + 2);
            }
            const bool act = t < nrows;
            const bool moves = act && (q[0] - pk[0] > 0);
            if (!seen && !moves && act) lead++;
            seen = seen || moves;
            if constexpr (GSEG)
                mean_step_v2seg<AVG>(st, ga, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                     mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, act);
            else
                mean_step<MODEL, JAC, AVG>(st, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                           mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, gk, act);
#pragma unroll
            for (int i = 0; i < 7; i++) pk[i] = q[i];
        }
        // ordered inclusive scan: lane l <- (l - d) o l, earlier on the left
        for (int d = 1; d < L; d <<= 1) {
            MeanState<JAC> B = run_shfl_up(st, d);
            GravAcc gB;
            if constexpr (GSEG) gB = run_shfl_up(ga, d);
            if (l >= d) {
                if constexpr (GSEG) { grav_combine(gB, B, ga, st); ga = gB; }   // before mean_combine: needs B.R and st.DT as they are
                mean_combine(B, st);
                st = B;
            }
        }
        // exclusive: the state at this lane's first knot
        {
            MeanState<JAC> B = run_shfl_up(st, 1);
            GravAcc gB;
            if constexpr (GSEG) gB = run_shfl_up(ga, 1);
            if (l == 0) { mean_init(B); if constexpr (GSEG) grav_init(gB); }
            st = B;
            if constexpr (GSEG) grav_apply(st, gB, gk);
        }
        // whose last row do the held-back rows repeat: the nearest earlier lane of the window that integrated anything
        const unsigned long long moved = __ballot(lead < nrows);
        const unsigned long long below = moved & ((1ull << lane) - 1ull) & ~((1ull << (grp * L)) - 1ull);
        src = below ? 63 - __builtin_clzll(below) : -1;
        if (src < 0) lead = 0;
        if constexpr (CARRY) {
            // No earlier lane integrated anything: the state at this lane's first knot IS the carried one, and its leading no-op
            // rows must show it bit for bit -- not `carried o identity o ...` as the scan composed it (mm() with the identity
            // and x + 0 y are not exact copies for every input).  Lane 0 is always such a lane.
            if (chead && src < 0) carry_load_mean<MODEL, JAC>(st, CA.in + w * CD, A.write_jac != 0);
            // Row N - 1 repeats the last row of the window's last lane that integrated anything, so that lane's walked state is
            // what carry_out must hold (the scanned total differs from it in the last bits); none: lane 0 holds the carried /
            // zero state untouched.  With per = ceil(N / L) trailing lanes may own no row at all: they never count as moved.
            const unsigned long long mine = moved & ((L >= 64 ? ~0ull : ((1ull << L) - 1ull)) << (grp * L));
            owner = mine ? 63 - __builtin_clzll(mine) : grp * L;
        }
    }
    if constexpr (CARRY) { if (cbad) mean_poison(st); }

    s_rowbase[lane] = w * (long long)A.N + r0;
    s_lo[lane] = lead;
    s_hi[lane] = nrows;
    const bool wm = A.write_means != 0;
    auto stage = [&](int tt, const RunRow &r) {
        sDT[lane * P1 + tt] = r.DT;
        double *a = sAl + lane * P3 + tt * 3, *b = sBe + lane * P3 + tt * 3, *c = sQ + lane * P4 + tt * 4;
        a[0] = r.alpha.x; a[1] = r.alpha.y; a[2] = r.alpha.z;
        b[0] = r.beta.x; b[1] = r.beta.y; b[2] = r.beta.z;
        c[0] = r.q.x; c[1] = r.q.y; c[2] = r.q.z; c[3] = r.q.w;
    };
    auto flush = [&](int tb) {
        __syncthreads();
        if (A.out.DT) run_flush<1, P1>(sDT, A.out.DT, s_rowbase, s_lo, s_hi, tb, lane);
        if (A.out.alpha) run_flush<3, P3>(sAl, A.out.alpha, s_rowbase, s_lo, s_hi, tb, lane);
        if (A.out.beta) run_flush<3, P3>(sBe, A.out.beta, s_rowbase, s_lo, s_hi, tb, lane);
        if (A.out.q) run_flush<4, P4>(sQ, A.out.q, s_rowbase, s_lo, s_hi, tb, lane);
        __syncthreads();
    };
    auto store_jac = [&](long long row, const MeanState<JAC> &s) {
        if (A.out.J_q) stm3_cm(A.out.J_q + row * 9, s.Jq);
        if (A.out.J_a) stm3_cm(A.out.J_a + row * 9, s.Ja);
        if (A.out.J_b) stm3_cm(A.out.J_b + row * 9, s.Jb);
        if (A.out.H_a) stm3_cm(A.out.H_a + row * 9, s.Ha);
        if (A.out.H_b) stm3_cm(A.out.H_b + row * 9, s.Hb);
    };
    const long long row0 = w * (long long)A.N + r0;

    // ---- the walk: one row per interval
    RunRow last;
    {
        double pk[7], nx[7];
        {
            const double *a = knot(r0), *b = knot(r0 + 1);
#pragma unroll
            for (int i = 0; i < 7; i++) { pk[i] = a[i]; nx[i] = b[i]; }
            if constexpr (CUT) { patch(pk, r0); patch(nx, r0 + 1); }
        }
        for (int tb = 0; tb < per; tb += T) {
            const int te = min(T, per - tb);
#pragma unroll 1
            for (int tt = 0; tt < te; ++tt) {
                const int t = tb + tt;
                double q[7];
#pragma unroll
                for (int i = 0; i < 7; i++) q[i] = nx[i];
                {
                    const double *b = knot(r0 + t + 2);
#pragma unroll
                    for (int i = 0; i < 7; i++) nx[i] = b[i];
                    if constexpr (CUT) patch(nx, r0 + t + 2);
                }
                mean_step<MODEL, JAC, AVG>(st, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                           mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, gk, t < nrows);
#pragma unroll
                for (int i = 0; i < 7; i++) pk[i] = q[i];
                last.DT = st.DT; last.alpha = st.alpha; last.beta = st.beta; last.q = rot_2_quat(st.R);
                if constexpr (CARRY) {   // (rot_2_quat of a NaN matrix is not all NaN)
                    if (cbad) last.q.x = last.q.y = last.q.z = last.q.w = __builtin_nan("");
                }
                if (wm) stage(tt, last);
                if constexpr (JAC) {
                    if (A.write_jac && t >= lead && t < nrows) store_jac(row0 + t, st);
                }
            }
            if (wm) flush(tb);
        }
    }

    // ---- the record the window is left in: the walked state of the lane that owns the state of row N - 1
    if constexpr (CARRY) {
        if (valid && lane == owner)
            carry_store_mean<MODEL, JAC>(CA.out + w * CD, st, true, cbad ? __builtin_nan("") : (double)CA.tag_out);
    }

    // ---- the fix-up: held-back rows repeat the last row of lane `src`
    if constexpr (MULTI) {
        if (__any(lead > 0)) {
            const int sl = max(src, 0);
            RunRow y;
            y.DT = __shfl(last.DT, sl);
            y.alpha = mk(__shfl(last.alpha.x, sl), __shfl(last.alpha.y, sl), __shfl(last.alpha.z, sl));
            y.beta = mk(__shfl(last.beta.x, sl), __shfl(last.beta.y, sl), __shfl(last.beta.z, sl));
            y.q.x = __shfl(last.q.x, sl); y.q.y = __shfl(last.q.y, sl); y.q.z = __shfl(last.q.z, sl); y.q.w = __shfl(last.q.w, sl);
            MeanState<JAC> ys;
            if constexpr (JAC) {
                ys.Jq = run_shfl(st.Jq, sl); ys.Ja = run_shfl(st.Ja, sl); ys.Jb = run_shfl(st.Jb, sl);
                ys.Ha = run_shfl(st.Ha, sl); ys.Hb = run_shfl(st.Hb, sl);
            }
            __syncthreads();
            s_lo[lane] = 0;
            s_hi[lane] = lead;
            const int maxlead = __builtin_amdgcn_readfirstlane(wave_max(lead));
            for (int tb = 0; tb < maxlead; tb += T) {
                if (wm) {
#pragma unroll 1
                    for (int tt = 0; tt < T; ++tt) stage(tt, y);
                    flush(tb);
                }
                if constexpr (JAC) {
                    if (A.write_jac)
                        for (int t = tb; t < min(tb + T, lead); ++t) store_jac(row0 + t, ys);
                }
            }
        }
    }
