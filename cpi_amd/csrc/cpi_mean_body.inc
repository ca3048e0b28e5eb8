// cpi_mean_body.inc -- the body of cpi_mean_kernel and cpi_mean_carry_kernel (cpi_mean_kernels.hpp), included inside both.
// Shared as text rather than through a device function so that the batch kernels compile to exactly the code they had
// before the carry path existed (a body function changes their scalar register allocation).  In scope where it is
// included: MODEL, JAC, AVG, L, CUT, BIG, CARRY, the kernel arguments A (PreArgs), CA (CarryArgs) and RA (RunArgs; CUT = 3 only),
// and the preloaded leading parameters knots, lin, W, N, first, count (CPI_MEAN_LEAD_PARAMS), read INSTEAD of their copies in A.
    static_assert(!BIG || (L == 1 && !JAC), "BIG: one lane per window, mean-only");
    constexpr int WPB = 64 / L;       // windows per wavefront
    // knots staged per lane per chunk: measured on MI355X -- 2 when a lane has several intervals (L <= 8; 20 k x 50 with
    // L = 3: 19.7 -> 18.4 us, 30 k with L = 2: 27.4 -> 24.8 us, 15 k with L = 4: 16.0 -> 15.3 us, 10 k with L = 6:
    // 12.5 -> 11.8 us once the padded second step of an odd last chunk is skipped), 1 when a wave is latency-bound
    // with few intervals per lane (L >= 12: 5 k windows 9.55 vs 9.65 us, 2.5 k 7.7 vs 8.0 us); 3 for BIG (above)
    constexpr int C = BIG ? CPI_MEAN_BIG_C : ((L <= 8 && !JAC) ? CPI_MEAN_C : 1);
    constexpr int SEGD = 7 * C;       // doubles per lane per chunk
    constexpr int PITCH = (SEGD & 1) ? SEGD : SEGD + 1;   // odd pitch (15, 21 doubles): a half-wave's ds_read_b64 hit 32 distinct even banks
    __shared__ double tile[64 * PITCH];
    __shared__ unsigned long long segdesc[64];  // per lane-segment: (first double of the segment << 16) | intervals

    const int lane = threadIdx.x;
    const int grp = lane / L, l = lane - grp * L;
    long long w = (long long)blockIdx.x * WPB + grp;
    const bool valid = (w < W) && (grp < WPB);   // L not a power of two leaves 64 - WPB*L idle lanes
    if (grp >= WPB) w = (long long)blockIdx.x * WPB;   // idle lanes shadow the block's first window (stays near the block)
    if (w >= W) w = W - 1;
    constexpr bool cut = CUT != 0;
    int n;
    long long k0;
    // Windows cut out of a stream in flight: the window's first knot takes the stamp t_start, and a partial tail interval
    // has NO knot in memory -- it is the last real knot's reading held until t_end.  The lane that owns the tail fetches one
    // knot less and builds that knot from its predecessor when it gets there.
    double t_start = 0.0, t_end = 0.0;
    bool tail = false;
    if constexpr (CUT == 3) {
        // many runs: the run of the wavefront's first window, by a bisection on wave-uniform values (scalar loads); when the
        // run also owns the wavefront's last window -- every wavefront but the few that straddle a run boundary -- that is
        // every lane's run, otherwise each lane bisects for its own.  Then the CUT = 2 arithmetic on the run's readings.
        const long long wb = (long long)blockIdx.x * WPB, we = min(wb + WPB, W) - 1;
        int r = run_of(RA, wb);
        if (!(RA.uoff[r + 1] > we)) r = run_of(RA, w);
        const RunWindow c = run_window(knots, A.K, A.update, RA, r, w);
        if (valid && l == 0) A.count_out[w] = c.cnt;                     // the TRUE count (cpi_stream_counts)
        k0 = c.k0;
        n = min(c.cnt, N);
        t_start = c.t_start;
        t_end = A.update[w];
        tail = c.tail && c.cnt <= N;                                   // a truncated window has lost its tail
    } else if constexpr (CUT == 2) {
        // the arithmetic of cpi_cut_windows_kernel (GraphSolver_IMU.cpp:50-69 as a closed form), per lane, in registers
        const double ts0 = knots[0], ts1 = knots[(A.K - 1) * 7];
        const double T = A.update[w], Tp = A.update[w > 0 ? w - 1 : 0];
        double stT, stP;
        const long long cT = knots_not_after_near(knots, A.K, ts0, ts1, T, stT);
        const long long cP = knots_not_after_near(knots, A.K, ts0, ts1, Tp, stP);
        const long long fp = (w > 0) ? max(cP - 1, 0ll) : 0ll;
        t_start = (w > 0) ? fmax(Tp, ts0) : ts0;
        const long long fu = max(max(cT - 1, 0ll), fp);
        const int m = (int)min(fu - fp, (long long)0x3fffffff);
        const double front_t = (m > 0) ? stT : t_start;                  // m > 0: fu = cT - 1 > 0, whose stamp the search returned
        const bool tl = (T - front_t) > 0;
        const int cnt = m + (tl ? 1 : 0);
        if (valid && l == 0) A.count_out[w] = cnt;                       // the TRUE count (cpi_stream_counts)
        k0 = fp;
        n = min(cnt, N);
        t_end = T;
        tail = tl && cnt <= N;                                         // a truncated window has lost its tail
    } else {
        n = count ? min(max(count[w], 0), N) : N;   // a count outside [0, N] must not corrupt the packed descriptors
        k0 = first ? first[w] : w * (long long)(N + 1);
        if constexpr (CUT == 1) {
            t_start = A.tstart[w]; t_end = A.tend[w];
            tail = (t_end == t_end) && (count[w] <= N);              // NaN = no tail; a truncated window has lost it
        }
    }
    const int per = (n + L - 1) / L;
    const int s0 = min(n, l * per), s1 = min(n, s0 + per);
    const int len = s1 - s0;
    const int maxlen = __builtin_amdgcn_readfirstlane(wave_max(len));   // wave-uniform: loop control stays scalar
    const bool tailseg = cut && tail && (s1 == n) && (len > 0);
    const int len_f = len - (tailseg ? 1 : 0);                          // knots after the segment's first that exist in memory
    // First knot of the segment IN MEMORY.  Knot s0 always exists (a window owns count + 1 knots) -- except the virtual tail
    // knot, which only an EMPTY trailing segment (s0 == n, lanes beyond ceil(n / per)) can start on: nothing of such a segment is
    // ever consumed, but its first knot is still fetched (pk below, and the staging path re-reads a never-valid element's base
    // knot), and when the window ends on the stream's last reading (update time past the last stamp) knot k0 + n lies 56 bytes
    // behind the caller's buffer -- unmapped memory, or NaN bits that reach the state through 0 * NaN on the dt = 0 steps with
    // imu_avg.  Such a segment is based on the last real knot instead.
    const int sb = (cut && tail && s0 == n && n > 0) ? s0 - 1 : s0;

    // (Deriving the descriptors of a dense layout arithmetically instead of through LDS was measured: +0.35 us per
    // 13 us launch -- the 64-bit integer arithmetic costs more than the shuffle reduction and the LDS round trip.)
    segdesc[lane] = ((unsigned long long)((k0 + sb) * 7) << 16) | (unsigned long long)(unsigned)len_f;

    const V3 bw = ldv3(lin + w * 6), ba = ldv3(lin + w * 6 + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));

    double pk[7];
    {
        const double *kb = knots + (k0 + sb) * 7;
#pragma unroll
        for (int i = 0; i < 7; i++) pk[i] = kb[i];
        if (cut && s0 == 0) pk[0] = t_start;
    }
    MeanState<JAC> st;
    mean_init(st);
    constexpr int CD = carry::doubles(MODEL);
    bool cbad = false;   // CARRY: the record does not hold what this call continues (its outputs become NaN)
    if constexpr (CARRY) {
        if (CA.in) {
            const double *ci = CA.in + w * CD;
            cbad = !carry_tag_ok(ci[carry::TAG], CA.need);
            if (l == 0 && !cbad) carry_load_mean<MODEL, JAC>(st, ci, A.write_jac != 0);
        }
    }
    // model 2, mean-only, several lanes per window: a lane integrates its segment from the raw specific force and
    // accumulates the segment's gravity response (cpi_math.hpp: mean_step_v2seg); gravity is applied after the tree
    constexpr bool GSEG = (MODEL == 2) && !JAC && (L > 1);
    GravAcc ga;
    if (GSEG) grav_init(ga);
    __syncthreads();

    // Analytic-Jacobian variant of model 1, one lane per window (large batches): the recursion is bound by registers
    // (61 doubles of state + the per-interval 3x3 temporaries), not by HBM, so it streams its knots straight into
    // registers, one interval ahead, instead of through the coalescing LDS stage -- that frees the stage's address /
    // staging registers and lets two wavefronts share a SIMD (256 registers + 36 B of scratch each).  Measured inside
    // "V1 full" (covariance kernel + this one): 1.405 -> 1.376 ms per 100 k windows, 13.25 -> 13.10 ms per 1 M.  With
    // several lanes per window (small, latency-bound batches) it loses (10 k windows: 192 -> 205 us), so those keep the stage.
    constexpr bool DIRECT = JAC && (MODEL == 1) && (L == 1);
    if constexpr (DIRECT) {
        const double *kp = knots + (k0 + s0) * 7;
        double nx[7];
        {
            const double *kb = kp + 7 * min(1, len_f);
#pragma unroll
            for (int i = 0; i < 7; i++) nx[i] = kb[i];
        }
        for (int sidx = 0; sidx < maxlen; ++sidx) {
            double q[7];
#pragma unroll
            for (int i = 0; i < 7; i++) q[i] = nx[i];
            {
                const double *kb = kp + 7 * min(sidx + 2, len_f);   // knot s0 + len_f is the segment's last one in memory: always valid
#pragma unroll
                for (int i = 0; i < 7; i++) nx[i] = kb[i];
            }
            if constexpr (cut) {      // the tail knot: the predecessor's reading under the update time
                const bool here = tailseg && sidx == len - 1;
                q[0] = here ? t_end : q[0];
#pragma unroll
                for (int i = 1; i < 7; i++) q[i] = here ? pk[i] : q[i];
            }
            mean_step<MODEL, JAC, AVG>(st, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                       mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, gk, sidx < len);
#pragma unroll
            for (int i = 0; i < 7; i++) pk[i] = q[i];
        }
    } else {
    // Tile element idx = e*64 + lane belongs to segment idx / SEGD at offset idx % SEGD, so consecutive
    // lanes read consecutive doubles of (mostly) one segment: coalesced.  Everything that does not depend
    // on the chunk index is hoisted: per staged element a lane keeps one pointer and the last chunk for
    // which its knot exists (later chunks re-read that knot; the value is never consumed), so the hot loop
    // spends ~3 VALU per element on addressing and no load is ever out of bounds.
    double stage[SEGD];
    const double *sptr[SEGD];   // !BIG
    unsigned voff[SEGD];   // byte offset of the element from blk0: the fast path's constant (dense layouts, uniform streams); BIG: of both paths
    int smax[SEGD];
    int tofs[SEGD];             // !BIG (BIG: the tile is flat, element e of lane i at 64 e + i)
    const double *blk0 = knots + (long long)blockIdx.x * WPB * (long long)(N + 1) * 7;   // wave-uniform (dense layout)
    bool fast_stream = false;
    const long long b = k0 + sb;
    long long b0 = 0;
    if constexpr (BIG) {
        // the wavefront's lowest first knot (stream windows out of time order may start below lane 0's)
        const long long bf = readfirstlane64(b);
        b0 = bf - (long long)wave_max((int)min(max(bf - b, 0ll), 0x7fffffffll));
        blk0 = knots + b0 * 7;
    }
    if constexpr (cut) {
        // The stream entry's twin of the dense layout's fast path below: "wave-uniform base + chunk stride in SGPRs + constant
        // 32-bit lane offsets" is valid for a stream whenever (a) every lane-segment of the wavefront has the same length --
        // then no lane ever CONSUMES a knot behind its own segment (the padded step of an odd last chunk is skipped, a tail
        // knot is replaced by a select), so reading on is harmless whatever those knots hold --, (b) the segments lie within
        // 2^30 bytes above the first one and (c) the furthest read stays inside the stream (PreArgs::K).  A uniform update
        // grid satisfies all three for every wavefront but the last; ragged wavefronts keep the per-element path.
        if constexpr (!BIG) b0 = readfirstlane64(b);
        const int nch = (maxlen + C - 1) / C;
        const bool ok = (A.K > 0) && (len == maxlen) && (b >= b0) && (b - b0 < (1ll << 24)) && (b + (long long)nch * C <= A.K - 1);
        fast_stream = __all(ok);
        if (fast_stream) blk0 = knots + b0 * 7;
    }
    {
        // (Issuing all SEGD descriptor reads before using the first -- one LDS round trip instead of SEGD dependent ones,
        // which hipcc keeps in program order with an s_waitcnt after each -- was measured: 12.55 vs 12.33 us per launch
        // at 10 k windows, i.e. slower; the wavefronts wait for the first HBM burst either way and start less staggered.)
        int seg = lane / SEGD, off = lane - seg * SEGD;
#pragma unroll
        for (int e = 0; e < SEGD; ++e) {
            const unsigned long long d = segdesc[seg];
            const long long base = (long long)(d >> 16);
            const int slen = (int)(d & 0xffffULL);
            const int kn = off / 7;                       // knot (1 + kn) of chunk 0
            const bool ok = slen >= 1 + kn;
            if constexpr (BIG) {
                voff[e] = (unsigned)((base - b0 * 7 + (ok ? 7 + off : off - 7 * kn)) * 8);   // < 2^32: the launcher's admission rule
            } else {
                sptr[e] = knots + base + (ok ? 7 + off : off - 7 * kn);
                voff[e] = (unsigned)((sptr[e] - blk0) * 8);   // only used when safe_overread (then 0 <= offset < 2^32)
                tofs[e] = seg * PITCH + off;
            }
            smax[e] = ok ? (slen - 1 - kn) / C : 0;       // never-valid elements keep re-reading knot 0
            off += 64 % SEGD; seg += 64 / SEGD;   // idx advances by 64 per staged element
            if (off >= SEGD) { off -= SEGD; seg += 1; }
        }
    }
    // Dense layout, not one of the last waves: reading a few knots past a short segment's end stays inside
    // the knot array, so every chunk is "block base + chunk stride (scalar) + constant lane offset".
    // (Not with per-window counts: the knots behind a short window's last interval belong to the caller's dense array and
    // may never have been written -- a NaN there would reach the state through 0 * NaN on the inactive steps.  The
    // per-element path below stops at the segment's end and re-reads its last, valid knot instead.)
    const bool safe_overread = cut ? fast_stream
                                   : ((first == nullptr) && (count == nullptr) && ((long long)(blockIdx.x + 1) * WPB + 2 < W));
    auto issue = [&](int it) {
        if (safe_overread) {
            // scalar base (advanced by SALU) + constant 32-bit lane offsets: no vector arithmetic per element
            const char *cb = reinterpret_cast<const char *>(blk0) + (long long)it * (SEGD * 8);
#pragma unroll
            for (int e = 0; e < SEGD; ++e) {
                asm volatile("" : "+v"(voff[e]));   // keeps the zero-extension next to the load: `global_load v, v_off32, s[base]`
                stage[e] = *reinterpret_cast<const double *>(cb + voff[e]);
            }
        } else if constexpr (BIG) {
            const char *cb = reinterpret_cast<const char *>(blk0);
#pragma unroll
            for (int e = 0; e < SEGD; ++e) {
                asm volatile("" : "+v"(voff[e]));
                stage[e] = *reinterpret_cast<const double *>(cb + voff[e]);
                voff[e] += (it < smax[e]) ? (unsigned)(SEGD * 8) : 0u;
            }
        } else {
#pragma unroll
            for (int e = 0; e < SEGD; ++e) { stage[e] = *sptr[e]; sptr[e] += (it < smax[e]) ? SEGD : 0; }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int e = 0; e < SEGD; ++e) {
            if constexpr (BIG) tile[e * 64 + lane] = stage[e]; else tile[tofs[e]] = stage[e];
        }
    };

    // One chunk ahead: the HBM round trip of chunk it+1 overlaps the FP64 work of chunk it.  Measured alternatives:
    // a TRUE two-chunk pipeline (two register stages, every path issuing the same loads so that hipcc emits the partial
    // wait s_waitcnt vmcnt(14) -- one conditional issue in the loop and it drains the queue with vmcnt(0)) is 8 % slower
    // at 10 k windows x 50 (13.5 vs 12.5 us: the first chunk's data queues behind the second's) and 5 % slower at 1 M;
    // a double-buffered LDS tile with the next chunk read back into registers during the integration: +2 %.
    // Per-wavefront time stamps explain why: with 1000 wavefronts in flight a chunk is 3.6 MB and takes 0.89 us
    // (0.74 us with 625 wavefronts, 1.2 us with 2000) -- the loop streams at ~4 TB/s and is paced by the memory
    // system, not by the latency of one wavefront's accesses.
    // Stream windows on a uniform update grid: EVERY lane-segment of the wavefront ends in its window's tail interval and all
    // are equally long -- the tail step is then peeled off behind the loop and the loop carries no per-step selects (14
    // v_cndmask per interval of ~300 VALU; measured on the 1 M x 51 stream: 724 -> see DESIGN.md 3.1b).  Wave-uniform.
    const bool utail = cut && __all(tailseg && len == maxlen);
    const int nsteps = utail ? maxlen - 1 : maxlen;
    const int nchunks = (nsteps + C - 1) / C;
    if (nchunks > 0) issue(0);
    for (int it = 0; it < nchunks; ++it) {
        commit();
        __syncthreads();
        if (it + 1 < nchunks) issue(it + 1);
#pragma unroll   // C <= 2: the two steps of a chunk share one basic block (no knot copy between them)
        for (int c = 0; c < C; ++c) {
            const int s = it * C + c;
            if (C > 1 && s >= nsteps) break;   // wave-uniform: no lane has this interval (odd longest segment)
            const double *nk = &tile[lane * PITCH + c * 7];
            double q[7];
#pragma unroll
            for (int i = 0; i < 7; i++) q[i] = nk[i];
            if constexpr (cut) {      // the tail knot: the predecessor's reading under the update time
                if (!utail) {
                    const bool here = tailseg && s == len - 1;
                    q[0] = here ? t_end : q[0];
#pragma unroll
                    for (int i = 1; i < 7; i++) q[i] = here ? pk[i] : q[i];
                }
            }
            if constexpr (GSEG)
                mean_step_v2seg<AVG>(st, ga, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                     mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, s < len);
            else
                mean_step<MODEL, JAC, AVG>(st, pk[0], q[0], mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                           mk(q[1], q[2], q[3]), mk(q[4], q[5], q[6]), bw, ba, gk, s < len);
#pragma unroll
            for (int i = 0; i < 7; i++) pk[i] = q[i];
        }
        __syncthreads();
    }
    if constexpr (cut) {
        if (utail) {   // the peeled tail interval [stamp of the last real knot, t_end], that knot's reading held
            if constexpr (GSEG)
                mean_step_v2seg<AVG>(st, ga, pk[0], t_end, mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                     mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]), bw, ba, true);
            else
                mean_step<MODEL, JAC, AVG>(st, pk[0], t_end, mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]),
                                           mk(pk[1], pk[2], pk[3]), mk(pk[4], pk[5], pk[6]), bw, ba, gk, true);
        }
    }

    }   // !DIRECT

    // order-preserving composition tree over the L lanes of a window (earlier = lower lane)
#pragma unroll
    for (int stp = 1; stp < L; stp <<= 1) {
        MeanState<JAC> B = shfl_down(st, stp);
        GravAcc gB;
        if constexpr (GSEG) gB = shfl_down(ga, stp);
        if ((L & (L - 1)) != 0) {
            // L not a power of two: lane l + stp may belong to the next window -- compose with the identity instead
            if (l + stp >= L) { mean_init(B); if (GSEG) grav_init(gB); }
        }
        if constexpr (GSEG) grav_combine(ga, st, gB, B);   // needs st.R / B.DT before they are composed
        mean_combine(st, B);
    }
    if constexpr (GSEG) grav_apply(st, ga, gk);
    if constexpr (CARRY) { if (cbad) mean_poison(st); }

    if (valid && l == 0) {
        // (Holding write_means and the four pointers in SGPRs from the prologue on takes the kernel-argument loads off the serial
        // tail, where the compiler puts them between the loop's exit and the tree, but costs 7 SGPRs in every mean-only
        // instantiation: not done.)
        if (A.write_means) {
            if (A.out.DT) A.out.DT[w] = st.DT;
            if (A.out.alpha) stv3(A.out.alpha + w * 3, st.alpha);
            if (A.out.beta) stv3(A.out.beta + w * 3, st.beta);
            if (A.out.q) {
                const Q4 q = rot_2_quat(st.R);
                double *p = A.out.q + w * 4;
                p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
            }
        }
        if (JAC && A.write_jac) {
            if (A.out.J_q) stm3_cm(A.out.J_q + w * 9, st.Jq);
            if (A.out.J_a) stm3_cm(A.out.J_a + w * 9, st.Ja);
            if (A.out.J_b) stm3_cm(A.out.J_b + w * 9, st.Jb);
            if (A.out.H_a) stm3_cm(A.out.H_a + w * 9, st.Ha);
            if (A.out.H_b) stm3_cm(A.out.H_b + w * 9, st.Hb);
            if (MODEL == 2) {
                if (A.out.O_a) stm3_cm(A.out.O_a + w * 9, st.Oa);
                if (A.out.O_b) stm3_cm(A.out.O_b + w * 9, st.Ob);
            }
        }
        if constexpr (CARRY) {
            if (cbad && A.write_means && A.out.q) {   // (rot_2_quat of a NaN matrix is not all NaN)
                double *p = A.out.q + w * 4;
                p[0] = p[1] = p[2] = p[3] = __builtin_nan("");
            }
        }
        if constexpr (CARRY)
            carry_store_mean<MODEL, JAC>(CA.out + w * CD, st, CA.own_means != 0, cbad ? __builtin_nan("") : (double)CA.tag_out);
    }
