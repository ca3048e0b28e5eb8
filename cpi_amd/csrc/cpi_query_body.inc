// cpi_query_body.inc -- body of cpi_query_kernel (cpi_query_kernels.hpp) and cpi_query_open_kernel
// (cpi_query_open_kernels.hpp).  Expects: the template
// parameters MODEL, JAC, AVG, the arguments QueryArgs A and QueryBase B, constexpr bool OPEN.
    static_assert(!(JAC && MODEL == 2), "model 2's Jacobians are read out of the state transition matrix");
    static_assert(!(AVG && MODEL == 1), "with the reading held, model 1's averaging is the identity (x + x) * 0.5");
    __shared__ __attribute__((aligned(16))) double sOut[64 * QRY_PITCH];
    const int lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * 64;
    const int nq = (int)min(64ll, A.Q - q0);
    const long long k = q0 + min(lane, nq - 1);      // lanes past the last query redo it and store nothing
    const long long w = min(max((long long)A.qwin[k], 0ll), A.W - 1);
    const double tq = A.qtime[k];
    const int n = A.count ? min(max(A.count[w], 0), A.N) : A.N;
    const double *kn = A.knots + (A.first ? A.first[w] : w * (long long)(A.N + 1)) * 7;

    // ---- the interval: sum of the steps = 2^trips - 1 >= N, so every index of [0, n] is reachable
    int i = 0;
    for (int s = A.trips - 1; s >= 0; --s) {
        const int probe = i + (1 << s);
        const double t = kn[min(probe, n) * 7];
        i = (probe <= n && t <= tq) ? probe : i;
    }

    // ---- knot i and the base row, in flight together
    double kt[7];
#pragma unroll
    for (int j = 0; j < 7; j++) kt[j] = kn[i * 7 + j];
    const bool has = OPEN || i > 0;
    const bool fromb = OPEN && i == 0;               // the state before knot 0: the base row
    const cpi_outputs &R = A.rows, &RB = B.rows;
    MeanState<JAC> st;
    mean_init(st);
    double bDT = 0.0;
    V3 bal = mk(0, 0, 0), bbe = mk(0, 0, 0);
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    if (OPEN || A.N > 0) {                           // wave-uniform.  N == 0: rows is not read, every query is the zero state / the base row
        const long long row = fromb ? w * (long long)B.N + (B.N - 1) : w * (long long)A.N + max(i - 1, 0);
        const double rDT = (fromb ? RB.DT : R.DT)[row];
        const V3 ral = ldv3((fromb ? RB.alpha : R.alpha) + row * 3), rbe = ldv3((fromb ? RB.beta : R.beta) + row * 3);
        const Q4 rq = ldq4((fromb ? RB.q : R.q) + row * 4);
        if (JAC) {
            const M3 rJq = ldm3_cm((fromb ? RB.J_q : R.J_q) + row * 9), rJa = ldm3_cm((fromb ? RB.J_a : R.J_a) + row * 9),
                     rJb = ldm3_cm((fromb ? RB.J_b : R.J_b) + row * 9), rHa = ldm3_cm((fromb ? RB.H_a : R.H_a) + row * 9),
                     rHb = ldm3_cm((fromb ? RB.H_b : R.H_b) + row * 9);
            if (has) { st.Jq = rJq; st.Ja = rJa; st.Jb = rJb; st.Ha = rHa; st.Hb = rHb; }
        }
        if (has) { bDT = rDT; bal = ral; bbe = rbe; bq = rq; }
    }
    st.DT = bDT; st.alpha = bal; st.beta = bbe;
    st.R = quat_2_Rot(bq);                           // [0 0 0 1] gives the identity exactly

    const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
    V3 gk = mk(0, 0, 0);
    if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));

    // ---- the partial interval [t_i, t_q] with reading i held; inactive: an exact no-op (JAC: the state is not touched at all)
    const bool step = (i < n) && (tq > kt[0]);
    const V3 wi = mk(kt[1], kt[2], kt[3]), ai = mk(kt[4], kt[5], kt[6]);
    mean_step<MODEL, JAC, AVG>(st, kt[0], tq, wi, ai, wi, ai, bw, ba, gk, step);
    const Q4 sq = rot_2_quat(st.R);

    const bool bad = (tq != tq) || (OPEN && bq.x != bq.x);
    const double qnan = __builtin_nan("");
    auto pick = [&](double stepped, double base) { return bad ? qnan : (step ? stepped : base); };
    {
        double *d = sOut + lane * QRY_PITCH;
        d[0] = pick(st.DT, bDT);
        d[1] = pick(st.alpha.x, bal.x); d[2] = pick(st.alpha.y, bal.y); d[3] = pick(st.alpha.z, bal.z);
        d[4] = pick(st.beta.x, bbe.x); d[5] = pick(st.beta.y, bbe.y); d[6] = pick(st.beta.z, bbe.z);
        d[7] = pick(sq.x, bq.x); d[8] = pick(sq.y, bq.y); d[9] = pick(sq.z, bq.z); d[10] = pick(sq.w, bq.w);
    }
    wave_lds_fence();
    if (A.out.DT) query_flush<1>(sOut, 0, A.out.DT, q0, nq, lane);
    if (A.out.alpha) query_flush<3>(sOut, 1, A.out.alpha, q0, nq, lane);
    if (A.out.beta) query_flush<3>(sOut, 4, A.out.beta, q0, nq, lane);
    if (A.out.q) query_flush<4>(sOut, 7, A.out.q, q0, nq, lane);
    if (JAC) {
        auto put = [&](double *field, const M3 &J) {
            if (!field) return;                      // wave-uniform
            wave_lds_fence();                        // in-order DS: the previous flush has read the area
            double *d = sOut + lane * QRY_PITCH;
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int r = 0; r < 3; r++) d[c * 3 + r] = bad ? qnan : J.m[r][c];
            wave_lds_fence();
            query_flush<9>(sOut, 0, field, q0, nq, lane);
        };
        put(A.out.J_q, st.Jq); put(A.out.J_a, st.Ja); put(A.out.J_b, st.Jb); put(A.out.H_a, st.Ha); put(A.out.H_b, st.Hb);
    }
