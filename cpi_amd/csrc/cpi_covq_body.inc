// cpi_covq_body.inc -- the statements of the covariance query body (described in cpi_covq_body.hpp), pasted into the three kernels
// over it.  Expects: the template parameters MODEL and AVG, constexpr bool OPEN, the locator type Loc, and the arguments A
// (QueryArgs or StreamQueryArgs), QueryCovNoise NZ and QueryBase B.
    static_assert(!(AVG && MODEL == 1), "with the reading held, model 1's averaging is the identity (x + x) * 0.5");
    typedef CovDims<MODEL> D;
    constexpr int GROUP = D::GROUP;   // lanes per query
    constexpr int G = 64 / GROUP;     // queries per wavefront
    constexpr int EP = EXCH_PITCH;
    constexpr int IRD = IrPitch<MODEL>::V;
    constexpr int R0 = 10;            // pitch of a group's start rotation (9 doubles, rows kept 16-B aligned)
    __shared__ __attribute__((aligned(16))) double irs[G * IRD];               // the interval record of each group
    __shared__ __attribute__((aligned(256))) double exch[exch_doubles(G)];   // transpose exchange (placement: cpi_math.hpp)
    __shared__ __attribute__((aligned(16))) double r0s[G * R0];                // rotation at the start of the interval

    const int lane = threadIdx.x;
    const int g = lane / GROUP, j = lane % GROUP;
    const long long q0 = (long long)blockIdx.x * G;
    const bool valid = q0 + g < A.Q;
    const long long k = min(q0 + g, A.Q - 1);        // groups past the last query redo it and store nothing
    const double q4[4] = { NZ.q4[0], NZ.q4[1], NZ.q4[2], NZ.q4[3] };
    const int jl = cov_col_of_lane<MODEL>(j);
    const int jj = (jl < D::NPCOL) ? jl : D::NCOL;                  // column owned by this lane; NCOL = idle
    const int cs = (MODEL == 2 && jj >= 15 && jj < D::NPCOL) ? jj - 15 : jj;   // the column of the 15 x 15 row it starts from
    CovLane<MODEL> Ln;
    cov_init(Ln, jj, q4);

    const double tq = A.qtime[k];
    const QueryAt at = Loc::find(A, k, tq);
    const long long w = at.w;
    const int n = at.n, i = at.i;
    const double *kt = at.kt;
    Loc::note_window(A, k, at, valid && j == 0);

    // ---- the base row's quaternion and this lane's column of S (knot i is in flight with them)
    const bool has = OPEN || i > 0;
    const bool fromb = OPEN && i == 0;               // the state before knot 0: the base row
    double S[D::NR];
    Q4 bq;
    bq.x = 0; bq.y = 0; bq.z = 0; bq.w = 1;
    if (OPEN || A.N > 0) {                           // wave-uniform.  N == 0: rows is not read, S is zero / the base row
        const long long row = fromb ? w * (long long)B.N + (B.N - 1) : w * (long long)A.N + max(i - 1, 0);
        const Q4 rq = ldq4((fromb ? B.rows.q : A.rows.q) + row * 4);
        const int c = min(cs, 14);                   // idle lanes load column 14 and drop it
        const bool own = has && cs < 15;
        const double *rP = fromb ? B.rows.P : A.rows.P, *rPs = fromb ? B.rows.P_sym : A.rows.P_sym;
        if (rP) {
            const double *p = rP + row * 225 + c * 15;
#pragma unroll
            for (int r = 0; r < 15; r++) S[r] = own ? p[r] : 0.0;
        } else {
            const double *p = rPs + row * CPI_TRI_DOUBLES;
#pragma unroll
            for (int r = 0; r < 15; r++) S[r] = own ? p[(r <= c) ? r + c * (c + 1) / 2 : c + r * (r + 1) / 2] : 0.0;
        }
        if (has) bq = rq;
    } else {
#pragma unroll
        for (int r = 0; r < 15; r++) S[r] = 0.0;
    }
    if (MODEL == 2) {
        constexpr int o = (D::NR >= 18) ? 15 : 0;    // (model 1 never takes this branch)
        S[o] = S[0]; S[o + 1] = S[1]; S[o + 2] = S[2];
    }
#pragma unroll
    for (int r = 0; r < D::NR; r++) Ln.P0[r] = S[r];

    double *ex_g = exch + g * EXCH_WIN;
    const double *ex_row = exch + (cov_row_off<MODEL>(G, g, jj) & ~1);   // 16-B aligned rows, said explicitly (cov_body)
    const int hoff = cov_h_offset<MODEL>(jj);        // ZERO: no lane owns a theta_klin transition column
    double *ir = irs + g * IRD;
    double *r0 = r0s + g * R0;
    for (int e = lane; e < exch_doubles(G); e += 64) exch[e] = 0.0;
    __syncthreads();
    cov_exch_init<MODEL>(exch, G, jj, q4);

    // ---- the record of the partial interval [t_i, t_q] with reading i held; no step: dt = 0, an exact no-op of the recursion
    const bool step = (i < n) && (tq > kt[0]);
    if (j == 0) {
        const M3 R_old = quat_2_Rot(bq);             // [0 0 0 1] gives the identity exactly
        const V3 bw = ldv3(A.lin + w * 6), ba = ldv3(A.lin + w * 6 + 3);
        V3 gk = mk(0, 0, 0);
        if (MODEL == 2) gk = mul(quat_2_Rot(ldq4(A.qk + w * 4)), mk(A.grav[0], A.grav[1], A.grav[2]));
        const V3 wi = mk(kt[1], kt[2], kt[3]), ai = mk(kt[4], kt[5], kt[6]);
        const SampleRec r = make_sample_rec<MODEL, AVG>(kt[0], step ? tq : kt[0], wi, ai, wi, ai, bw, ba);
        finish_interval<MODEL, AVG>(r, R_old, gk, ir);
        rec_put_mat(r0, 0, R_old);
    }
    wave_lds_fence();

    // ---- one interval of cov_body's phase C: F x is lane-local, P F^T arrives through the exchange rows
    cov_begin<MODEL>(Ln, ir, hoff);
    M3 Rs = rec_mat(r0, 0);
#pragma unroll
    for (int stg = 0; stg < 4; ++stg) {
        double M[9];
        if (stg == 1 || stg == 3) Rs = cov_stage_rotation<MODEL>(ir, stg);   // stages 1 and 2 share R_mid
        cov_stage_M(Ln, stg, Rs, M);
        if (jj < D::NPCOL) {
#pragma unroll
            for (int rr = 0; rr < CovExchRows<MODEL>::V; rr++) ex_g[rr * EP + exch_pos<MODEL>(jj)] = M[rr];
        }
        wave_lds_fence();   // a wave's DS instructions execute in issue order: only the compiler must not reorder them
        if constexpr (CovPBySymmetry<MODEL>::V) {
            double mt[D::NR];
            const double *Xs = cov_stage_X(Ln, stg);
#pragma unroll
            for (int r = 0; r < D::NR; r++)
                mt[r] = (MODEL == 1) ? dpp_shr6_bank3(ex_row[exch_pos<MODEL>(r)], Xs[r])
                                     : dpp_shr6_bank3_oddrows(ex_row[exch_pos<MODEL>(r)], Xs[r]);
            cov_stage_finish_regs(Ln, stg, M, mt);
        } else {
            cov_stage_finish(Ln, stg, M, ex_row);
        }
    }

    // ---- columns jj < 15: the stepped column, or the gathered one bit for bit
    if (!valid || jj >= 15) return;
    const bool bad = (tq != tq) || (OPEN && bq.x != bq.x) || at.none;
    double v[15];
#pragma unroll
    for (int r = 0; r < 15; r++) v[r] = bad ? __builtin_nan("") : (step ? Ln.P0[r] : S[r]);
    if (A.out.P) {
        double *p = A.out.P + k * 225 + jj * 15;
#pragma unroll
        for (int r = 0; r < 15; r++) p[r] = v[r];
    }
    if (A.out.P_sym) {   // rows 0 .. jj of the same column: the packed upper triangle (CPI_TRI_INDEX)
        double *p = A.out.P_sym + k * CPI_TRI_DOUBLES + jj * (jj + 1) / 2;
#pragma unroll
        for (int r = 0; r < 15; r++) if (r <= jj) p[r] = v[r];
    }
