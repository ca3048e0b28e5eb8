"""A NumPy restatement of cpi_merge_batch (include/cpi_amd.h): consecutive model-1 measurements joined into one.  TEST
INFRASTRUCTURE ONLY: dense 15 x 15 algebra, vectorised over the batch, in float64 or longdouble -- nothing of the kernel's block
sparsity or lane layout.

For A (earlier) followed by B (later), R_X = quat_2_Rot(q_X), error-state order [theta b_g v b_a p]:
    DT = DT_A + DT_B,  R = R_B R_A,  beta = beta_A + R_A^T beta_B,  alpha = alpha_A + beta_A DT_B + R_A^T alpha_B
    J_q = R_B J_q_A + J_q_B,  J_b = J_b_A + R_A^T (J_b_B + [beta_B x] J_q_A),  H_b = H_b_A + R_A^T H_b_B
    J_a = J_a_A + DT_B J_b_A + R_A^T (J_a_B + [alpha_B x] J_q_A),  H_a = H_a_A + DT_B H_b_A + R_A^T H_a_B
    P = Phi~ P_A Phi~^T + T P_B T^T, then 0.5 (P + P^T);  T = blkdiag(I, I, R_A^T, I, R_A^T),  Phi~ = T Phi(B) T^T
and Phi(X) = the identity with (theta,theta) = R_X, (theta,b_g) = -J_q, (v,theta) = -[beta x], (v,b_g) = J_b, (v,b_a) = H_b,
(p,theta) = -[alpha x], (p,b_g) = J_a, (p,v) = DT I, (p,b_a) = H_a.

States are dicts of arrays over a batch: DT [W], alpha / beta [W, 3], R and the five Jacobians [W, 3, 3] ([row][col]), P [W, 15, 15].
Measurement dicts are what the library returns: matrices flat and column-major, q JPL [x y z w].

MUTATIONS (profiles/merge_bench.md): compose(..., mutate=) breaks one term on purpose, so that the tests can show they would see it.

identity_blocks (compose / fold / merge_ref, default True): the (v,v) and (p,p) blocks of Phi~ are I and its (p,v) block DT_B I BY
CONSTRUCTION, as include/cpi_amd.h states and the kernel computes.  The dense triple product T Phi(B) T^T gives R_A^T R_A and
DT_B R_A^T R_A there, which is the same thing only while R_A is orthonormal, i.e. while the operand's quaternion is unit: with
identity_blocks=False the restatement is valid for unit quaternions alone (a q that is unit only to float32 moves its P by 4e-7 to
7.5e-6 relative).  For unit quaternions the two forms agree to rounding (tests/test_merge_cpu.py asserts it).

hard_knots / hard_rows: operands at rates of up to 20 rad/s (joined rotations past 3 rad: all four branches of rot_2_quat) in four
regimes -- as computed, q negated, q unit only to float32, a zero-state row among the operands."""
import numpy as np

MEAN = ("DT", "alpha", "beta", "q")
JAC = ("J_q", "J_a", "J_b", "H_a", "H_b")
MUTATIONS = ("drop_beta_x_Jq", "no_T_on_PB", "wrong_sign_theta_bg")
_TH, _BG, _V, _BA, _P = (slice(3 * i, 3 * i + 3) for i in range(5))


def skew(v):
    """[W, 3] -> [W, 3, 3], skew(v) u = v x u (quat_ops.h:92-98)."""
    z = np.zeros_like(v[:, 0])
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1), np.stack([v[:, 2], z, -v[:, 0]], -1), np.stack([-v[:, 1], v[:, 0], z], -1)], -2)


def quat_2_Rot(q):
    """JPL [W, 4] -> [W, 3, 3] (quat_ops.h:104-109)."""
    v, w = q[:, :3], q[:, 3]
    eye = np.eye(3, dtype=q.dtype)[None]
    return (2 * w * w - 1)[:, None, None] * eye - 2 * w[:, None, None] * skew(v) + 2 * v[:, :, None] * v[:, None, :]


def rot_2_quat(R):
    """[W, 3, 3] -> JPL [W, 4], w >= 0, normalised: the branches of quat_ops.h:45-86."""
    R = np.asarray(R)
    out = np.zeros(R.shape[:1] + (4,), dtype=R.dtype)
    for i, r in enumerate(R):
        T = r[0, 0] + r[1, 1] + r[2, 2]
        q = np.zeros(4, dtype=R.dtype)
        if r[0, 0] >= T and r[0, 0] >= r[1, 1] and r[0, 0] >= r[2, 2]:
            q[0] = np.sqrt((1 + 2 * r[0, 0] - T) / 4)
            q[1], q[2], q[3] = (r[0, 1] + r[1, 0]) / (4 * q[0]), (r[0, 2] + r[2, 0]) / (4 * q[0]), (r[1, 2] - r[2, 1]) / (4 * q[0])
        elif r[1, 1] >= T and r[1, 1] >= r[0, 0] and r[1, 1] >= r[2, 2]:
            q[1] = np.sqrt((1 + 2 * r[1, 1] - T) / 4)
            q[0], q[2], q[3] = (r[0, 1] + r[1, 0]) / (4 * q[1]), (r[1, 2] + r[2, 1]) / (4 * q[1]), (r[2, 0] - r[0, 2]) / (4 * q[1])
        elif r[2, 2] >= T and r[2, 2] >= r[0, 0] and r[2, 2] >= r[1, 1]:
            q[2] = np.sqrt((1 + 2 * r[2, 2] - T) / 4)
            q[0], q[1], q[3] = (r[0, 2] + r[2, 0]) / (4 * q[2]), (r[1, 2] + r[2, 1]) / (4 * q[2]), (r[0, 1] - r[1, 0]) / (4 * q[2])
        else:
            q[3] = np.sqrt((1 + T) / 4)
            q[0], q[1], q[2] = (r[1, 2] - r[2, 1]) / (4 * q[3]), (r[2, 0] - r[0, 2]) / (4 * q[3]), (r[0, 1] - r[1, 0]) / (4 * q[3])
        if q[3] < 0:
            q = -q
        out[i] = q / np.sqrt((q * q).sum())
    return out


def branch_of(R):
    """[W, 3, 3] -> [W] int: the branch of rot_2_quat a rotation takes, 0 / 1 / 2 = the r00 / r11 / r22 branch, 3 = the w branch
    (the conditions of rot_2_quat above, in the same order)."""
    R = np.asarray(R)
    d = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], -1)
    T = d.sum(-1)
    take = (d >= T[:, None]) & (d >= d[:, [1, 0, 0]]) & (d >= d[:, [2, 2, 1]])
    return np.where(take.any(-1), take.argmax(-1), 3)


BRANCHES = ("r00", "r11", "r22", "w")


def _cm(flat, dtype):
    """[W, 9] column-major -> [W, 3, 3] [row][col]."""
    return np.asarray(flat, dtype=dtype).reshape(-1, 3, 3).transpose(0, 2, 1)


def state_of(meas, dtype=np.float64, cov=True):
    """Measurement dict (rows of a batch) -> state.  P may be given dense ("P") or packed ("P_sym")."""
    s = {"DT": np.asarray(meas["DT"], dtype=dtype).reshape(-1), "alpha": np.asarray(meas["alpha"], dtype=dtype),
         "beta": np.asarray(meas["beta"], dtype=dtype), "R": quat_2_Rot(np.asarray(meas["q"], dtype=dtype))}
    for k in JAC:
        if k in meas:
            s[k] = _cm(meas[k], dtype)
    if cov and "P" in meas:
        s["P"] = np.asarray(meas["P"], dtype=dtype).reshape(-1, 15, 15).transpose(0, 2, 1)
    elif cov and "P_sym" in meas:
        s["P"] = unpack_sym(np.asarray(meas["P_sym"], dtype=dtype))
    return s


def zero_state(W, dtype=np.float64, jac=True, cov=True):
    s = {"DT": np.zeros(W, dtype), "alpha": np.zeros((W, 3), dtype), "beta": np.zeros((W, 3), dtype),
         "R": np.tile(np.eye(3, dtype=dtype), (W, 1, 1))}
    if jac:
        for k in JAC:
            s[k] = np.zeros((W, 3, 3), dtype)
    if cov:
        s["P"] = np.zeros((W, 15, 15), dtype)
    return s


def tri_index():
    cols = np.repeat(np.arange(15), np.arange(1, 16))
    rows = np.arange(120) - cols * (cols + 1) // 2
    return rows, cols


def unpack_sym(Ps):
    rows, cols = tri_index()
    M = np.zeros((Ps.shape[0], 15, 15), dtype=Ps.dtype)
    M[:, rows, cols] = Ps
    M[:, cols, rows] = Ps
    return M


def meas_of(s, q=None):
    """State -> measurement dict (flat, column-major; P stays in the state's dtype, everything else too).  q: the quaternion to
    report instead of rot_2_quat(R)."""
    W = s["DT"].shape[0]
    m = {"DT": s["DT"], "alpha": s["alpha"], "beta": s["beta"], "q": rot_2_quat(s["R"]) if q is None else q}
    for k in JAC:
        if k in s:
            m[k] = s[k].transpose(0, 2, 1).reshape(W, 9)
    if "P" in s:
        m["P"] = s["P"].transpose(0, 2, 1).reshape(W, 225)
        rows, cols = tri_index()
        m["P_sym"] = s["P"][:, rows, cols]
    return m


def phi(s):
    """Phi(X) [W, 15, 15] from the public fields of X."""
    W = s["DT"].shape[0]
    dtype = s["DT"].dtype
    F = np.tile(np.eye(15, dtype=dtype), (W, 1, 1))
    F[:, _TH, _TH] = s["R"]
    F[:, _TH, _BG] = -s["J_q"]
    F[:, _V, _TH] = -skew(s["beta"])
    F[:, _V, _BG] = s["J_b"]
    F[:, _V, _BA] = s["H_b"]
    F[:, _P, _TH] = -skew(s["alpha"])
    F[:, _P, _BG] = s["J_a"]
    F[:, _P, _V] = s["DT"][:, None, None] * np.eye(3, dtype=dtype)
    F[:, _P, _BA] = s["H_a"]
    return F


def compose(A, B, mutate=None, identity_blocks=True):
    """A o B for batches of states (same dtype); what B lacks (Jacobians, P) the result lacks.  identity_blocks: the (v,v), (p,p)
    and (p,v) blocks of Phi~ are set to I, I and DT_B I after the triple product (the module's docstring)."""
    assert mutate is None or mutate in MUTATIONS
    RA, RAt = A["R"], A["R"].transpose(0, 2, 1)
    dtB = B["DT"][:, None, None]
    mv = lambda M, v: np.einsum("wij,wj->wi", M, v)
    out = {"DT": A["DT"] + B["DT"], "R": B["R"] @ RA, "beta": A["beta"] + mv(RAt, B["beta"]),
           "alpha": A["alpha"] + A["beta"] * B["DT"][:, None] + mv(RAt, B["alpha"])}
    if "J_q" in A and "J_q" in B:
        sb = 0 if mutate == "drop_beta_x_Jq" else skew(B["beta"]) @ A["J_q"]
        out["J_q"] = B["R"] @ A["J_q"] + B["J_q"]
        out["J_b"] = A["J_b"] + RAt @ (B["J_b"] + sb)
        out["H_b"] = A["H_b"] + RAt @ B["H_b"]
        out["J_a"] = A["J_a"] + dtB * A["J_b"] + RAt @ (B["J_a"] + skew(B["alpha"]) @ A["J_q"])
        out["H_a"] = A["H_a"] + dtB * A["H_b"] + RAt @ B["H_a"]
    if "P" in A and "P" in B:
        W = RA.shape[0]
        T = np.tile(np.eye(15, dtype=RA.dtype), (W, 1, 1))
        T[:, _V, _V] = RAt
        T[:, _P, _P] = RAt
        Tt = T.transpose(0, 2, 1)
        F = phi(B)
        if mutate == "wrong_sign_theta_bg":
            F[:, _TH, _BG] = B["J_q"]
        Ft = T @ F @ Tt
        if identity_blocks:
            eye = np.eye(3, dtype=RA.dtype)
            Ft[:, _V, _V] = eye
            Ft[:, _P, _P] = eye
            Ft[:, _P, _V] = dtB * eye
        PB = B["P"] if mutate == "no_T_on_PB" else T @ B["P"] @ Tt
        P = Ft @ A["P"] @ Ft.transpose(0, 2, 1) + PB
        out["P"] = 0.5 * (P + P.transpose(0, 2, 1))
    return out


def fold(segments, dtype=np.float64, mutate=None, identity_blocks=True):
    """Left fold of a list of measurement dicts (each a batch of W rows: segment k of every window) -> measurement dict."""
    s = state_of(segments[0], dtype)
    for seg in segments[1:]:
        s = compose(s, state_of(seg, dtype), mutate, identity_blocks)
    return meas_of(s, q=np.asarray(segments[0]["q"], dtype=dtype) if len(segments) == 1 else None)


def merge_ref(meas, M, G, first=None, count=None, dtype=np.float64, packed_in=False, mutate=None, identity_blocks=True, state=False):
    """cpi_merge_batch on a measurement dict of in_rows rows: [M, ...] rows, count clamped into [0, G], groups clipped at in_rows,
    count 0 -> the zero state, count 1 -> the row itself (q as it is).  packed_in: read the covariance from P_sym.  state: return
    (measurement dict, the folded state) -- the state's R is the rotation rot_2_quat is given (branch_of)."""
    in_rows = np.asarray(meas["DT"]).reshape(-1).shape[0]
    f = np.arange(M, dtype=np.int64) * G if first is None else np.asarray(first, dtype=np.int64).copy()
    n = np.full(M, G, dtype=np.int64) if count is None else np.asarray(count, dtype=np.int64).copy()
    n = np.clip(n, 0, G)
    f = np.clip(f, 0, in_rows)
    n = np.minimum(n, in_rows - f)
    src = dict(meas)
    if packed_in:
        src.pop("P", None)
    jac, cov = "J_q" in src, ("P" in src or "P_sym" in src)
    S = zero_state(M, dtype, jac, cov)
    q1 = np.tile(np.array([0, 0, 0, 1], dtype=dtype), (M, 1))
    for k in range(int(n.max()) if M else 0):
        act = np.nonzero(k < n)[0]
        rows = {key: np.asarray(v)[f[act] + k] for key, v in src.items()}
        B = state_of(rows, dtype)
        new = B if k == 0 else compose({key: v[act] for key, v in S.items()}, B, mutate, identity_blocks)
        for key in S:
            S[key][act] = new[key]
        if k == 0:
            q1[act] = np.asarray(rows["q"], dtype=dtype)
    out = meas_of(S)
    keep = n <= 1
    out["q"][keep] = q1[keep]
    return (out, S) if state else out


def ragged_groups(M, G, in_rows, seed):
    """first / count with every count 0 .. G, counts past G and below 0, groups that reach and pass the end of the input."""
    g = np.random.default_rng(seed)
    first = g.integers(0, in_rows - G, size=M).astype(np.int64)
    count = g.integers(0, G + 1, size=M).astype(np.int32)
    if M >= 4:
        first[-1], count[-1] = in_rows - 1, G          # clipped to one row (G > 1) -> the row itself
        count[0] = G + 3                               # clamped to G
        count[1] = -2                                  # clamped to 0
        first[2] = in_rows                             # nothing left
    return first, count


def cut_segments(kn, cuts):
    """knots [W, N + 1, 7] -> the list of segments [W, n_s + 1, 7] between consecutive cut indices (consecutive segments share their
    boundary knot); cuts: increasing interior knot indices."""
    edges = [0] + list(cuts) + [kn.shape[1] - 1]
    return [kn[:, a:b + 1] for a, b in zip(edges[:-1], edges[1:])]


def align_q(q, ref):
    """q with the sign of every row flipped to match ref (q and -q are one rotation)."""
    q = np.asarray(q, dtype=np.float64)
    sgn = np.where((q * np.asarray(ref, dtype=np.float64)).sum(-1) < 0, -1.0, 1.0)
    return q * sgn[:, None]


def deviations(got, ref):
    """max-abs deviation per mean / Jacobian field (q sign-aligned), P relative to sqrt(P_ii P_jj) of ref."""
    from tests.tol import cov_rel_err
    d = {}
    for k in MEAN + JAC:
        if k in got and k in ref:
            g = align_q(got[k], ref[k]) if k == "q" else np.asarray(got[k], dtype=np.float64)
            d[k] = float(np.abs(g - np.asarray(ref[k], dtype=np.float64)).max())
    if "P" in got and "P" in ref:
        d["P"] = cov_rel_err(np.asarray(got["P"], dtype=np.float64), np.asarray(ref["P"], dtype=np.float64))
    return d


# ---- rows of tests/hostsim/hostsim_merge.cpp: 401 doubles = the staged operand layout, P, P_sym
HS_FIELDS = (("DT", 0, 1), ("alpha", 1, 3), ("beta", 4, 3), ("q", 7, 4), ("J_q", 11, 9), ("J_a", 20, 9), ("J_b", 29, 9), ("H_a", 38, 9),
             ("H_b", 47, 9), ("P", 56, 225), ("P_sym", 281, 120))
HS_ROW = 401


def hs_rows(meas):
    """Measurement dict -> [rows, 401] float64 (P_sym filled from P)."""
    n = np.asarray(meas["DT"]).reshape(-1).shape[0]
    raw = np.zeros((n, HS_ROW))
    rows, cols = tri_index()
    for k, o, w in HS_FIELDS:
        if k == "P_sym":
            raw[:, o:o + w] = np.asarray(meas["P"], dtype=np.float64).reshape(n, 15, 15)[:, cols, rows]
        else:
            raw[:, o:o + w] = np.asarray(meas[k], dtype=np.float64).reshape(n, w)
    return raw


def hs_meas(raw):
    return {k: (raw[:, o] if w == 1 else raw[:, o:o + w]) for k, o, w in HS_FIELDS}


# ---- hard operands: large rotations, odd quaternions, a zero-state row, and the rows of a long fold
HARD_W, HARD_N, HARD_S, HARD_GYRO = 256, 40, 8, 8.0
LONG_W, LONG_G = 64, 40
REGIMES = ("as computed", "q negated on odd segments", "q rounded to float32", "one zero-state segment")
ZERO_AT = (0, 3, 7)


def hard_knots():
    """(knots [256, 41, 7], lin [256, 6], q_k_lin [256, 4]) as make_windows(256, 40, edge_cases=False) gives them, the three gyro
    columns multiplied by 8: rates of up to 20 rad/s (inside a 2000 dps gyro), 3 rad and more over the 0.2 s of a window."""
    from cpi_amd import synth
    kn, lin, q = synth.make_windows(HARD_W, HARD_N, edge_cases=False)
    kn = kn.clone()
    kn[:, :, 1:4] *= HARD_GYRO
    return kn, lin, q


def regime_of(w):
    return np.asarray(w) % 4


def stack_rows(parts):
    """segments [S] of batches [W] (arrays or tensors) -> one measurement dict of W * S numpy rows, window-major: row w * S + s;
    P_sym is the upper triangle of P where the batches do not bring it."""
    S, out = len(parts), {}
    host = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v, dtype=np.float64)
    for k in MEAN + JAC + ("P", "P_sym"):
        if k == "P_sym" and k not in parts[0]:
            rows, cols = tri_index()
            out[k] = np.ascontiguousarray(out["P"].reshape(-1, 15, 15)[:, cols, rows])
            continue
        a = np.stack([host(p[k]).reshape(host(p["DT"]).reshape(-1).shape[0], -1) for p in parts], axis=1)
        out[k] = np.ascontiguousarray(a.reshape(a.shape[0] * S, -1))
    out["DT"] = out["DT"].reshape(-1)
    return out


def hard_rows(measure):
    """measure(knots [W, n + 1, 7], lin [W, 6]) -> the model-1 measurements of a batch (imu_avg = 1; a dict of [W, ...] arrays or
    tensors with the means, the five Jacobians and P): the oracle on the CPU, Engine.preintegrate on the GPU.
    Returns (rows, regime, long_rows):
      rows       the 2048 operand rows of hard_knots() cut into 8 segments of 5 intervals, row w * 8 + s, after the regime of
                 window w (w % 4, REGIMES): 0 as computed; 1 q negated on the odd segments; 2 q rounded to float32 and back
                 (| |q|^2 - 1 | <= 6e-8); 3 one segment replaced by the zero-state row (what count = 0 writes), at position 0, 3
                 or 7 in turn.  Four consecutive windows = four consecutive groups = one wavefront hold all four regimes.
      regime     [256] the regime of every window
      long_rows  the 40 x 64 one-interval rows of the first 64 windows, row w * 40 + s, as computed."""
    kn, lin, _ = hard_knots()
    step = HARD_N // HARD_S
    rows = stack_rows([measure(kn[:, s * step:s * step + step + 1].contiguous(), lin) for s in range(HARD_S)])
    regime = regime_of(np.arange(HARD_W))
    w, s = np.divmod(np.arange(HARD_W * HARD_S), HARD_S)
    neg = (regime[w] == 1) & (s % 2 == 1)
    rows["q"][neg] = -rows["q"][neg]
    f32 = regime[w] == 2
    rows["q"][f32] = rows["q"][f32].astype(np.float32).astype(np.float64)
    zero = (regime[w] == 3) & (s == np.asarray(ZERO_AT)[(w // 4) % 3])
    for k in rows:
        rows[k][zero] = 0.0
    rows["q"][zero, 3] = 1.0
    long_rows = stack_rows([measure(kn[:LONG_W, s:s + 2].contiguous(), lin[:LONG_W].contiguous()) for s in range(LONG_G)])
    return rows, regime, long_rows


def joined_angle(q):
    """[W, 4] (any float type) -> the rotation angle in [0, pi] of every row."""
    q = np.asarray(q)
    return np.asarray(2 * np.arctan2(np.sqrt((q[:, :3] * q[:, :3]).sum(-1)), np.abs(q[:, 3])), dtype=np.float64)


def long_counts():
    """[64] int32 counts of the long fold's mixed call: 0 .. 40 drawn per group, with 40, 0, 1 and 39 side by side in every fourth
    wavefront (groups 16 i .. 16 i + 3), so finished groups idle through up to 40 trips beside a group that still folds."""
    count = np.random.default_rng(40).integers(0, LONG_G + 1, size=LONG_W).astype(np.int32)
    count[0::16], count[1::16], count[2::16], count[3::16] = LONG_G, 0, 1, LONG_G - 1
    return count


def group_regime(M, G, first=None):
    """[M] the regime (REGIMES) of the window that holds the first row of every group of hard_rows' rows."""
    f = np.arange(M, dtype=np.int64) * G if first is None else np.asarray(first, dtype=np.int64)
    return regime_of(np.clip(f, 0, HARD_W * HARD_S - 1) // HARD_S)


def deviations_by(got, ref, label_of, names):
    """deviations() over the rows of every label: {names[i]: deviations of the rows with label_of == i} (labels without a row left out)."""
    out = {}
    for i, name in enumerate(names):
        m = np.asarray(label_of) == i
        if m.any():
            out[name] = deviations({k: np.asarray(v)[m] for k, v in got.items()}, {k: np.asarray(v)[m] for k, v in ref.items()})
    return out


def worst(d):
    """deviations() -> (worst mean field, worst Jacobian field, P): three figures."""
    return (max(d[k] for k in MEAN if k in d), max([d[k] for k in JAC if k in d] or [0.0]), d.get("P", 0.0))
