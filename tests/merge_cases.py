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

MUTATIONS (profiles/merge_bench.md): compose(..., mutate=) breaks one term on purpose, so that the tests can show they would see it."""
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


def compose(A, B, mutate=None):
    """A o B for batches of states (same dtype); what B lacks (Jacobians, P) the result lacks."""
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
        PB = B["P"] if mutate == "no_T_on_PB" else T @ B["P"] @ Tt
        P = Ft @ A["P"] @ Ft.transpose(0, 2, 1) + PB
        out["P"] = 0.5 * (P + P.transpose(0, 2, 1))
    return out


def fold(segments, dtype=np.float64, mutate=None):
    """Left fold of a list of measurement dicts (each a batch of W rows: segment k of every window) -> measurement dict."""
    s = state_of(segments[0], dtype)
    for seg in segments[1:]:
        s = compose(s, state_of(seg, dtype), mutate)
    return meas_of(s, q=np.asarray(segments[0]["q"], dtype=dtype) if len(segments) == 1 else None)


def merge_ref(meas, M, G, first=None, count=None, dtype=np.float64, packed_in=False):
    """cpi_merge_batch on a measurement dict of in_rows rows: [M, ...] rows, count clamped into [0, G], groups clipped at in_rows,
    count 0 -> the zero state, count 1 -> the row itself (q as it is).  packed_in: read the covariance from P_sym."""
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
        new = B if k == 0 else compose({key: v[act] for key, v in S.items()}, B)
        for key in S:
            S[key][act] = new[key]
        if k == 0:
            q1[act] = np.asarray(rows["q"], dtype=dtype)
    out = meas_of(S)
    keep = n <= 1
    out["q"][keep] = q1[keep]
    return out


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
