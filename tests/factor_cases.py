"""Inputs for the tests of the evaluateError sweeps (cpi_factor_eval_batch, _packed_, _whitened_[tri_], cpi_factor_hessian_[tri_]batch)
away from the predicted state, where cpi_amd.synth.make_states never goes, and a second, independent restatement of
ImuFactorCPIv1.cpp:37-208 / ImuFactorCPIv2.cpp:38-212 in numpy.longdouble (x87: 64-bit mantissa) to compare them with.

make_states puts state j on the prediction (+ 1e-3 rad, 1e-2 m ...) and the biases of state i on the linearisation point
(+ 1e-3 / 1e-2): the four quaternion products of the residual have w ~ 1 (the flip of quat_multiply never fires), q_b has an
angle of ~2.5e-4 rad (rot_2_quat: trace branch only, sincos_fast: short polynomial only) and S.Ra / S.Rb are O(1e-2).  The
regimes below move one of these at a time; mixed() deals them out factor by factor so that every wavefront of every sweep
(4, 8 or 21 factors each) holds a mix of them.

tests/test_factor_cases_cpu.py checks, on the CPU, the oracle and the host emulation of the kernels against the reference
here and that no sign decision of these inputs sits within rounding of zero; tests/test_gpu_factor_edges.py runs the sweeps."""
import functools
import math
import os

import numpy as np

LD = np.longdouble
SEED = 20260117
MARGIN_MIN = 1e-9          # a sign decision with |w| below this is a genuine discontinuity: mixed() must not contain one

# columns of a factor record (oracle_py.FACTOR_FIELDS)
C_ALPHA, C_BETA, C_Q, C_BA, C_BG = slice(0, 3), slice(3, 6), slice(6, 10), slice(10, 13), slice(13, 16)
C_JQ, C_JB, C_JA, C_HB, C_HA = slice(16, 25), slice(25, 34), slice(34, 43), slice(43, 52), slice(52, 61)
C_DT, C_GRAV, C_QLIN, C_OB, C_OA = 61, slice(62, 65), slice(65, 69), slice(69, 78), slice(78, 87)


# ------------------------------------------------------------------------------------------ the long-double reference
def _skew(w):
    S = np.zeros(w.shape[:-1] + (3, 3), dtype=LD)
    S[..., 0, 1], S[..., 0, 2] = -w[..., 2], w[..., 1]
    S[..., 1, 0], S[..., 1, 2] = w[..., 2], -w[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -w[..., 1], w[..., 0]
    return S


def _eye(F):
    return np.broadcast_to(np.eye(3, dtype=LD), (F, 3, 3)).copy()


def _mv(A, x):
    return (A * x[:, None, :]).sum(axis=2)


def _cm3(a):
    """[F, 9] column-major -> [F, 3, 3] [row][col]."""
    return np.asarray(a, dtype=LD).reshape(-1, 3, 3).transpose(0, 2, 1)


def _norm4(q):
    return np.sqrt((q * q).sum(axis=1))


def rot_2_quat_ld(R):
    """quat_ops.h:45-86 -> (q [F, 4], its w before the flip (scaled as q) [F], the branch taken: 0, 1, 2 diagonal, 3 trace [F])."""
    r00, r11, r22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    T = r00 + r11 + r22
    b0 = (r00 >= T) & (r00 >= r11) & (r00 >= r22)
    b1 = ~b0 & (r11 >= T) & (r11 >= r00) & (r11 >= r22)
    b2 = ~b0 & ~b1 & (r22 >= T) & (r22 >= r00) & (r22 >= r11)
    b3 = ~(b0 | b1 | b2)
    q = np.zeros((R.shape[0], 4), dtype=LD)
    with np.errstate(all="ignore"):
        for sel, d, m, others in (
                (b0, 1 + 2 * r00 - T, 0, ((1, R[:, 0, 1] + R[:, 1, 0]), (2, R[:, 0, 2] + R[:, 2, 0]), (3, R[:, 1, 2] - R[:, 2, 1]))),
                (b1, 1 + 2 * r11 - T, 1, ((0, R[:, 0, 1] + R[:, 1, 0]), (2, R[:, 1, 2] + R[:, 2, 1]), (3, R[:, 2, 0] - R[:, 0, 2]))),
                (b2, 1 + 2 * r22 - T, 2, ((0, R[:, 0, 2] + R[:, 2, 0]), (1, R[:, 1, 2] + R[:, 2, 1]), (3, R[:, 0, 1] - R[:, 1, 0]))),
                (b3, 1 + T, 3, ((0, R[:, 1, 2] - R[:, 2, 1]), (1, R[:, 2, 0] - R[:, 0, 2]), (2, R[:, 0, 1] - R[:, 1, 0])))):
            lead = np.sqrt(d / 4)
            q[sel, m] = lead[sel]
            for k, v in others:
                q[sel, k] = ((1 / (4 * lead)) * v)[sel]
    w0 = q[:, 3].copy()
    q = np.where((q[:, 3] < 0)[:, None], -q, q)
    n = _norm4(q)
    branch = np.where(b0, 0, np.where(b1, 1, np.where(b2, 2, 3)))
    return q / n[:, None], w0 / n, branch


def quat_multiply_ld(q, p):
    """quat_ops.h:115-128 -> (q (x) p flipped to w >= 0 and normalised, |w| after the normalisation, whether it was flipped)."""
    qv, pv = q[:, :3], p[:, :3]
    t = np.empty_like(q)
    t[:, :3] = q[:, 3:4] * pv - np.cross(qv, pv) + qv * p[:, 3:4]
    t[:, 3] = q[:, 3] * p[:, 3] - (qv * pv).sum(axis=1)
    flip = t[:, 3] < 0
    t = np.where(flip[:, None], -t, t)
    t = t / _norm4(t)[:, None]
    return t, np.abs(t[:, 3]), flip


def quat_inv_ld(q):
    return q * np.array([-1, -1, -1, 1], dtype=LD)


def exp_so3_ld(w):
    """quat_ops.h:145-162, the identity at theta == 0."""
    theta = np.sqrt((w * w).sum(axis=1))
    zero = theta == 0
    th = np.where(zero, LD(1), theta)
    wx = _skew(w)
    R = _eye(w.shape[0]) + (np.sin(th) / th)[:, None, None] * wx + ((1 - np.cos(th)) / (th * th))[:, None, None] * (wx @ wx)
    R[zero] = np.eye(3, dtype=LD)
    return R


def quat_2_rot_ld(q):
    """quat_ops.h:104-109 (no normalisation: 2 w^2 - 1 on the quaternion as it comes)."""
    c = 2 * q[:, 3] * q[:, 3] - 1
    return c[:, None, None] * _eye(q.shape[0]) - 2 * q[:, 3, None, None] * _skew(q[:, :3]) + 2 * q[:, :3, None] * q[:, None, :3]


def _qL(q, sign):
    return q[:, 3, None, None] * _eye(q.shape[0]) + sign * _skew(q[:, :3])


def evaluate_error_longdouble(model, rec, xi, xj, details=False):
    """ImuFactorCPIv{1,2}::evaluateError restated from oracle/cpi_oracle.c: factor_eval in numpy.longdouble, the batch at once.
    rec [F, 87] (matrices column-major), xi / xj [F, 16] -> err [F, 15], H1 [F, 225], H2 [F, 225] (column-major flat, longdouble) and
    margin [F]: the smallest |w| at the sign decisions taken for that factor -- the normalised results of the quat_multiply calls
    q_n, q_rminus, q_r, q_m, q_kR (model 2) and the w of rot_2_quat before its flip.  details=True adds a dict: the branch of
    rot_2_quat taken, |J_q dbg| and which results were flipped."""
    v2 = (model == 2)
    rec, xi, xj = (np.asarray(a, dtype=LD) for a in (rec, xi, xj))      # doubles convert exactly; longdouble states pass through
    F = rec.shape[0]
    J_q, J_beta, J_alpha = _cm3(rec[:, C_JQ]), _cm3(rec[:, C_JB]), _cm3(rec[:, C_JA])
    H_beta, H_alpha, O_beta, O_alpha = _cm3(rec[:, C_HB]), _cm3(rec[:, C_HA]), _cm3(rec[:, C_OB]), _cm3(rec[:, C_OA])
    dt, grav, q_meas = rec[:, C_DT], rec[:, C_GRAV], rec[:, C_Q]
    q_i, bg_i, v_i, ba_i, p_i = xi[:, 0:4], xi[:, 4:7], xi[:, 7:10], xi[:, 10:13], xi[:, 13:16]
    q_j, bg_j, v_j, ba_j, p_j = xj[:, 0:4], xj[:, 4:7], xj[:, 7:10], xj[:, 10:13], xj[:, 13:16]
    dbg, dba = bg_i - rec[:, C_BG], ba_i - rec[:, C_BA]

    q_b, w_b, branch = rot_2_quat_ld(exp_so3_ld(-_mv(J_q, dbg)))
    q_n, m_n, f_n = quat_multiply_ld(q_j, quat_inv_ld(q_i))
    q_rminus, m_rm, f_rm = quat_multiply_ld(q_n, quat_inv_ld(q_meas))
    q_r, m_r, f_r = quat_multiply_ld(q_rminus, q_b)
    q_m, m_m, f_m = quat_multiply_ld(quat_inv_ld(q_b), q_meas)
    margin = np.minimum.reduce([m_n, m_rm, m_r, m_m, np.abs(w_b)])
    q_kR = np.zeros((F, 4), dtype=LD)
    q_kR[:, 3] = 1
    f_k = np.zeros(F, dtype=bool)
    if v2:
        q_kR, m_k, f_k = quat_multiply_ld(q_i, quat_inv_ld(rec[:, C_QLIN]))
        margin = np.minimum(margin, m_k)
    dthk = 2 * q_kR[:, :3]

    Rk = quat_2_rot_ld(q_i)
    if not v2:
        pa = p_j - p_i - v_i * dt[:, None] + LD(0.5) * grav * (dt * dt)[:, None]
        pb = v_j - v_i + grav * dt[:, None]
    else:
        pa = p_j - p_i - v_i * dt[:, None]
        pb = v_j - v_i
    Ra, Rb = _mv(Rk, pa), _mv(Rk, pb)
    alphahat = Ra - _mv(J_alpha, dbg) - _mv(H_alpha, dba)
    betahat = Rb - _mv(J_beta, dbg) - _mv(H_beta, dba)
    if v2:
        alphahat = alphahat - _mv(O_alpha, dthk)
        betahat = betahat - _mv(O_beta, dthk)
    err = np.concatenate([2 * q_r[:, :3], bg_j - bg_i, betahat - rec[:, C_BETA], ba_j - ba_i, alphahat - rec[:, C_ALPHA]], axis=1)

    I = _eye(F)
    Hi = np.zeros((F, 15, 15), dtype=LD)
    Hi[:, 0:3, 0:3] = -(_qL(q_n, -1) @ _qL(q_m, -1) + q_n[:, :3, None] * q_m[:, None, :3])
    Hi[:, 6:9, 0:3] = _skew(Rb) - ((O_beta @ _qL(q_kR, +1)) if v2 else 0)
    Hi[:, 12:15, 0:3] = _skew(Ra) - ((O_alpha @ _qL(q_kR, +1)) if v2 else 0)
    Hi[:, 0:3, 3:6] = _qL(q_rminus, -1) @ J_q
    Hi[:, 3:6, 3:6] = -I
    Hi[:, 6:9, 3:6] = -J_beta
    Hi[:, 12:15, 3:6] = -J_alpha
    Hi[:, 6:9, 6:9] = -Rk
    Hi[:, 12:15, 6:9] = -dt[:, None, None] * Rk
    Hi[:, 6:9, 9:12] = -H_beta
    Hi[:, 9:12, 9:12] = -I
    Hi[:, 12:15, 9:12] = -H_alpha
    Hi[:, 12:15, 12:15] = -Rk
    Hj = np.zeros((F, 15, 15), dtype=LD)
    Hj[:, 0:3, 0:3] = _qL(q_r, +1)
    Hj[:, 3:6, 3:6] = I
    Hj[:, 6:9, 6:9] = Rk
    Hj[:, 9:12, 9:12] = I
    Hj[:, 12:15, 12:15] = Rk
    out = (err, Hi.transpose(0, 2, 1).reshape(F, 225), Hj.transpose(0, 2, 1).reshape(F, 225), np.asarray(margin, dtype=np.float64))
    if details:
        return out + (dict(branch=branch, angle_b=np.asarray(np.sqrt((_mv(J_q, dbg) ** 2).sum(axis=1)), dtype=np.float64),
                           flip=dict(q_n=f_n, q_rminus=f_rm, q_r=f_r, q_m=f_m, q_kR=f_k, q_b=w_b < 0)),)
    return out


def predict_longdouble(model, rec, xi):
    """GraphSolver_IMU.cpp:263-307 (oracle/cpi_oracle.c: cpi_oracle_predict) in longdouble -> xj [F, 16]."""
    rec, xi = (np.asarray(a, dtype=LD) for a in (rec, xi))
    q_i, v_i, p_i = xi[:, 0:4], xi[:, 7:10], xi[:, 13:16]
    dt, grav = rec[:, C_DT, None], rec[:, C_GRAV]
    xj = xi.copy()
    xj[:, 0:4] = quat_multiply_ld(rec[:, C_Q], q_i)[0]
    Rinv = quat_2_rot_ld(quat_inv_ld(q_i))
    rb, ra = _mv(Rinv, rec[:, C_BETA]), _mv(Rinv, rec[:, C_ALPHA])
    if model == 1:
        xj[:, 7:10] = v_i - grav * dt + rb
        xj[:, 13:16] = p_i + v_i * dt - LD(0.5) * grav * dt * dt + ra
    else:
        xj[:, 7:10] = v_i + rb
        xj[:, 13:16] = p_i + v_i * dt + ra
    return xj


def _rc(a):
    """[F, 225] column-major flat -> [F, 15, 15] [row][col], longdouble."""
    return np.asarray(a, dtype=LD).reshape(-1, 15, 15).transpose(0, 2, 1)


def whitened_longdouble(ref, R):
    """(R e, R H1, R H2) from the reference's (err, H1, H2, ...) and R [F, 225] (column-major doubles, used as given)."""
    Rl = _rc(R)
    e, H1, H2 = ref[0], _rc(ref[1]), _rc(ref[2])
    F = e.shape[0]
    return (_mv(Rl, e), (Rl @ H1).transpose(0, 2, 1).reshape(F, 225), (Rl @ H2).transpose(0, 2, 1).reshape(F, 225))


def hessian_longdouble(ref, R):
    """[F, 496]: packed upper triangle (entry (i, d), i <= d, at i + d (d + 1) / 2) of Hc^T (R^T R) Hc, Hc = [H1 H2 -e]."""
    Rl = _rc(R)
    Hc = np.concatenate([_rc(ref[1]), _rc(ref[2]), -ref[0][:, :, None]], axis=2)
    A = Rl @ Hc
    M = A.transpose(0, 2, 1) @ A
    return np.stack([M[:, i, d] for d in range(31) for i in range(d + 1)], axis=1)


# ------------------------------------------------------------------------------------------ base cases
@functools.lru_cache(maxsize=None)
def base_cases(model):
    """320 base cases, every fifth one (k % 5 == 4) from other seeds than the golden file's: rec [B, 87], xi, xj [B, 16] and the
    windows (knots [B, 51, 7], lin, q_k_lin) whose preintegration gives the covariance that goes with record k.
    The golden records (tests/golden/factor_256.npz) keep their stored doubles; the others are the oracle's preintegration of
    synth.make_windows(32, 50, seed) for two seeds with the states of synth.make_states -- for model 2 the even ones with state
    i's orientation near q_k_lin as in the golden file, the odd ones as make_states leaves it (q_kR anywhere, flips included)."""
    import torch
    from cpi_amd import synth
    from oracle import oracle_py as op
    d = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_256.npz")))
    kg, lg, qg = (t.numpy() for t in synth.make_windows(256, 50, seed=synth.BASE_SEED + 2))     # oracle/gen_golden.py
    recs, xis, xjs, kns, lins, qs = [], [], [], [], [], []
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    orc = op.oracle()
    for seed in (7101, 7102):
        kn, lin, q = (t.numpy() for t in synth.make_windows(32, 50, seed=seed, edge_cases=False))
        out = orc.run(op.make_params(model, 0, 1), kn, lin, q)
        rec = op.factor_records(out, lin, q if model == 2 else None)
        xi, xj = (t.numpy().copy() for t in synth.make_states(T(out["alpha"]), T(out["beta"]), T(out["q"]), T(out["DT"]), T(lin),
                                                               model, seed=seed + 50))
        if model == 2:
            rng = np.random.default_rng(seed)
            pert = rng.standard_normal((32, 15)) * np.array([1e-3] * 3 + [1e-4] * 3 + [1e-2] * 3 + [1e-3] * 3 + [1e-2] * 3)
            dth = 1e-2 * rng.standard_normal((32, 3))
            for k in range(0, 32, 2):
                xi[k] = orc.retract(np.concatenate([q[k], xi[k, 4:]]), np.concatenate([dth[k], np.zeros(12)]))
                xj[k] = orc.retract(orc.predict(2, rec[k:k + 1], xi[k:k + 1])[0], pert[k])
        recs.append(rec); xis.append(xi); xjs.append(xj); kns.append(kn); lins.append(lin); qs.append(q)
    other = [np.concatenate(a) for a in (recs, xis, xjs, kns, lins, qs)]
    gold = [d["v%d_rec" % model], d["v%d_xi" % model], d["v%d_xj" % model], kg, lg, qg]
    B = 320
    k = np.arange(B)
    from_other = (k % 5 == 4)
    src = np.where(from_other, k // 5, k - k // 5)
    out = []
    for g, o in zip(gold, other):
        a = np.empty((B,) + g.shape[1:])
        a[~from_other] = g[src[~from_other]]
        a[from_other] = o[src[from_other]]
        a.setflags(write=False)
        out.append(a)
    return dict(zip(("rec", "xi", "xj", "knots", "lin", "q_k_lin"), out))


# ------------------------------------------------------------------------------------------ the regimes
def _qmul(q, p):
    """JPL product of double quaternions, normalised, w >= 0 (quat_ops.h:115-128)."""
    qv, pv = q[:, :3], p[:, :3]
    t = np.concatenate([q[:, 3:4] * pv - np.cross(qv, pv) + qv * p[:, 3:4], q[:, 3:4] * p[:, 3:4] - (qv * pv).sum(1, keepdims=True)], axis=1)
    t = np.where(t[:, 3:4] < 0, -t, t)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def _resrot(a):
    def f(rec, xi, xj, r):
        dq = np.concatenate([math.sin(a / 2) * r["axis"], np.full((xi.shape[0], 1), math.cos(a / 2))], axis=1)
        xj = xj.copy()
        xj[:, 0:4] = _qmul(dq, xj[:, 0:4])
        return xi, xj
    return f


def _qb(phi, on_axis=False):
    def f(rec, xi, xj, r):
        xi = xi.copy()
        J = rec[:, C_JQ].reshape(-1, 3, 3).transpose(0, 2, 1)
        # the direction's largest component sits on x, y, z in turn (r["turn"]): next to pi each one is another branch of rot_2_quat
        u = r["dir"]
        big = np.abs(u).argmax(axis=1)
        u = np.stack([np.roll(u[k], int(r["turn"][k] - big[k])) for k in range(u.shape[0])]) if u.shape[0] else u
        if on_axis:       # 1e-3 beside the coordinate axis: the other two components of q_b are ~5e-4, small but not rounding
            u = np.eye(3)[r["turn"]] + 1e-3 * u
            u = u / np.linalg.norm(u, axis=1, keepdims=True)
        xi[:, 4:7] = rec[:, C_BG] + (np.linalg.solve(J, (-phi * u)[:, :, None])[:, :, 0] if phi != 0 else 0.0)
        return xi, xj
    return f


def _negw(i, j):
    def f(rec, xi, xj, r):
        xi, xj = xi.copy(), xj.copy()
        if i:
            xi[:, 0:4] = -xi[:, 0:4]
        if j:
            xj[:, 0:4] = -xj[:, 0:4]
        return xi, xj
    return f


def _f32quat(rec, xi, xj, r):
    xi, xj = xi.copy(), xj.copy()
    xi[:, 0:4] = xi[:, 0:4].astype(np.float32).astype(np.float64)
    xj[:, 0:4] = xj[:, 0:4].astype(np.float32).astype(np.float64)
    return xi, xj


def _utm(rec, xi, xj, r):
    xi, xj = xi.copy(), xj.copy()
    xi[:, 13:16] += 5e6 * r["off"]
    xj[:, 13:16] += 5e6 * r["off"]
    return xi, xj


def _bigres(rec, xi, xj, r):
    xj = xj.copy()
    xj[:, 7:10] += 100.0 * r["dv"]
    xj[:, 13:16] += 1e4 * r["dp"]
    return xi, xj


def _base(rec, xi, xj, r):
    return xi, xj


def _both(f, g):
    def h(rec, xi, xj, r):
        xi, xj = f(rec, xi, xj, r)
        return g(rec, xi, xj, r)
    return h


RESROT = [0.3, 1.0, 2.0, 3.0, math.pi - 1e-3, math.pi + 1e-3, 4.5]
QB = [0.0, 1e-9, 0.2, 0.3, 1.5, 2.5, math.pi - 1e-3]
REGIMES = ([("base", _base)] + [("resrot(%.4g)" % a, _resrot(a)) for a in RESROT] + [("qb(%.4g)" % p, _qb(p)) for p in QB]
           + [("negw_i", _negw(1, 0)), ("negw_j", _negw(0, 1)), ("negw_ij", _negw(1, 1)), ("f32quat", _f32quat), ("utm", _utm),
              ("bigres", _bigres), ("resrot(2)+qb(1.5)", _both(_resrot(2.0), _qb(1.5))),
              # beyond the issue's table: two large rotations about independent axes compose past pi about half the time, which is what
              # flips q_r = q_rminus (x) q_b (the rows above flip it in a handful of cases only)
              ("resrot(2.5)+qb(2.5)", _both(_resrot(2.5), _qb(2.5))),
              # ... and a rotation next to pi 1e-3 beside a coordinate axis: there the diagonal branches of rot_2_quat are NOT
              # interchangeable.  Each branch is exact algebra, so taking the "wrong" one goes unnoticed wherever its own component is
              # O(1); with that component at 5e-4 its square root loses eight digits.  (ON the axis the device hides it again: the
              # clamp of mag_and_inverse turns a zero argument into a common scale that the normalisation removes.)
              ("qb_axis(3.141)", _qb(math.pi - 1e-3, on_axis=True))])
if len(REGIMES) % 2 == 0 or len(REGIMES) % 3 == 0:           # coprime to 2 and 3: every regime meets every lane group of the 4-, 8- and
    REGIMES.append(("base", _base))                          # 21-factor wavefronts
assert len(REGIMES) % 2 and len(REGIMES) % 3
NAMES = [n for n, _ in REGIMES]
NEGW = [k for k, n in enumerate(NAMES) if n.startswith("negw")]


def _unit_rows(rng, F):
    u = rng.standard_normal((F, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def mixed(model, F, negate=True, seed=SEED):
    """The batch of every test: factor k is base case k mod 320 under regime k mod len(REGIMES), in the order of REGIMES.  Each random
    quantity has a generator of its own, so mixed(F) is the head of mixed(F') for F < F'.  negate=False leaves the quaternions of the
    negw regimes as they are (the same rotations).  Returns rec [F, 87], xi, xj [F, 16], regime [F] and base [F]."""
    b = base_cases(model)
    k = np.arange(F)
    base, regime = k % b["rec"].shape[0], k % len(REGIMES)
    rec, xi, xj = b["rec"][base].copy(), b["xi"][base].copy(), b["xj"][base].copy()
    g = lambda tag: np.random.default_rng([seed, model, tag])
    draws = dict(axis=_unit_rows(g(1), F), dir=_unit_rows(g(2), F), off=g(3).standard_normal((F, 3)), dv=g(4).standard_normal((F, 3)),
                 dp=g(5).standard_normal((F, 3)), turn=(k // len(REGIMES)) % 3)
    for r, (name, fn) in enumerate(REGIMES):
        sel = np.nonzero(regime == r)[0]
        if sel.size == 0 or (name.startswith("negw") and not negate):
            continue
        xi[sel], xj[sel] = fn(rec[sel], xi[sel], xj[sel], {key: v[sel] for key, v in draws.items()})
    return dict(rec=rec, xi=xi, xj=xj, regime=regime, base=base)


def meas_of(rec):
    """The preintegration outputs a sweep is given (cpi_outputs field names), lin and q_k_lin from factor records."""
    meas = dict(DT=rec[:, C_DT], alpha=rec[:, C_ALPHA], beta=rec[:, C_BETA], q=rec[:, C_Q], J_q=rec[:, C_JQ], J_b=rec[:, C_JB],
                J_a=rec[:, C_JA], H_b=rec[:, C_HB], H_a=rec[:, C_HA], O_b=rec[:, C_OB], O_a=rec[:, C_OA])
    meas = {key: np.ascontiguousarray(v) for key, v in meas.items()}
    return meas, np.ascontiguousarray(np.concatenate([rec[:, C_BG], rec[:, C_BA]], axis=1)), np.ascontiguousarray(rec[:, C_QLIN])


def rel_err(got, ref):
    """Per factor: max |got - ref| / max(1, max |ref| of that output of that factor), in longdouble -> float64 [F]."""
    ref = np.asarray(ref, dtype=LD)
    d = np.abs(np.asarray(got, dtype=LD) - ref).max(axis=1)
    return np.asarray(d / np.maximum(1, np.abs(ref).max(axis=1)), dtype=np.float64)


def rel_err_scaled(got, ref):
    """Per factor: max |got - ref| / max |ref| of the factor (the Hessian's measure, as tests/tools/fuzz_campaign.py)."""
    ref = np.asarray(ref, dtype=LD)
    d = np.abs(np.asarray(got, dtype=LD) - ref).max(axis=1)
    return np.asarray(d / np.abs(ref).max(axis=1), dtype=np.float64)


def per_regime(e, regime):
    """{regime name: largest of e over the factors of that regime} (the two 'base' slots merge)."""
    out = {}
    for r, name in enumerate(NAMES):
        sel = regime == r
        if sel.any():
            out[name] = max(out.get(name, 0.0), float(e[sel].max()))
    return out
