"""GPU: the evaluateError sweeps away from the predicted state -- cpi_factor_eval_batch (H1 / H2 out and err alone),
cpi_factor_eval_packed_batch, cpi_factor_eval_whitened_[tri_]batch and cpi_factor_hessian_[tri_]batch on tests/factor_cases.mixed():
residual rotations through pi (the flip of quat_multiply in q_n, q_rminus, q_r), bias steps that take q_b through Exp_so3 at zero, both
sides of the 0.25 rad switch of sincos_fast, its reduced path, the three diagonal branches of rot_2_quat and the flip in q_m, negated
and float32-rounded state quaternions, positions of 5e6 m and residuals of 1e4 -- every wavefront a mix of them.

The reference is the long-double restatement of tests/factor_cases.py on exactly the doubles the device is given (for the whitened
and Hessian forms that includes R: Engine.sqrt_information of the windows' covariance, read back and used as given).  No case is
excluded from any comparison (tests/test_factor_cases_cpu.py::test_no_case_has_to_be_excluded).

Gates: the contractual TOL_FACTOR x max(1, max |ref| of the factor's output) (Hessian: 1e-12 of max |M| of the factor, as
tests/test_gpu_whitening.py), and REG: 100 x the largest error measured on an MI355X against the long-double reference per output group
and model (profiles/factor_edges.md, which also holds the per-regime tables; pytest -s prints them)."""
import functools

import numpy as np
import pytest
import torch

import cpi_amd
from tests import factor_cases as fc
from tests.tol import TOL_FACTOR

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 21, 22, 64, 257]      # one factor; 4-factor wavefronts -1 / 0 / +1; the packed sweep's 21 and 22; blocks + ragged tail
F_8LANE = 32768 + 5                        # cpi_abi.hip: factor_lanes() picks the 8-lane dense kernel from 32768 factors up
TOL_HESSIAN = 1e-12
# 100 x the floors of profiles/factor_edges.md (MI355X, against the long-double reference), model 1 | model 2: err, H1, H2 of the dense /
# packed sweeps (floors 6.4e-16, 3.0e-16, 3.3e-16 | 1.4e-15, 8.0e-16, 3.8e-16), the whitened outputs together (1.0e-14 | 2.1e-14, in R e
# of the regimes near the prediction: a small residual against rows of R of 1e4 and more), the Hessian of max |M| (5.9e-16 | 7.5e-16)
# and the residual of the predicted state (2.4e-15 | 2.6e-15).  None is looser than the contractual gate (_gate asserts it).
REG = {1: dict(err=6.4e-14, H1=3.0e-14, H2=3.3e-14, white=1.0e-12, hess=5.9e-14, predict=2.4e-13),
       2: dict(err=1.4e-13, H1=8.0e-14, H2=3.8e-14, white=2.1e-12, hess=7.5e-14, predict=2.6e-13)}


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _dev(a, eng):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(eng.device)       # a copy: the cases are read-only


@functools.lru_cache(maxsize=None)
def _sqrt_info(eng, model):
    """R [320, 225] and its packed triangle [320, 120] of the base cases' windows, on the device, + R read back."""
    bc = fc.base_cases(model)
    out = eng.preintegrate(_dev(bc["knots"], eng), _dev(bc["lin"], eng), _dev(bc["q_k_lin"], eng), eng.make_params(model),
                           want=("cov", "cov_sym"))
    R, Rt = eng.sqrt_information(out["P"]), eng.sqrt_information(out["P_sym"])
    torch.cuda.synchronize()
    assert torch.equal(cpi_amd.unpack_tri(Rt), R) and bool(torch.isfinite(R).all())
    return R, Rt, R.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(eng, model, negate=True):
    """mixed(257) and the long-double reference of every form for it -- computed once, shared and never written to."""
    b = fc.mixed(model, 257, negate=negate)
    R = _sqrt_info(eng, model)[2][b["base"]]
    ref = fc.evaluate_error_longdouble(model, b["rec"], b["xi"], b["xj"])
    assert (ref[3] >= fc.MARGIN_MIN).all()
    return b, dict(err=ref[0], H1=ref[1], H2=ref[2], white=fc.whitened_longdouble(ref, R), hess=fc.hessian_longdouble(ref, R))


class Inputs:
    """The first F factors of mixed(257) (rows `rows` of it, default arange(F)) on the device: states shuffled into one array and
    gathered through idx_i / idx_j (gather=False: xi then xj, idx = f and F + f)."""

    def __init__(self, eng, model, F, gather=True, rows=None, negate=True):
        b = _reference(eng, model, negate)[0]
        rows = np.arange(F) if rows is None else np.asarray(rows)
        F = rows.shape[0]
        self.F, self.model, self.rows = F, model, rows
        meas, lin, qlin = fc.meas_of(b["rec"][rows])
        self.meas = {k: _dev(v, eng) for k, v in meas.items()}
        self.lin, self.q = _dev(lin, eng), (_dev(qlin, eng) if model == 2 else None)
        st = np.concatenate([b["xi"][rows], b["xj"][rows]], axis=0)
        where = np.random.default_rng(1000 + F).permutation(2 * F) if gather else np.arange(2 * F)
        shuffled = np.empty_like(st)
        shuffled[where] = st
        self.states = _dev(shuffled, eng)
        self.ii, self.jj = _dev(where[:F].astype(np.int32), eng), _dev(where[F:].astype(np.int32), eng)
        R, Rt, _ = _sqrt_info(eng, model)
        sel = _dev(b["base"][rows], eng)
        self.R, self.Rt = R[sel].contiguous(), Rt[sel].contiguous()


def _run(eng, x, pad=1):
    """Every form of the sweep on x, each into a buffer `pad` factors longer and pre-filled; returns the buffers."""
    F, m = x.F, x.model
    big = lambda n: torch.full((F + pad, n), -7.0, dtype=torch.float64, device=eng.device)
    trio = lambda: {"err": big(15), "H1": big(225), "H2": big(225)}
    head = lambda d: {k: v[:F] for k, v in d.items()}
    o = dict(dense=trio(), eonly={"err": big(15)}, packed=big(72), white=trio(), white_tri=trio(), hess=big(496), hess_tri=big(496))
    a = (m, x.meas, x.lin, x.q, x.states)
    eng.factor_eval(*a, x.ii, x.jj, out=head(o["dense"]))
    eng.factor_eval(*a, x.ii, x.jj, want_H=False, out=head(o["eonly"]))
    eng.factor_eval_packed(*a, x.ii, x.jj, out=o["packed"][:F])
    eng.factor_eval(*a, x.ii, x.jj, sqrt_info=x.R, out=head(o["white"]))
    eng.factor_eval(*a, x.ii, x.jj, sqrt_info=x.Rt, out=head(o["white_tri"]))
    eng.factor_hessian(*a, x.R, x.ii, x.jj, out=o["hess"][:F])
    eng.factor_hessian(*a, x.Rt, x.ii, x.jj, out=o["hess_tri"][:F])
    torch.cuda.synchronize()
    return o


def _errors(eng, model, rows, dense, white=None, hess=None):
    """Per-factor errors of each output against the reference rows `rows`: {name: [F]}."""
    ref = _reference(eng, model)[1]
    h = lambda t: t.cpu().numpy()
    e = {k: fc.rel_err(h(dense[k]), ref[k][rows]) for k in dense}
    if white is not None:
        for i, k in enumerate(("err", "H1", "H2")):
            e["R " + k] = fc.rel_err(h(white[k]), ref["white"][i][rows])
    if hess is not None:
        e["hess"] = fc.rel_err_scaled(h(hess), ref["hess"][rows])
    return e


def _report(title, e, regime, table):
    if table:
        names = list(dict.fromkeys(fc.NAMES))
        per = {c: fc.per_regime(v, regime) for c, v in e.items()}
        print("\n%s\n%-20s %s" % (title, "regime", " ".join("%9s" % c for c in e)))
        for n in names:
            if all(n in per[c] for c in e):
                print("%-20s %s" % (n, " ".join("%9.1e" % per[c][n] for c in e)))
    print("%-20s %s" % (title if not table else "largest", " ".join("%s %.1e" % (c, float(v.max())) for c, v in e.items())))


def _gate(model, e):
    """The contractual gate and, where a floor has been measured, the regression gate of each output group."""
    bad = []
    for k, v in e.items():
        group = "hess" if k == "hess" else ("white" if k.startswith("R ") else k)
        tol = TOL_HESSIAN if group == "hess" else TOL_FACTOR
        reg = REG[model][group]
        assert reg is None or reg <= tol
        worst = float(v.max())
        if not worst <= (tol if reg is None else reg):
            bad.append("%s %.2e > %.1e (row %d)" % (k, worst, tol if reg is None else reg, int(v.argmax())))
    assert not bad, "model %d: %s" % (model, "; ".join(bad))


@pytest.mark.parametrize("F", SIZES)
@pytest.mark.parametrize("model", [1, 2])
def test_every_form_against_the_longdouble_reference(eng, model, F):
    """Dense err / H1 / H2, err alone, the packed sweep through unpack_factor, the whitened sweep and the Hessian blocks from dense
    and from packed R, gathered states -- and the bit rules between the forms, which until now were asserted near the prediction
    only: packed == dense, _tri_ == dense-R, want_H=False err == err of the full call; nothing written past F."""
    x = Inputs(eng, model, F)
    o = _run(eng, x)
    d = {k: v[:F] for k, v in o["dense"].items()}
    rows, regime = x.rows, x.rows % len(fc.REGIMES)
    e = _errors(eng, model, rows, d, {k: v[:F] for k, v in o["white"].items()}, o["hess"][:F])
    _report("model %d F %d" % (model, F), e, regime, table=(F == 257))
    _gate(model, e)
    # the bit rules
    assert torch.equal(o["eonly"]["err"][:F], d["err"])
    pe, pH1, pH2 = cpi_amd.unpack_factor(o["packed"][:F], x.meas)
    assert torch.equal(pe, d["err"]) and torch.equal(pH1, d["H1"]) and torch.equal(pH2, d["H2"])
    for k in ("err", "H1", "H2"):
        assert torch.equal(o["white_tri"][k], o["white"][k]), k
    assert torch.equal(o["hess_tri"], o["hess"])
    # unwritten neighbours
    for name, t in (("dense", o["dense"]), ("eonly", o["eonly"]), ("white", o["white"]), ("white_tri", o["white_tri"])):
        for k, v in t.items():
            assert torch.all(v[F:] == -7.0), (name, k)
    for name in ("packed", "hess", "hess_tri"):
        assert torch.all(o[name][F:] == -7.0), name


@pytest.mark.parametrize("model", [1, 2])
def test_a_permutation_of_the_factors_permutes_the_rows(eng, model):
    """A factor's bits do not depend on its place in the wavefront, on its neighbours' regimes or on where its states sit: the
    257 factors in another order, states contiguous instead of gathered, give the same rows in that order -- every form."""
    F = 257
    a = _run(eng, Inputs(eng, model, F))
    perm = np.random.default_rng(77).permutation(F)
    assert len(set((perm % 4 - np.arange(F) % 4) % 4)) == 4            # factors change their position in the wavefront
    b = _run(eng, Inputs(eng, model, F, gather=False, rows=perm))
    p = torch.from_numpy(perm).to(eng.device)
    for name in a:
        for k in (a[name] if isinstance(a[name], dict) else [None]):
            u, v = (a[name], b[name]) if k is None else (a[name][k], b[name][k])
            assert torch.equal(u[:F][p], v[:F]), (name, k)


@pytest.mark.parametrize("model", [1, 2])
def test_the_eight_lane_dense_kernel(eng, model):
    """F = 32768 + 5: the 8-lane launch of the plain dense sweep (H1 / H2 out and err alone), mixed(257) tiled with gathered states.
    Every tile of 257 rows is, bit for bit, the first one, and the first one is, bit for bit, what the 16-lane launch gives for these
    257 factors alone; that one is compared with the long-double reference."""
    x = Inputs(eng, model, 257)
    t = torch.arange(F_8LANE, device=eng.device) % 257
    meas = {k: v[t].contiguous() for k, v in x.meas.items()}
    lin, q = x.lin[t].contiguous(), (None if x.q is None else x.q[t].contiguous())
    ii, jj = x.ii[t].contiguous(), x.jj[t].contiguous()
    big = {k: torch.full((F_8LANE + 1, n), -7.0, dtype=torch.float64, device=eng.device) for k, n in (("err", 15), ("H1", 225), ("H2", 225))}
    eng.factor_eval(model, meas, lin, q, x.states, ii, jj, out={k: v[:F_8LANE] for k, v in big.items()})
    eonly = eng.factor_eval(model, meas, lin, q, x.states, ii, jj, want_H=False)
    small = eng.factor_eval(model, x.meas, x.lin, x.q, x.states, x.ii, x.jj)
    torch.cuda.synchronize()
    e = _errors(eng, model, x.rows, {k: v[:257] for k, v in big.items()})
    _report("model %d 8-lane" % model, e, x.rows % len(fc.REGIMES), table=False)
    _gate(model, e)
    full = (F_8LANE // 257) * 257
    for k, v in big.items():
        assert torch.all(v[F_8LANE:] == -7.0), k
        assert torch.equal(v[:257], small[k]), k                                             # 8 lanes == 16 lanes
        assert bool((v[:full].view(-1, 257, v.shape[1]) == v[:257]).all()), k
        assert torch.equal(v[full:F_8LANE], v[:F_8LANE - full]), k
    assert torch.equal(eonly["err"], big["err"][:F_8LANE])


@pytest.mark.parametrize("model", [1, 2])
def test_negated_state_quaternions_give_the_same_rows(eng, model):
    """-q is the same rotation.  BIT FOR BIT in every form (measured; the stronger of the two statements): each quaternion product's
    sign is undone by its own flip, and qrot is even in q."""
    b = _reference(eng, model)[0]
    rows = np.nonzero(np.isin(b["regime"], fc.NEGW))[0]
    assert rows.size >= 30
    a = _run(eng, Inputs(eng, model, 0, rows=rows))
    p = Inputs(eng, model, 0, rows=rows, negate=False)
    assert not torch.equal(p.states, Inputs(eng, model, 0, rows=rows).states)
    c = _run(eng, p)
    for name in a:
        for k in (a[name] if isinstance(a[name], dict) else [None]):
            u, v = (a[name], c[name]) if k is None else (a[name][k], c[name][k])
            assert torch.equal(u, v), (name, k)


@pytest.mark.parametrize("model", [1, 2])
def test_prediction_at_the_edge_of_qb(eng, model):
    """State i with the gyro bias stepped by qb(phi) (every phi of the table; accelerometer bias and, model 2, orientation on the
    linearisation point), state j = Engine.predict(state i), then the residual.  At phi = 0 exactly -- Exp_so3's zero case, the
    1e-280 clamp of mag_and_inverse on the device -- that residual is zero; elsewhere it is the bias step seen through q_b and the
    bias Jacobians.  Gate: against the same composition in long double (prediction NOT rounded to double in between), so the floor
    rests on the rounding of the predicted p_j (O(10) m: half an ulp is 1.8e-15) and v_j to double, which R_k carries into the
    alpha / beta rows; the contractual TOL_FACTOR x max(1, max |ref|) applies, and REG's gate of this composition."""
    b = _reference(eng, model)[0]
    reg = np.array(fc.NAMES)[b["regime"]]
    rows = np.nonzero(np.char.startswith(reg, "qb("))[0]
    rec, xi = b["rec"][rows], b["xi"][rows].copy()
    xi[:, 10:13] = rec[:, fc.C_BA]
    if model == 2:
        xi[:, 0:4] = rec[:, fc.C_QLIN]
    meas, lin, qlin = fc.meas_of(rec)
    meas = {k: _dev(v, eng) for k, v in meas.items()}
    xi_d = _dev(xi, eng)
    xj_d = eng.predict(model, meas, xi_d)
    F = rows.size
    states = torch.cat([xi_d, xj_d], dim=0).contiguous()
    ii = torch.arange(F, dtype=torch.int32, device=eng.device)
    err = eng.factor_eval(model, meas, _dev(lin, eng), _dev(qlin, eng) if model == 2 else None, states, ii, ii + F, want_H=False)["err"]
    torch.cuda.synchronize()
    xj_l = fc.predict_longdouble(model, rec, xi)
    ref = fc.evaluate_error_longdouble(model, rec, xi, xj_l)
    assert (ref[3] >= fc.MARGIN_MIN).all()
    assert fc.rel_err(xj_d.cpu().numpy(), xj_l).max() <= TOL_FACTOR
    e = fc.rel_err(err.cpu().numpy(), ref[0])
    _report("model %d predict + residual" % model, {"predict": e}, b["regime"][rows], table=True)
    zero = reg[rows] == "qb(0)"
    # "zero": the double quaternion of state i is unit to 1e-16 only and quat_2_Rot does not normalise, so R_k R_k^-1 beta - beta is
    # O(1e-16 |beta|) in exact arithmetic too (reference: <= 1.3e-15 over these cases); the device's residual stays within the gate of 0
    got0 = float(np.abs(err.cpu().numpy()[zero]).max())
    print("largest |residual| at phi = 0: reference %.1e, device %.1e" % (np.abs(np.asarray(ref[0], dtype=np.float64)[zero]).max(), got0))
    assert zero.sum() >= 10 and np.abs(np.asarray(ref[0], dtype=np.float64)[zero]).max() < 1e-14
    _gate(model, {"predict": e})
    assert got0 <= (REG[model]["predict"] or TOL_FACTOR) + 1e-14
