"""CPU: the inputs of tests/factor_cases.py and everything of the evaluateError sweeps that can be checked without a GPU, against
the long-double restatement there (NOT against the oracle, whose factor code is parity-unpinned):

  * the oracle (oracle/cpi_oracle.c: factor_eval) on every regime, both models;
  * tests/hostsim: the kernels' lane algebra compiled for the host -- the column functions of the dense sweep (hs.factor) and the
    block table of state_blocks_column with the Hessian's 3x3 block algebra (hs.hessian);
  * that no sign decision of these inputs is within rounding of zero (nothing has to be excluded from any comparison), that the
    regimes reach the paths they are there for, and that negating a state quaternion changes nothing.

Gates: 100 x the largest error measured (profiles/factor_edges.md holds the per-regime tables; pytest -s prints them)."""
import functools

import numpy as np
import pytest

from oracle import oracle_py as op
from tests import factor_cases as fc
from tests import hostsim_py as hs
from tests.tol import sqrt_info_longdouble

SIZES = [1, 3, 4, 5, 21, 22, 64, 257]          # tests/test_gpu_factor_edges.py (32768 + 5 there is mixed(257) tiled)
# measured (profiles/factor_edges.md), the larger of the two models: oracle 1.9e-15 / 5.5e-16 / 3.5e-16 (err / H1 / H2), hostsim
# 1.2e-15 / 6.1e-16 / 3.2e-16, hostsim Hessian 7.7e-16 of max |M|
GATE_ORACLE = 1.9e-13
GATE_HOSTSIM = 1.2e-13
GATE_HOSTSIM_HESSIAN = 7.7e-14


@functools.lru_cache(maxsize=None)
def _case(model):
    b = fc.mixed(model, 257)
    ref = fc.evaluate_error_longdouble(model, b["rec"], b["xi"], b["xj"], details=True)
    return b, ref


def _table(title, cols):
    """cols: {output: per-factor error [F]} -> printed per regime; returns the largest of each column."""
    names = list(dict.fromkeys(fc.NAMES))
    print("\n%s\n%-20s %s" % (title, "regime", " ".join("%10s" % c for c in cols)))
    per = {c: fc.per_regime(e, np.arange(len(e)) % len(fc.REGIMES)) for c, e in cols.items()}
    for n in names:
        print("%-20s %s" % (n, " ".join("%10.1e" % per[c][n] for c in cols)))
    print("%-20s %s" % ("largest", " ".join("%10.1e" % float(e.max()) for e in cols.values())))
    return {c: float(e.max()) for c, e in cols.items()}


def test_mixed_is_seeded_and_every_size_is_a_head_of_the_largest():
    assert len(fc.REGIMES) % 2 and len(fc.REGIMES) % 3
    for model in (1, 2):
        big = fc.mixed(model, 257)
        again = fc.mixed(model, 257)
        for F in SIZES:
            b = fc.mixed(model, F)
            for k in ("rec", "xi", "xj", "regime", "base"):
                assert np.array_equal(b[k], big[k][:F]), (model, F, k)
                assert np.array_equal(again[k], big[k])
        # every wavefront is a mix: 4 consecutive factors are 4 different regimes
        assert all(len(set(big["regime"][k:k + 4])) == 4 for k in range(0, 256, 4))


@pytest.mark.parametrize("model", [1, 2])
def test_no_case_has_to_be_excluded(model):
    """The exclusion rule: a case may be left out of a comparison only when a sign decision of the reference (the w of the five
    quaternion products and of rot_2_quat before its flip) is below 1e-9 -- and for these inputs that is NO case.  If a seed ever
    falls below, change the seed (factor_cases.SEED), not the rule."""
    for F in SIZES:
        b = fc.mixed(model, F)
        margin = fc.evaluate_error_longdouble(model, b["rec"], b["xi"], b["xj"])[3]
        excluded = int((margin < fc.MARGIN_MIN).sum())
        print("model %d F %d: smallest margin %.2e (%s), excluded %d" % (model, F, margin.min(), fc.NAMES[b["regime"][margin.argmin()]], excluded))
        assert excluded == 0


@pytest.mark.parametrize("model", [1, 2])
def test_the_regimes_reach_what_they_are_for(model):
    b, ref = _case(model)
    det, err, H2 = ref[4], ref[0], ref[2]
    reg = np.array(fc.NAMES)[b["regime"]]
    flip = det["flip"]
    # the flip of quat_multiply in each of the four products of the residual, in the regimes built for it and NOT in base -- q_n
    # excepted: q_j (x) q_i^-1 of two quaternions that each have w >= 0 comes out with w < 0 wherever the double cover put them on
    # different sheets, near the prediction too.  The products after it (w ~ 1 near the prediction) are the ones base never flips.
    for k in ("q_rminus", "q_r", "q_m"):
        assert not flip[k][reg == "base"].any(), k
    assert flip["q_r"].any() and flip["q_rminus"].any() and flip["q_m"][np.char.startswith(reg, "qb")].any()
    pos = np.arange(257) % 4                         # q_n: every position of a 4-factor wavefront sees a flipped and an unflipped factor
    assert all(flip["q_n"][pos == p].any() and (~flip["q_n"][pos == p]).any() for p in range(4))
    for k, least in (("q_rminus", 8), ("q_r", 5), ("q_m", 3), ("q_b", 5)):      # the rarer ones: often enough, in more than one position
        assert flip[k].sum() >= least and len(set(pos[flip[k]])) >= 2, (k, int(flip[k].sum()))
    assert flip["q_r"][:64].any() and flip["q_rminus"][:21].any() and flip["q_n"][:21].any()      # the small sizes too
    if model == 2:
        assert flip["q_kR"].any()
    # rot_2_quat: the three diagonal branches next to pi, the trace branch elsewhere; Exp_so3 at exactly zero
    near_pi = ("qb(2.5)", "qb(3.141)", "resrot(2.5)+qb(2.5)", "qb_axis(3.141)")
    for name in near_pi:
        assert set(det["branch"][reg == name]) == {0, 1, 2}, name
    assert set(det["branch"][~np.isin(reg, near_pi)]) == {3}
    assert np.all(det["angle_b"][reg == "qb(0)"] == 0.0)
    a = det["angle_b"]
    assert np.all(a[reg == "qb(1e-09)"] < 2e-9) and np.all(a[reg == "qb(1e-09)"] > 0)
    # sincos_fast: both sides of the 0.25 switch, the long polynomial (<= 1) and the reduced path (> 1)
    assert np.all((a[reg == "qb(0.2)"] > 0.19) & (a[reg == "qb(0.2)"] < 0.25)) and np.all((a[reg == "qb(0.3)"] > 0.25) & (a[reg == "qb(0.3)"] < 1))
    assert np.all(a[np.isin(reg, ("qb(1.5)", "qb(2.5)", "qb(3.141)", "resrot(2)+qb(1.5)", "resrot(2.5)+qb(2.5)", "qb_axis(3.141)"))] > 1.0)
    # magnitudes: residuals of O(1e4), positions of O(5e6), H2(0,0) = q_r,w I + [q_r,v]x near I at base and far from it next to pi
    e = np.abs(np.asarray(err, dtype=np.float64))
    assert e[reg == "bigres"].max() > 1e4 and np.abs(b["xi"][reg == "utm", 13:16]).max() > 1e6
    H200 = np.asarray(H2, dtype=np.float64).reshape(-1, 15, 15)[:, 0:3, 0:3]
    assert np.abs(H200[np.char.startswith(reg, "resrot(3")] - np.eye(3)).max(axis=(1, 2)).min() > 0.5
    assert np.abs(H200[reg == "base"] - np.eye(3)).max() < 0.05
    # f32quat: unit to float32 rounding only
    n = np.linalg.norm(b["xi"][reg == "f32quat", 0:4], axis=1)
    assert np.abs(n - 1).max() < 1.2e-7 and np.abs(n - 1).max() > 1e-9


@pytest.mark.parametrize("model", [1, 2])
def test_oracle_against_the_longdouble_restatement(model):
    b, ref = _case(model)
    err, H1, H2 = op.oracle().factor(model, b["rec"], b["xi"], b["xj"])
    worst = _table("oracle vs long double, model %d" % model,
                   dict(err=fc.rel_err(err, ref[0]), H1=fc.rel_err(H1, ref[1]), H2=fc.rel_err(H2, ref[2])))
    assert max(worst.values()) <= GATE_ORACLE, worst
    e0, _, _ = op.oracle().factor(model, b["rec"], b["xi"], b["xj"], want_H=False)
    assert np.array_equal(e0, err)


@pytest.mark.parametrize("model", [1, 2])
def test_hostsim_columns_against_the_longdouble_restatement(model):
    b, ref = _case(model)
    err, H1, H2 = hs.factor(model, b["rec"], b["xi"], b["xj"])
    worst = _table("hostsim dense columns vs long double, model %d" % model,
                   dict(err=fc.rel_err(err, ref[0]), H1=fc.rel_err(H1, ref[1]), H2=fc.rel_err(H2, ref[2])))
    assert max(worst.values()) <= GATE_HOSTSIM, worst


@functools.lru_cache(maxsize=None)
def sqrt_info_of_base_cases(model):
    """R [320, 225] column-major: tol.sqrt_info_longdouble of the oracle's covariance of the base cases' windows."""
    bc = fc.base_cases(model)
    P = op.oracle().run(op.make_params(model, 0, 1), bc["knots"], bc["lin"], bc["q_k_lin"], nthreads=8)["P"]
    R = sqrt_info_longdouble(P.reshape(-1, 15, 15))
    return np.ascontiguousarray(R.transpose(0, 2, 1)).reshape(-1, 225)


@pytest.mark.parametrize("model", [1, 2])
def test_hostsim_hessian_blocks_against_the_longdouble_restatement(model):
    """state_blocks_column (the packed and Hessian kernels' copy of the column code) + the block algebra, against Hc^T (R^T R) Hc
    formed in long double from the reference's [H1 H2 -e]; R is a fixed double matrix, the realistic square-root information."""
    b, ref = _case(model)
    R = sqrt_info_of_base_cases(model)[b["base"]]
    got = hs.hessian(model, b["rec"], b["xi"], b["xj"], R)
    assert np.all(np.isfinite(got))
    worst = _table("hostsim Hessian vs long double (of max |M| of the factor), model %d" % model,
                   dict(M=fc.rel_err_scaled(got, fc.hessian_longdouble(ref, R))))
    assert worst["M"] <= GATE_HOSTSIM_HESSIAN, worst


@pytest.mark.parametrize("model", [1, 2])
def test_negated_state_quaternions_give_the_same_rows(model):
    """-q is the same rotation: every row of the negw regimes equals the row of the batch with the quaternions left alone -- bit for
    bit for the reference, the oracle and the host emulation (each product's sign is undone by its own flip, quat_2_Rot is even)."""
    b, ref = _case(model)
    p = fc.mixed(model, 257, negate=False)
    sel = np.isin(b["regime"], fc.NEGW)
    assert sel.sum() >= 30 and not np.array_equal(b["xi"][sel], p["xi"][sel]) and np.array_equal(b["xi"][~sel], p["xi"][~sel])
    ref0 = fc.evaluate_error_longdouble(model, p["rec"], p["xi"], p["xj"])
    for a, c in zip(ref[:3], ref0[:3]):
        assert np.array_equal(a, c)
    for fn in (lambda x: op.oracle().factor(model, x["rec"][sel], x["xi"][sel], x["xj"][sel]),
               lambda x: hs.factor(model, x["rec"][sel], x["xi"][sel], x["xj"][sel])):
        for a, c in zip(fn(b), fn(p)):
            assert np.array_equal(a, c)
