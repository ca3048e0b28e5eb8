"""CPU: cpi_state_between_batch at the edges of its contract, on the host twin tests/hostsim/hostsim_between.cpp.  What must come back is
stated once in tests/between_edge_checks.py, for the twin and for the device (tests/test_gpu_between_edges.py) alike; here every check
also runs on a twin with the defect it is there for, built in tmp_path, and must fail on it.  The twin is held to GATE_EDGE_HOST of
tests/between_cases.py or to bits; the figures of a comparison are printed before anything is asserted.

What the twin cannot carry, because it has no such code path, is not pretended: it moves no 16-byte pieces, so nothing here stands for
the alignment test of the device (btw_d2u, st16_nt), and it has no lanes, lane groups or workgroups, so check_many shows on it only that
a factor's bits are its own data's -- a lane-mapping defect exists on the device alone.  The twin decides "in place" per factor by
comparing the row's pointer with the base's (chn::factor_between) and takes chi2_base by value; the defect "in place decided on chi2"
is therefore put where the twin forms those pointers (hostsim_between.cpp): when chi2 is in place, the row is taken for its own base."""
import re
import time

import numpy as np
import pytest

from tests import between_cases as bc
from tests import between_edge_checks as be
from tests import fix_cases as fx
from tests.test_between_cpu import _err, _mutant, _ptr, hb, lib, twin  # noqa: F401  (hb, lib: fixtures)

LD = np.longdouble
GATE = bc.GATE_EDGE_HOST


def run_on(h):
    return lambda c, **form: twin(h, c, **form)


def _hold(m, gate, what):
    for k, v in m.items():
        assert v <= gate[k], (what, k, v)


# ---------------------------------------------------------------- the inputs
def test_the_edge_inputs_are_honest():
    """identity: unit quaternions [0, 0, 0, 1], positions on the grid, the longdouble residual exactly 0; pi: the longdouble qd.w exactly
    0 and e_th = +-2 on one axis, all six of PI_Z present; scaled: norms 0.5, 3 and 1e-150; long: a fold of 300 whose reference takes
    a few seconds at most; many: 257 workgroups, the last with three live factors, the first nine pairs those of the explicit variant."""
    for name, kinds in bc.EDGE_BUILDERS:
        for kind in kinds:
            c = bc.edge_case(name, kind)
            fi, fj = c.pairs()
            own = c.owner()
            if name in ("identity", "pi"):
                assert (c.states[:, :4] == [0, 0, 0, 1]).all() and (c.states[:, 13:16] * 4 == np.round(c.states[:, 13:16] * 4)).all()
                for m in range(c.M):
                    xi, xj = c.states[fi[own[m]]], c.states[fj[own[m]]]
                    e = bc.residual_ld(kind, xi, xj, c.z[m])[0]
                    if name == "identity":
                        assert (e == 0).all(), (kind, m)
                    else:
                        rin = bc._unit_flip(*fx.quat_mul_ld(xj[:4], bc._inv(np.asarray(xi[:4], dtype=LD))))[0]
                        qd = fx.quat_mul_ld(c.z[m, :4], bc._inv(rin))[0]
                        assert qd[3] == 0 and sorted(np.abs(e[:3])) == [0, 0, 2], (kind, m, qd)
                        assert np.array_equal(np.asarray(e[:3], dtype=np.float64), 2 * c.z[m, :3])                 # taken as it is: never negated
                        if kind == 2:
                            assert (e[3:] != 0).all() and (bc.unpack_R(c.R[m], 6, np.float64) == np.diag(np.diag(bc.unpack_R(c.R[m], 6, np.float64)))).all()
                if name == "pi":
                    assert len(set(map(tuple, c.z[:, :4]))) == 6 and all(len(set(map(tuple, c.z[c.mfirst[f]:c.mfirst[f + 1], :4]))) == 6 for f in (0, 5))
            if name == "scaled":
                n = np.linalg.norm(c.z[:, :4], axis=1)
                assert all((np.abs(n / s - 1) < 1e-12).any() for s in bc.Z_SCALES)
            if name == "long":
                assert tuple(c.counts) == (0, 300, 1, 33, 0) == bc.LONG_COUNTS
                t0 = time.perf_counter()
                bc.edge_reference("long", kind)
                took = time.perf_counter() - t0
                print("long, %s: the reference of %d measurements took %.2f s" % (bc.KINDS[kind], c.M, took))
                assert took < 5.0
            if name == "many":
                assert c.F == 1027 and (c.F + 3) // 4 == 257 and c.F - 4 * 256 == 3 and c.S == bc.MANY_S and (c.idx_i != c.idx_j).all()
                assert tuple(c.idx_i[:9]) == bc.IDX_I and tuple(c.idx_j[:9]) == bc.IDX_J and c.idx_j.max() == c.S - 1 and c.idx_i.min() == 0
                assert set(c.counts.tolist()) == {0, 1, 2, 17}
    for kind in range(3):                                                     # the breaks stay inside the pads, by construction
        c, x = bc.case(kind, 9), bc.case(kind, 9, "explicit")
        for _, bad, f in be.broken_mfirsts(c):
            assert bad.mfirst.min() > -be.PAD and bad.mfirst.max() < c.M + be.PAD and 0 <= f < c.F
        for _, bad, f in be.broken_indices(x):
            assert min(bad.idx_i.min(), bad.idx_j.min()) >= -be.PADS and max(bad.idx_i.max(), bad.idx_j.max()) < x.S + be.PADS


# ---------------------------------------------------------------- 1. broken mfirst, broken indices
@pytest.mark.parametrize("kind", [0, 2], ids=["position", "pose"])
def test_twin_broken_mfirst_and_indices_stay_inside(hb, lib, kind):
    c, x = bc.case(kind, 9), bc.case(kind, 9, "explicit")
    assert be.check_broken(run_on(hb), c, be.broken_mfirsts(c)) == 2                # (-3 and M + 3 clamp to the sound call itself)
    assert be.check_broken(run_on(hb), x, be.broken_indices(x)) == 4
    for what, bad, f in be.broken_mfirsts(c) + be.broken_indices(x):         # the host entry refuses each of them, naming the factor
        a = [np.ascontiguousarray(v) if v is not None else None for v in (bad.mfirst, bad.states, bad.idx_i, bad.idx_j, bad.z, bad.R, bad.weight, bad.base,
                                                                         bad.chi2_base, np.zeros((bad.F, 496)), np.zeros(bad.F), np.zeros(bad.M))]
        rc = lib.cpi_state_between_batch_host(None, bad.F, bad.M, kind, _ptr(a[0]), _ptr(a[1]), bad.S, *[_ptr(v) for v in a[2:]])
        print("%s: %s" % (what, _err(lib)))
        text = ("the measurements of factor %d leave [0, M] or mfirst decreases there" if "mfirst" in what else "state index out of range at factor %d") % f
        assert rc == 1 and _err(lib) == "cpi_state_between_batch_host: " + text, what


# ---------------------------------------------------------------- 3. mixed aliasing
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_mixed_aliasing(hb, kind):
    be.check_mixed_aliasing(run_on(hb), kind)


# ---------------------------------------------------------------- 4. NaN locality
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_nan_stays_where_it_is(hb, kind):
    assert be.check_nan_locality(run_on(hb), kind) == be.nan_calls(kind) >= 52


# ---------------------------------------------------------------- 5. exact residuals
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_exact_zero_residual(hb, kind):
    _hold(be.check_identity(run_on(hb), kind), GATE["identity"], "identity")


@pytest.mark.parametrize("kind", [1, 2], ids=bc.KINDS[1:])
def test_twin_rotations_of_exactly_pi(hb, kind):
    _hold(be.check_pi(run_on(hb), kind), GATE["pi"], "pi")


@pytest.mark.parametrize("kind", [1, 2], ids=bc.KINDS[1:])
def test_twin_scaled_quaternions(hb, kind):
    _hold(be.check_scaled(run_on(hb), kind), GATE["scaled"], "scaled")


# ---------------------------------------------------------------- 6. weight 0, long folds, position in the grid
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_weight_zero_removes_a_measurement_exactly(hb, kind):
    be.check_weight_zero(run_on(hb), kind)


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_long_fold(hb, kind):
    _hold(be.check_long(run_on(hb), kind), GATE["long"], "long")


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_many_factors(hb, kind):
    be.check_many(run_on(hb), kind)


# ---------------------------------------------------------------- each check fails on the defect it is there for
_CLAMP = "long long clampM(long long v, long long M) { return v < 0 ? 0 : (v > M ? M : v); }"
_BASE = "weight ? weight + m0 : nullptr, hess_base ? hess_base + f * 496 : nullptr,"
EDGE_MUTATIONS = {
    "a missing clamp, broken mfirst": (_CLAMP, "long long clampM(long long v, long long M) { return v; }", True,
                                       lambda h: be.check_broken(run_on(h), bc.case(0, 9), be.broken_mfirsts(bc.case(0, 9)))),
    "a missing clamp, broken indices": (_CLAMP, "long long clampM(long long v, long long M) { return v; }", True,
                                        lambda h: be.check_broken(run_on(h), bc.case(2, 9, "explicit"), be.broken_indices(bc.case(2, 9, "explicit")))),
    "in place decided on chi2 instead of hess": (_BASE, "weight ? weight + m0 : nullptr, (chi2 && chi2 == chi2_base && hess) ? hess + f * 496 : "
                                                        "(hess_base ? hess_base + f * 496 : nullptr),", True, lambda h: be.check_mixed_aliasing(run_on(h), 2)),
    "p read for the orientation kind": ("g.qji = quat_inv(quat_multiply(xj.q, quat_inv(xi.q)));",
                                        "g.qji = quat_inv(quat_multiply(xj.q, quat_inv(xi.q))); g.qji.x += 0.0 * (xj.p.x - xi.p.x);", False,
                                        lambda h: be.check_nan_locality(run_on(h), 1)),
    "the qd.w < 0 test turned into <=": ("if (r.w < 0) {", "if (r.w <= 0) {", False, lambda h: _hold(be.check_pi(run_on(h), 1), GATE["pi"], "pi")),
    "the weight applied to chi2_m, NaN weight": ("if (chi2_m) chi2_m[m] = c2;", "if (chi2_m) chi2_m[m] = w * c2;", False,
                                                 lambda h: be.check_nan_locality(run_on(h), 0)),
    "the weight applied to chi2_m, weight 0": ("if (chi2_m) chi2_m[m] = c2;", "if (chi2_m) chi2_m[m] = w * c2;", False,
                                               lambda h: be.check_weight_zero(run_on(h), 0)),
    "a residual that is never exactly zero": ("const Q4 qd = quat_multiply(ldq(z), g.qji);\n        e[0] = 2 * qd.x;", "const Q4 qd = quat_multiply(ldq(z), g.qji);\n        e[0] = 2 * qd.x + 1e-160;", False,
                                              lambda h: be.check_identity(run_on(h), 1)),
    "a fold that forgets its last measurement": ("        for (long long m = 0; m < n; m++) {\n            const double *Rm = R + m * T::RN, w = weight",
                                                 "        for (long long m = 0; m < n - (n > 32); m++) {\n            const double *Rm = R + m * T::RN, w = weight",
                                                 False, lambda h: _hold(be.check_long(run_on(h), 0), GATE["long"], "long")),
    "a factor that reads its neighbour's base chi2": ("chi2_base ? chi2_base[f] : 0.0,", "chi2_base ? chi2_base[f > 999 ? f - 1 : f] : 0.0,", True,
                                                      lambda h: be.check_many(run_on(h), 0)),
}


@pytest.mark.parametrize("what", list(EDGE_MUTATIONS))
def test_the_edge_checks_fail_when_they_should(hb, tmp_path, what):
    """The twin with one defect, built in tmp_path: the check named in EDGE_MUTATIONS passes on the twin and fails on the mutant.  (The
    padded arrays keep a twin without the clamp inside its allocations: it reads a NaN pad or writes over a guard.)"""
    old, new, in_twin, check = EDGE_MUTATIONS[what]
    mutant = _mutant(tmp_path, old, new, twin=in_twin)
    check(hb)
    with pytest.raises(AssertionError) as info:
        check(mutant)
    print("%s: the mutant fails with %s" % (what, re.sub(r"\s+", " ", str(info.value))[:200]))
