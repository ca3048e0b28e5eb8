"""GPU: cpi_state_fix_batch at the edges of its contract -- the builders of tests/fix_cases.py that leave the comfortable range (GPS-sized
positions, float32-rounded and scaled quaternions, a residual rotation of exactly zero, 1027 states in 257 workgroups), a broken mfirst
on the device, and one NaN in every place it can sit.  What must come back is stated once in tests/fix_edge_checks.py, for the host
twin (tests/test_fix_cpu.py, where each check is also shown to fail on a twin with the defect it is there for) and for the device alike.
The figures of a comparison are printed before anything is asserted; the gates are those of tests/fix_cases.py."""
import os

import numpy as np
import pytest
import torch

import cpi_amd
from tests import fix_cases as fx
from tests import fix_edge_checks as fe
from tests import test_fix_cpu as tf
from tests.test_gpu_fix import _t, dev_fix
from tests.test_lm_cpu import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


@pytest.fixture(scope="module")
def hf():
    if (not os.path.exists(tf._LIB)) or os.path.getmtime(tf._LIB) < max(os.path.getmtime(p) for p in (tf._SRC, tf._MATH)):
        tf.tm._build(tf._SRC, tf._LIB)
    return tf._bind(tf._LIB)


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name,kind", tf.EDGE_CASES, ids=["%s-%s" % (n, fx.KINDS[k]) for n, k in tf.EDGE_CASES])
def test_edge_builders_against_the_reference(eng, hf, name, kind):
    c = fx.edge_case(name, kind)
    worst, full = {}, None
    for weight, base in ((True, True), (False, False)):
        out, pcost, chi2 = dev_fix(eng, c, weight, base)
        assert not np.isnan(out).any() and not np.isnan(pcost).any() and not np.isnan(chi2).any()
        assert (out[:, 135] == 0.0).all()
        full = (out, pcost, chi2) if full is None else full
        for k, v in fx.metrics(out, pcost, chi2, fx.reference(c, weight, base)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("device, %s, %s: %s (gates %s)" % (name, fx.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), fx.GATE_DEVICE))
    for k, v in worst.items():
        assert v <= fx.GATE_DEVICE[k], (k, v)
    if kind < 2:                                                              # no quaternion in it: the twin's bits
        for weight, base in ((True, True), (False, False)):
            assert all(same_bits(a, b) for a, b in zip(dev_fix(eng, c, weight, base), tf.twin(hf, c, weight, base))), (weight, base)
    if name == "many":                                                        # a state's bits: not S, nor where it sits
        out, pcost, chi2 = full
        o, p, x2 = dev_fix(eng, c.head(9))
        assert same_bits(o, out[:9]) and same_bits(p, pcost[:9]) and same_bits(x2, chi2[:len(x2)])
        mv, order, fixes = fx.reversed_case(c)
        o, p, x2 = dev_fix(eng, mv)
        assert same_bits(o, np.ascontiguousarray(out[order])) and same_bits(p, np.ascontiguousarray(pcost[order])) and same_bits(x2, np.ascontiguousarray(chi2[fixes]))


# ------------------------------------------------------------------------------------------ 2. exact zero residual
@pytest.mark.parametrize("kind", [2, 3], ids=fx.KINDS[2:])
def test_exact_zero_residual(eng, kind):
    m = fe.check_exact_zero(lambda c: dev_fix(eng, c), kind)
    for k, v in m.items():
        assert v <= fx.GATE_DEVICE[k], (k, v)


# ------------------------------------------------------------------------------------------ 3. broken mfirst
def dev_padded(eng, p, mfirst):
    """state_fix on the interiors of the padded arrays of fe.Padded -> the whole buffers (out, pcost, chi2) as numpy."""
    c, P, dev = p.c, fe.PAD, eng.device
    big = {k: _t(v, dev) for k, v in p.big.items()}
    out = torch.full((c.S + 2, 136), float("nan"), dtype=torch.float64, device=dev)
    pcost = torch.full((c.S + 2,), float("nan"), dtype=torch.float64, device=dev)
    out[0], out[-1], pcost[0], pcost[-1] = fe.GUARD, fe.GUARD, fe.GUARD, fe.GUARD
    inner = lambda t: t[P:P + c.M]
    eng.state_fix(_t(c.states, dev), c.kind, inner(big["z"]), inner(big["R"]), _t(np.asarray(mfirst, dtype=np.int64), dev), weight=inner(big["weight"]),
                  base=_t(c.base, dev), pcost_base=_t(c.pcost_base, dev), out=out[1:-1], pcost=pcost[1:-1], chi2=inner(big["chi2"]))
    torch.cuda.synchronize()
    for name in ("z", "R", "weight"):                                         # the inputs as they went in
        assert same_bits(big[name].cpu().numpy(), p.big[name])
    return out.cpu().numpy(), pcost.cpu().numpy(), big["chi2"].cpu().numpy()


@pytest.mark.parametrize("kind", [0, 3], ids=["position", "pose"])
def test_broken_mfirst_stays_inside(eng, kind):
    """include/cpi_amd.h: "a broken mfirst gives unspecified contents, no access out of bounds".  Every broken value stays within
    pads that belong to the test, so a kernel without the clamp would read a NaN or write over a guard: a failure, not a fault."""
    fe.check_broken_mfirst(lambda p, mf: dev_padded(eng, p, mf), kind)
    c = fx.case(kind, 9)
    for what, mf, _ in fe.broken_mfirsts(c):                                  # the host form refuses each of them, naming a state
        bad = fe.variant(c, mfirst=mf)
        with pytest.raises(cpi_amd.CpiError, match=r"the fixes of state \d+ "):
            dev_fix(eng, bad, host=True)


# ------------------------------------------------------------------------------------------ 4. NaN stays where it is
@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_nan_stays_where_it_is(eng, kind):
    assert fe.check_nan_locality(lambda c: dev_fix(eng, c), kind) >= 24
