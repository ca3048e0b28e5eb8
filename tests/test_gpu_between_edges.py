"""GPU: cpi_state_between_batch at the edges of its contract -- a broken mfirst and broken state indices on the device, every double array
at an address that is 8 but not 16 bytes aligned, hess and chi2 in place each by itself, one NaN in every place it can sit, residuals of
exactly zero and rotations of exactly pi, weight 0, a fold of 300, 1027 factors in 257 workgroups, and Engine.chain_lm with fixes and
betweens together.  What must come back is stated once in tests/between_edge_checks.py, for the host twin
(tests/test_between_edges_cpu.py, where each check is also shown to fail on a twin with the defect it is there for) and for the device
alike.  The figures of a comparison are printed before anything is asserted; the gates are those of tests/between_cases.py; everything
else is bit equality or a property of the header."""
import numpy as np
import pytest
import torch

import cpi_amd
from tests import between_cases as bc
from tests import between_edge_checks as be
from tests import fix_cases as fx
from tests.test_gpu_between import ITER, LAM0, _t, dev_between, make_problem, run_lm
from tests.test_gpu_lm_edges import equal_runs, odd
from tests.test_lm_cpu import same_bits

pytestmark = pytest.mark.gpu
GATE = bc.GATE_EDGE_DEVICE


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def run_on(eng):
    return lambda c, **form: dev_between(eng, c, **form)


def _hold(m, gate, what):
    for k, v in m.items():
        assert v <= gate[k], (what, k, v)


# ------------------------------------------------------------------------------------------ 1. broken mfirst, broken indices
@pytest.mark.parametrize("kind", [0, 2], ids=["position", "pose"])
def test_broken_mfirst_and_indices_stay_inside(eng, kind):
    """include/cpi_amd.h: every mfirst range is "clamped into [0, M] where it is read", the state indices "into [0, S)".  Every broken
    value stays within pads that belong to the test, so a kernel without a clamp would read a NaN or write over a guard: a failure, not a
    fault.  The clamp is specified, so the bits are those of the call clamped in numpy (be.check_broken)."""
    c, x = bc.case(kind, 9), bc.case(kind, 9, "explicit")
    assert be.check_broken(run_on(eng), c, be.broken_mfirsts(c)) == 2
    assert be.check_broken(run_on(eng), x, be.broken_indices(x)) == 4
    for what, bad, f in be.broken_mfirsts(c) + be.broken_indices(x):         # the host form refuses each of them, naming the factor
        text = ("the measurements of factor %d leave \\[0, M\\] or mfirst decreases there" if "mfirst" in what else "state index out of range at factor %d") % f
        with pytest.raises(cpi_amd.CpiError, match="cpi_state_between_batch_host: " + text + "$"):
            dev_between(eng, bad, host=True)


# ------------------------------------------------------------------------------------------ 2. rows at 8-byte alignment
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_every_double_array_at_8_byte_alignment(eng, kind):
    """include/cpi_amd.h: "a double array needs the alignment of a double (8 bytes) and no more".  states, z, R, weight, hess_base,
    chi2_base, out, chi2 and chi2_m at data_ptr % 16 == 8 (dev_between asserts it of every output): the bits of the call on ordinary
    tensors.  This pins btw_d2u (packed, aligned 8), through which the kernel loads the base rows as 16-byte pieces, and st16_nt on the
    between rows."""
    c = bc.case(kind, 9, "explicit")
    for what, form in (("out of place", dict()), ("in place", dict(inplace=True)), ("cost only", dict(rows=False)), ("hess_base NULL", dict(bases=(False, True)))):
        want = dev_between(eng, c, **form)
        got = dev_between(eng, c, wrap=odd, **form)
        print("%s, %s at 8 mod 16: %s" % (bc.KINDS[kind], what, [a is None or same_bits(a, b) for a, b in zip(got, want)]))
        assert all((a is None and b is None) or same_bits(a, b) for a, b in zip(got, want)), what
        assert all(a is None or not np.isnan(a).any() for a in got), what


@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


def _weighted(pb, wrap=lambda t: t):
    """The betweens of a problem with a weight key (seeded, 0.5 .. 1.5), every float64 tensor through wrap."""
    rng = np.random.default_rng(71)
    return [dict(kind=b["kind"], z=wrap(b["z"]), R=wrap(b["R"]), mfirst=b["mfirst"], weight=wrap(_t(rng.uniform(0.5, 1.5, b["z"].shape[0]), b["z"].device)))
            for b in pb["on_dev"]]


def test_chain_lm_with_betweens_on_rows_at_8_byte_alignment(eng, pipe):
    """chain_lm(betweens=...) on the dense problem of tests/test_gpu_between.py, every float64 input, the buffers dict and the between
    dicts (z, R and a weight) at data_ptr % 16 == 8: the four returns of the run on ordinary tensors.  The in-place between kernel and the
    cost-only one run between factor_hessian / factor_cost and chain_solve / chain_accept on such rows."""
    pb = make_problem(eng, pipe, False)
    C, G, dev = pipe.C, pipe.G, eng.device
    S, F = C * G, pb["lin"].shape[0]
    want = run_lm(eng, pipe, dict(pb, on_dev=_weighted(pb)))
    torch.cuda.synchronize()
    want = tuple(t.clone() for t in want)
    z64 = lambda *shape: odd(torch.zeros(shape, dtype=torch.float64, device=dev))
    i32 = lambda: torch.zeros((C,), dtype=torch.int32, device=dev)
    b = dict(lam=odd(torch.full((C,), LAM0, dtype=torch.float64, device=dev)), cost=z64(C), phase=i32(), accepted=i32(), status=i32(), chi2=z64(F),
             chi2_new=z64(F), hess=z64(F, 496), delta=z64(S, 15), trial=z64(S, 16), workspace=z64(eng.chain_solve_workspace_doubles(S)),
             prior=z64(S, 136), pcost=z64(S), pcost_new=z64(S), idx_i=pb["ii"], idx_j=pb["jj"])
    got = eng.chain_lm(1, {n: odd(v) for n, v in pb["meas"].items()}, odd(pb["lin"]), None, odd(pipe.states), odd(pb["Rt"]), C, G, idx_i=pb["ii"],
                       idx_j=pb["jj"], prior0=odd(pb["prior0"]), anchor=odd(pb["anchor"]), prior_idx=pb["idx"], iterations=ITER, buffers=b,
                       betweens=_weighted(pb, odd))
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 8 for t in got[:3]) and b["hess"].data_ptr() % 16 == 8 and b["chi2"].data_ptr() % 16 == 8
    print("betweens on rows at 8-byte alignment: phase %s, states differ in %d entries, cost in %d" % (got[3].cpu().tolist(), (got[0] != want[0]).sum().item(),
                                                                                                      (got[1] != want[1]).sum().item()))
    assert equal_runs(got, want) and not torch.isnan(got[0]).any()


# ------------------------------------------------------------------------------------------ 3. mixed aliasing
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_mixed_aliasing(eng, kind):
    """The in-place rule is stated per array (hess == hess_base, chi2 == chi2_base); the kernel's flag looks at hess alone."""
    be.check_mixed_aliasing(run_on(eng), kind)
    be.check_mixed_aliasing(lambda c, **form: dev_between(eng, c, host=True, **form), kind)


# ------------------------------------------------------------------------------------------ 4. NaN stays where it is
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_nan_stays_where_it_is(eng, kind):
    assert be.check_nan_locality(run_on(eng), kind) == be.nan_calls(kind) >= 52


# ------------------------------------------------------------------------------------------ 5. exact residuals
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_exact_zero_residual(eng, kind):
    _hold(be.check_identity(run_on(eng), kind), GATE["identity"], "identity")


@pytest.mark.parametrize("kind", [1, 2], ids=bc.KINDS[1:])
def test_rotations_of_exactly_pi(eng, kind):
    _hold(be.check_pi(run_on(eng), kind), GATE["pi"], "pi")


@pytest.mark.parametrize("kind", [1, 2], ids=bc.KINDS[1:])
def test_scaled_quaternions(eng, kind):
    _hold(be.check_scaled(run_on(eng), kind), GATE["scaled"], "scaled")


# ------------------------------------------------------------------------------------------ 6. weight 0, long folds, position in the grid
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_weight_zero_removes_a_measurement_exactly(eng, kind):
    be.check_weight_zero(run_on(eng), kind)


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_long_fold(eng, kind):
    _hold(be.check_long(run_on(eng), kind), GATE["long"], "long")


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_many_factors(eng, kind):
    be.check_many(run_on(eng), kind)


# ------------------------------------------------------------------------------------------ 7. fixes and betweens together
def test_fixes_and_betweens_together_are_the_entries_issued_by_hand(eng, pipe):
    """chain_lm(fixes=..., betweens=...) on the ragged problem of tests/test_gpu_between.py, the betweens with a weight key, the fixes of
    tests/test_gpu_fix.py: two iterations against the entries issued by hand in the order of INTEGRATION.md 3q / 3r, bit for bit; then
    one iteration captured into a graph (a chain without parallel branches) and replayed twice: the eager run."""
    pb = make_problem(eng, pipe, True)
    C, G, dev, L = pipe.C, pipe.G, eng.device, pb["layout"]
    fixes = [dict(kind=f["kind"], z=_t(f["z"], dev), R=_t(f["R"], dev), mfirst=_t(f["mfirst"], dev)) for f in fx.e2e_fixes(pipe.pred.cpu().numpy(), L["member"])]
    betweens = _weighted(pb)
    chain = dict(C=C, G=G, **pb["chain"])
    call = lambda st, it, bufs, init=True, hist=None: eng.chain_lm(
        1, pb["meas"], pb["lin"], None, st, pb["Rt"], C, G, prior0=pb["prior0"], anchor=pb["anchor"], prior_idx=pb["idx"], lam=LAM0, iterations=it, buffers=bufs,
        init=init, fixes=fixes, betweens=betweens, cost_history=hist, **pb["chain"])
    bufs = {}
    hist = torch.zeros((3, C), dtype=torch.float64, device=dev)
    got = call(pipe.states.clone(), 2, bufs, hist=hist)
    torch.cuda.synchronize()
    got = tuple(t.clone() for t in got)
    assert len(bufs["fix_rows"]) == 2 and "prior" in bufs
    sweep = dict(idx_i=pb["ii"], idx_j=pb["jj"])

    def chi2_of(x):
        chi2 = eng.factor_cost(1, pb["meas"], pb["lin"], None, x, pb["Rt"], want_total=False, **sweep)["chi2"]
        for b in betweens:
            eng.state_between(x, b["kind"], b["z"], b["R"], b["mfirst"], pb["ii"], pb["jj"], weight=b["weight"], chi2_base=chi2, chi2=chi2, want_rows=False)
        return chi2

    def pcost_of(x):
        pc = eng.prior_relinearize(x, pb["anchor"], pb["prior0"], idx=pb["idx"], want_prior=False)[1]
        for f in fixes:
            pc = eng.state_fix(x, f["kind"], f["z"], f["R"], f["mfirst"], pcost_base=pc, want_rows=False)[1]
        return pc

    st = pipe.states.clone()
    lam = torch.full((C,), LAM0, dtype=torch.float64, device=dev)
    phase = torch.zeros((C,), dtype=torch.int32, device=dev)
    chi2 = chi2_of(st)
    cost = eng.chain_cost(chi2, pcost_of(st), **chain)
    costs, accepted = [cost.clone()], []
    for _ in range(2):
        rows = eng.prior_relinearize(st, pb["anchor"], pb["prior0"], idx=pb["idx"], want_cost=False)[0]
        for f in fixes:
            rows = eng.state_fix(st, f["kind"], f["z"], f["R"], f["mfirst"], base=rows, want_cost=False)[0]
        hess = eng.factor_hessian(1, pb["meas"], pb["lin"], None, st, pb["Rt"], **sweep)
        for b in betweens:
            eng.state_between(st, b["kind"], b["z"], b["R"], b["mfirst"], pb["ii"], pb["jj"], weight=b["weight"], hess_base=hess, out=hess, want_cost=False)
        delta = eng.chain_solve(hess, prior=rows, lam=lam, damping="diagonal", **chain)
        trial = eng.retract(st, delta)
        chi2_new = chi2_of(trial)
        acc = torch.zeros((C,), dtype=torch.int32, device=dev)
        eng.chain_accept(chi2_new, pcost_of(trial), trial, cost, st, lam, phase, chi2=chi2, accepted=acc, **chain)
        costs.append(cost.clone())
        accepted.append(acc)
    torch.cuda.synchronize()
    print("fixes and betweens together: cost per iteration (rows) and chain (columns):\n%s\naccepted %s, lambda %s, phase %s"
          % (np.array2string(torch.stack(costs).cpu().numpy(), precision=5, max_line_width=200), [a.cpu().tolist() for a in accepted],
             lam.cpu().tolist(), phase.cpu().tolist()))
    assert equal_runs(got, (st, cost, lam, phase)) and torch.equal(hist, torch.stack(costs))
    assert accepted[0].cpu().tolist() == [1] * C and (costs[1] < costs[0]).all()
    member = torch.from_numpy(L["member"]).to(dev)
    assert torch.equal(got[0][~member], pipe.states[~member])                 # a state of no chain is never moved
    # one iteration as a graph, replayed twice
    gb, gst = {}, pipe.states.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(gst, 1, gb)                                                      # warm-up on a side stream; fills gb
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(gst, 1, gb, init=False)
    gst.copy_(pipe.states)                                                    # back to the start: states, lambda, phase, then cost and chi2 (init)
    gb["lam"].fill_(LAM0)
    gb["phase"].zero_()
    call(gst, 0, gb)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert equal_runs((gst, gb["cost"], gb["lam"], gb["phase"]), got)
