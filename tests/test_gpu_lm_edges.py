"""GPU: the Levenberg-Marquardt step per chain at the edges of its contract -- cpi_prior_relinearize_batch at GPS-sized positions with
float32-rounded and scaled quaternions, the equalities and infinities of cpi_chain_accept_batch's rule and chains on both sides of its
copy loop's trip, every double array of the whole loop at an address that is 8 but not 16 bytes aligned, Engine.chain_lm with fixes and
no prior against the entries issued by hand, and weight 0 as the exact removal of an outlier.  The figures of a comparison are printed
before anything is asserted; the gates are those of tests/lm_cases.py; everything else is bit equality or a property of the header.

The alignment tests pin the types through which the chain family moves 16-byte pieces of 8-byte aligned rows: fix_d2u
(cpi_fix_kernels.hpp), lm_d2u (cpi_lm_kernels.hpp), chain_d2u, trial_d2u, cpi_d2v and st16_nt.  All rows of the family have an even
number of doubles, so a row inherits the alignment of its allocation, and an allocation of torch is aligned to far more than 16."""
import os

import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import fix_cases as fx
from tests import lm_cases as lc
from tests import test_lm_cpu as tl
from tests.test_gpu_fix import ITER, LAM0, _t, run_lm
from tests.test_gpu_lm import dev_accept, dev_cost, dev_prior, twin_from_xi
from tests.test_lm_cpu import check_accept, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


@pytest.fixture(scope="module")
def hl():
    if (not os.path.exists(tl._LIB)) or os.path.getmtime(tl._LIB) < max(os.path.getmtime(p) for p in (tl._SRC, tl._MATH)):
        tl.tm._build(tl._SRC, tl._LIB)
    return tl._bind(tl._LIB)


# ------------------------------------------------------------------------------------------ 1. the hard prior case
def test_prior_on_the_hard_case(eng, hl):
    """S = 65: sixteen workgroups of four records and a last one that holds a single record."""
    S = 65
    states, anchor, prior0 = lc.hard_prior_case(S)
    xi = eng.local_coordinates(_t(states, eng.device), _t(anchor, eng.device)).cpu().numpy()
    prior, pcost = dev_prior(eng, S, None, states, anchor, prior0)
    rows, pc = lc.prior_documented(xi, prior0)
    assert same_bits(prior, rows) and same_bits(pcost, pc)                    # the documented orders, bit for bit
    tr, tp = twin_from_xi(hl, xi, prior0)
    assert same_bits(prior, tr) and same_bits(pcost, tp)                      # ... and the twin's arithmetic from the device's own xi
    assert same_bits(prior[:, :120], prior0[:, :120]) and (prior[:, 135] == 0.0).all()       # Lam is copied
    hp, hc = dev_prior(eng, S, None, states, anchor, prior0, host=True)
    assert same_bits(hp, prior) and same_bits(hc, pcost)
    at = np.arange(S) % 4 == 0
    m_eta, m_pc = lc.prior_metrics(prior, pcost, lc.oracle_local(states, anchor), prior0, skip=at)
    print("the hard prior case, S %d: eta %.3g units (gate %.0f), pcost %.3g units (gate %.0f); at the anchor the device's |xi| max %.3g"
          % (S, m_eta, lc.GATE_ETA_DEVICE, m_pc, lc.GATE_PCOST_DEVICE, np.abs(xi[at]).max()))
    assert m_eta <= lc.GATE_ETA_DEVICE and m_pc <= lc.GATE_PCOST_DEVICE


# ------------------------------------------------------------------------------------------ 2. the rule's equalities and infinities
def test_edge_rule_table(eng):
    case, want = lc.edge_rule_table()
    got = dev_accept(eng, case)
    for c, (rule, (acc, phase, lam)) in enumerate(zip(lc.RULES_EDGE, want)):
        print("%-28s accepted %d phase %d lambda %g cost %g" % (rule[0], got[5][c], got[4][c], got[3][c], got[0][c]))
        assert (got[5][c], got[4][c], got[3][c]) == (acc, phase, lam), rule[0]
    check_accept(got, case.expected())                                        # accepted rows = the trial's, every sentinel elsewhere intact
    b = case.call.b
    for c in (6, 7, 8):                                                       # 16, 17 and 32 states: both sides of the trip of 128 pieces
        rows = b.rows(c)
        assert same_bits(got[1][rows], case.trial[rows])
        assert same_bits(got[1][rows.start - 2:rows.start], case.states[rows.start - 2:rows.start])
        assert same_bits(got[1][rows.stop:rows.stop + 2], case.states[rows.stop:rows.stop + 2])
    new = dev_cost(eng, case.call, case.chi2_new, case.pcost_new)
    assert same_bits(got[0][got[5] == 1], new[got[5] == 1])
    check_accept(dev_accept(eng, case, host=True), got)                       # the host form: the device form's bits


# ------------------------------------------------------------------------------------------ the dense end-to-end problem
@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


@pytest.fixture(scope="module")
def pb(eng, pipe):
    """The dense problem of tests/test_gpu_fix.py: eight chains of six, a Gaussian prior on every chain's first state, a position fix on
    every state and pose fixes on the first and the fourth of every chain."""
    C, G, dev = pipe.C, pipe.G, eng.device
    L = fx.layout(False)
    P0 = np.zeros((C, 16, 16))
    P0[:, np.arange(15), np.arange(15)] = 0.1 * cc.SCALES ** 2
    first = _t(L["first"], dev)
    fixes = fx.e2e_fixes(pipe.pred.cpu().numpy(), L["member"])
    on_dev = [dict(kind=f["kind"], z=_t(f["z"], dev), R=_t(f["R"], dev), mfirst=_t(f["mfirst"], dev)) for f in fixes]
    return dict(layout=L, ragged=False, anchor=pipe.pred[first].contiguous(), prior0=_t(cc.pack_upper(P0), dev), idx=first.to(torch.int32), fixes=fixes,
                on_dev=on_dev, chain={}, ii=pipe.ii, jj=pipe.jj, lin=pipe.lin, Rt=pipe.Rt, meas={n: v for n, v in pipe.meas.items() if not n.startswith("_")})


@pytest.fixture(scope="module")
def eager(eng, pipe, pb):
    out = run_lm(eng, pipe, pb)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def equal_runs(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ 3. rows at 8-byte alignment
def odd(t):
    """The float64 tensor copied to an address that is 8 but not 16 bytes aligned."""
    assert t.dtype == torch.float64
    flat = torch.empty((t.numel() + 1,), dtype=torch.float64, device=t.device)
    out = flat[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous()
    return out


def test_the_whole_loop_on_rows_at_8_byte_alignment(eng, pipe, pb, eager):
    """Every float64 array of chain_lm -- inputs and the buffers dict, whose keys are interface -- at data_ptr % 16 == 8: the bits of the
    run on ordinary tensors.  The run covers factor_cost, prior_relinearize, state_fix, factor_hessian, chain_solve, retract and
    chain_accept."""
    C, G, dev = pipe.C, pipe.G, eng.device
    S, F = C * G, pb["lin"].shape[0]
    z64 = lambda *shape: odd(torch.zeros(shape, dtype=torch.float64, device=dev))
    i32 = lambda: torch.zeros((C,), dtype=torch.int32, device=dev)
    b = dict(lam=odd(torch.full((C,), LAM0, dtype=torch.float64, device=dev)), cost=z64(C), phase=i32(), accepted=i32(), status=i32(), chi2=z64(F),
             chi2_new=z64(F), hess=z64(F, 496), delta=z64(S, 15), trial=z64(S, 16), workspace=z64(eng.chain_solve_workspace_doubles(S)),
             prior=z64(S, 136), pcost=z64(S), pcost_new=z64(S), idx_i=pb["ii"], idx_j=pb["jj"], fix_rows=[z64(S, 136), z64(S, 136)],
             fix_pcost=[z64(S), z64(S)])
    fixes = [dict(kind=f["kind"], z=odd(f["z"]), R=odd(f["R"]), mfirst=f["mfirst"]) for f in pb["on_dev"]]
    got = eng.chain_lm(1, {n: odd(v) for n, v in pb["meas"].items()}, odd(pb["lin"]), None, odd(pipe.states), odd(pb["Rt"]), C, G, idx_i=pb["ii"],
                       idx_j=pb["jj"], prior0=odd(pb["prior0"]), anchor=odd(pb["anchor"]), prior_idx=pb["idx"], iterations=ITER, buffers=b, fixes=fixes)
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 8 for t in got[:3]) and got[1].data_ptr() == b["cost"].data_ptr()
    print("rows at 8-byte alignment: phase %s, states differ in %d entries, cost in %d" % (got[3].cpu().tolist(), (got[0] != eager[0]).sum().item(),
                                                                                          (got[1] != eager[1]).sum().item()))
    assert equal_runs(got, eager)


def test_marginals_and_marginalize_on_rows_at_8_byte_alignment(eng, pipe, pb, eager):
    C, G, dev = pipe.C, pipe.G, eng.device
    S = C * G
    st = eager[0]
    rows, _ = eng.prior_relinearize(st, pb["anchor"], pb["prior0"], idx=pb["idx"])
    hess = eng.factor_hessian(1, pb["meas"], pb["lin"], None, st, pb["Rt"], pb["ii"], pb["jj"])
    ws = torch.zeros((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    status = torch.zeros((C,), dtype=torch.int32, device=dev)
    eng.chain_solve(hess, C=C, G=G, prior=rows, status=status, workspace=ws)
    cov = eng.chain_marginals(ws, C=C, G=G, status=status)
    cov8 = eng.chain_marginals(odd(ws), C=C, G=G, status=status, out=odd(torch.full((S, 120), float("nan"), dtype=torch.float64, device=dev)))
    marg = eng.chain_marginalize(hess, C=C, G=G, prior=rows, drop=2)
    marg8 = eng.chain_marginalize(odd(hess), C=C, G=G, prior=odd(rows), drop=2, out=odd(torch.full((C, 136), float("nan"), dtype=torch.float64, device=dev)))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * C and not torch.isnan(cov).any() and not torch.isnan(marg[:, :135]).any()
    assert cov8.data_ptr() % 16 == 8 and marg8.data_ptr() % 16 == 8
    assert torch.equal(cov8, cov) and torch.equal(marg8, marg)


# ------------------------------------------------------------------------------------------ 4. fixes without a prior
def test_fixes_without_a_prior_are_the_entries_issued_by_hand(eng, pipe, pb):
    """chain_lm(prior0=None, fixes=...): _lm_fixes starts from a None base and the buffers dict has no "prior" / "pcost" / "pcost_new".
    Two iterations against the entries in the order of INTEGRATION.md 3q, bit for bit.  The sanity check is loose on purpose: a
    longdouble CPU loop of this case (fx.FixLoop with a zero prior0) takes the costs from 3e4 .. 7e4 to 8 .. 23 in the first iteration,
    a ratio of at most 4e-4 against the 1e-2 asserted.  The final states are not compared with that loop: without the prior the
    undamped systems have condition numbers of 2.5e11, above cc.COND_MAX."""
    C, G, dev = pipe.C, pipe.G, eng.device
    bufs = {}
    hist = torch.zeros((3, C), dtype=torch.float64, device=dev)
    got = eng.chain_lm(1, pb["meas"], pb["lin"], None, pipe.states.clone(), pb["Rt"], C, G, idx_i=pb["ii"], idx_j=pb["jj"], prior0=None, anchor=None,
                       prior_idx=None, lam=LAM0, iterations=2, buffers=bufs, fixes=pb["on_dev"], cost_history=hist)
    assert not {"prior", "pcost", "pcost_new"} & set(bufs) and len(bufs["fix_rows"]) == 2 and len(bufs["fix_pcost"]) == 2
    sweep = dict(idx_i=pb["ii"], idx_j=pb["jj"])

    def fix_cost(x):
        pc = None
        for f in pb["on_dev"]:
            pc = eng.state_fix(x, f["kind"], f["z"], f["R"], f["mfirst"], pcost_base=pc, want_rows=False)[1]
        return pc

    st = pipe.states.clone()
    lam = torch.full((C,), LAM0, dtype=torch.float64, device=dev)
    phase = torch.zeros((C,), dtype=torch.int32, device=dev)
    chi2 = eng.factor_cost(1, pb["meas"], pb["lin"], None, st, pb["Rt"], want_total=False, **sweep)["chi2"]
    cost = eng.chain_cost(chi2, fix_cost(st), C=C, G=G)
    costs, accepted = [cost.clone()], []
    for _ in range(2):
        rows = None
        for f in pb["on_dev"]:
            rows = eng.state_fix(st, f["kind"], f["z"], f["R"], f["mfirst"], base=rows, want_cost=False)[0]
        hess = eng.factor_hessian(1, pb["meas"], pb["lin"], None, st, pb["Rt"], **sweep)
        delta = eng.chain_solve(hess, C=C, G=G, prior=rows, lam=lam, damping="diagonal")
        trial = eng.retract(st, delta)
        chi2_new = eng.factor_cost(1, pb["meas"], pb["lin"], None, trial, pb["Rt"], want_total=False, **sweep)["chi2"]
        acc = torch.zeros((C,), dtype=torch.int32, device=dev)
        eng.chain_accept(chi2_new, fix_cost(trial), trial, cost, st, lam, phase, C=C, G=G, chi2=chi2, accepted=acc)
        costs.append(cost.clone())
        accepted.append(acc)
    torch.cuda.synchronize()
    print("fixes without a prior: cost per iteration (rows) and chain (columns):\n%s\naccepted %s, lambda %s, phase %s"
          % (np.array2string(torch.stack(costs).cpu().numpy(), precision=5, max_line_width=200), [a.cpu().tolist() for a in accepted],
             lam.cpu().tolist(), phase.cpu().tolist()))
    assert equal_runs(got, (st, cost, lam, phase)) and torch.equal(hist, torch.stack(costs))
    assert accepted[0].cpu().tolist() == [1] * C and (costs[1] < 1e-2 * costs[0]).all()


# ------------------------------------------------------------------------------------------ 5. weight 0 removes an outlier exactly
def test_weight_zero_removes_an_outlier_exactly(eng, pipe, pb, eager):
    """One gross outlier per chain among the position fixes (100 m off, on the chain's third state, in CSR order behind the real fix):
    with weight 0 on the outliers the run has the bits of the run without them -- fma(0, G, Lam) and fma(0, chi2, pcost) are exact --,
    with weight 1 it ends more than one standard deviation elsewhere."""
    C, G, dev = pipe.C, pipe.G, eng.device
    S = C * G
    pos = pb["fixes"][0]
    assert np.array_equal(pos["mfirst"], np.arange(S + 1))
    hit = np.arange(C) * G + 2
    counts = np.ones(S, dtype=np.int64)
    counts[hit] = 2
    own = np.repeat(np.arange(S), counts)
    second = np.concatenate([[False], own[1:] == own[:-1]])                   # the outliers: the second fix of their state
    z = pos["z"][own].copy()
    z[second] += np.array([100.0, 0.0, 0.0])
    with_out = lambda w: [dict(kind="position", z=_t(z, dev), R=_t(pos["R"][own], dev), mfirst=_t(fx.offsets(counts), dev), weight=_t(w, dev)), pb["on_dev"][1]]
    assert second.sum() == C and torch.equal(eng.fix_offsets(_t(own, dev), S), _t(fx.offsets(counts), dev))
    gated = run_lm(eng, pipe, dict(pb, on_dev=with_out(np.where(second, 0.0, 1.0))))
    torch.cuda.synchronize()
    gated = tuple(t.clone() for t in gated)
    print("weight 0 on the outliers: states differ from the run without them in %d entries, cost in %d" % ((gated[0] != eager[0]).sum().item(),
                                                                                                         (gated[1] != eager[1]).sum().item()))
    assert equal_runs(gated, eager)
    # sigma at the final states of the run without outliers, formed as tests/test_gpu_fix.py forms it
    st = eager[0]
    rows, _ = eng.prior_relinearize(st, pb["anchor"], pb["prior0"], idx=pb["idx"])
    for f in pb["on_dev"]:
        rows, _ = eng.state_fix(st, f["kind"], f["z"], f["R"], f["mfirst"], base=rows, want_cost=False)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    status = torch.zeros((C,), dtype=torch.int32, device=dev)
    eng.chain_solve(eng.factor_hessian(1, pb["meas"], pb["lin"], None, st, pb["Rt"], pb["ii"], pb["jj"]), C=C, G=G, prior=rows, status=status, workspace=ws)
    cov = eng.chain_marginals(ws, C=C, G=G, status=status)
    kept = run_lm(eng, pipe, dict(pb, on_dev=with_out(np.ones(len(own)))))
    torch.cuda.synchronize()
    sigma = np.sqrt(cov.cpu().numpy()[:, [cc.tri(i) + i for i in range(15)]])
    away = np.abs(lc.oracle_local(kept[0].cpu().numpy(), st.cpu().numpy()) / sigma)
    print("weight 1 on the outliers: %.3g sigma away (per chain %s), phase %s" % (away.max(), np.array2string(away.reshape(C, -1).max(1), precision=3),
                                                                                 kept[3].cpu().tolist()))
    assert status.cpu().tolist() == [0] * C and (away.reshape(C, -1).max(1) > 1.0).all()
