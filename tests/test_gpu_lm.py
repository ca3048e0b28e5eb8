"""GPU: cpi_prior_relinearize_batch, cpi_chain_cost_batch and cpi_chain_accept_batch against the restatements and references of
tests/lm_cases.py at the smallest shapes where the kernels can go wrong, the host forms and the C++ facade against the device forms bit
for bit, and Engine.chain_lm end to end on the chains of tests/chain_pipeline.py: eager, with a chain that must give up, and as one
captured graph.  The figures of a comparison are printed before anything is asserted; the gates are those of tests/lm_cases.py.

What "bit for bit with the host twin" means for the prior: the twin's arithmetic on the xi the DEVICE forms (cpi_local_batch).  The
quaternion part of localCoordinates is not the same bits on the host and on the device (a reciprocal square root there, a square root and
a division here: tests/test_gpu_trial.py holds it to a tolerance for the same reason); everything after xi is."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import lm_cases as lc
from tests import test_lm_cpu as tl
from tests.test_lm_cpu import check_accept, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = lc.SENTINEL


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


@pytest.fixture(scope="module")
def hl():
    if (not os.path.exists(tl._LIB)) or os.path.getmtime(tl._LIB) < max(os.path.getmtime(p) for p in (tl._SRC, tl._MATH)):
        tl.tm._build(tl._SRC, tl._LIB)
    return tl._bind(tl._LIB)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kw(call, dev):
    return dict(C=call.C, G=call.G, first=_t(call.first, dev), count=_t(call.count, dev), ffirst=_t(call.ffirst, dev))


# ------------------------------------------------------------------------------------------ prior_relinearize
def dev_prior(eng, S, idx, states, anchor, prior0, want_prior=True, want_cost=True, host=False):
    """prior_relinearize -> (prior [S, 136], pcost [S]) as numpy, sentinels wherever nothing is written; the row past S keeps its own."""
    dev = "cpu" if host else eng.device
    prior = torch.full((S + 1, 136), SENTINEL, dtype=torch.float64, device=dev) if want_prior else None
    pcost = torch.full((S + 1,), SENTINEL, dtype=torch.float64, device=dev) if want_cost else None
    fn = eng.prior_relinearize_host if host else eng.prior_relinearize
    out = fn(_t(states, dev), _t(anchor, dev), _t(prior0, dev), idx=_t(None if idx is None else np.asarray(idx, dtype=np.int32), dev),
             out=None if prior is None else prior[:S], pcost=None if pcost is None else pcost[:S], want_prior=want_prior, want_cost=want_cost)
    if not host:
        torch.cuda.synchronize()
    assert (out[0] is None) == (not want_prior) and (out[1] is None) == (not want_cost)
    assert (prior is None or (prior[S] == SENTINEL).all()) and (pcost is None or pcost[S] == SENTINEL)
    return (None if prior is None else prior[:S].cpu().numpy()), (None if pcost is None else pcost[:S].cpu().numpy())


def twin_from_xi(hl, xi, prior0):
    rows, pc = np.zeros((len(xi), 136)), np.zeros(len(xi))
    assert hl.hsl_prior_from_xi(len(xi), tl._ptr(np.ascontiguousarray(xi)), tl._ptr(np.ascontiguousarray(prior0)), tl._ptr(rows), tl._ptr(pc)) == 0
    return rows, pc


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_prior_against_the_twin_the_host_form_and_the_reference(eng, hl, S):
    states, anchor, prior0 = lc.prior_case(S)
    xi = eng.local_coordinates(_t(states, eng.device), _t(anchor, eng.device)).cpu().numpy()      # cpi_local_batch: the xi the entry promises
    at = np.arange(S) % 4 == 0
    print("S %d: records at their anchor: the device's |xi| max %.3g" % (S, np.abs(xi[at]).max()))
    for P in sorted({S, S - 1}):
        prior, pcost = dev_prior(eng, S, None, states, anchor[:P], prior0[:P])
        rows, pc = lc.prior_documented(xi[:P], prior0[:P])
        assert same_bits(prior[:P], rows) and same_bits(pcost[:P], pc), P                    # the documented orders, bit for bit
        tr, tp = twin_from_xi(hl, xi[:P], prior0[:P])
        assert same_bits(prior[:P], tr) and same_bits(pcost[:P], tp), P                      # ... and the twin's arithmetic
        assert same_bits(prior[:P, :120], prior0[:P, :120]) and (prior[:P, 135] == 0.0).all()   # Lam and entry 135 are exact
        assert (prior[P:] == SENTINEL).all() and (pcost[P:] == SENTINEL).all()               # the state without a record
        still = at[:P] & (xi[:P] == 0.0).all(1)                                              # xi = 0: prior0 with entry 135 zeroed, pcost 0
        print("S %d P %d: %d of the %d records at their anchor have xi == 0 on the device (the others: the bit comparison above; "
              "test_prior_at_the_anchor_passes_prior0_through holds the property where xi is exactly zero)" % (S, P, still.sum(), at[:P].sum()))
        assert same_bits(prior[:P][still, :135], prior0[:P][still, :135]) and (pcost[:P][still] == 0.0).all()
        hp, hc = dev_prior(eng, S, None, states, anchor[:P], prior0[:P], host=True)
        assert same_bits(hp, prior) and same_bits(hc, pcost), P                              # the host form: the device form's bits
        if P:
            m_eta, m_pc = lc.prior_metrics(prior[:P], pcost[:P], lc.oracle_local(states[:P], anchor[:P]), prior0[:P], skip=at[:P])
            print("S %d P %d: eta %.3g units (gate %.0f), pcost %.3g units (gate %.0f)" % (S, P, m_eta, lc.GATE_ETA_DEVICE, m_pc, lc.GATE_PCOST_DEVICE))
            assert m_eta <= lc.GATE_ETA_DEVICE and m_pc <= lc.GATE_PCOST_DEVICE


def test_prior_at_the_anchor_passes_prior0_through(eng):
    """states[s] == anchor[p] with xi exactly zero on the device too: quaternions with one non-zero entry (the identity and the half turns
    about the axes), whose product with their inverse has no rounding.  The row is prior0 with entry 135 zeroed and pcost is +0.0 or -0.0."""
    S = 67
    states, _, prior0 = (x.copy() for x in lc.prior_case(130))
    states, prior0 = states[:S], prior0[:S]
    states[:, :4] = np.eye(4)[(np.arange(S) + 3) % 4]
    xi = eng.local_coordinates(_t(states, eng.device), _t(states, eng.device)).cpu().numpy()
    assert (xi == 0.0).all()                                                  # the premise, on the device: not vacuous
    prior, pcost = dev_prior(eng, S, None, states, states.copy(), prior0)
    assert same_bits(prior[:, :135], prior0[:, :135]) and (prior[:, 135] == 0.0).all() and (pcost == 0.0).all()
    assert (np.abs(prior0[1::2, 120:135]).max(1) > 0).all()                   # eta0 non-zero in every other record: it passes through as it is


def test_prior_idx_outputs_and_nan(eng):
    S = 70
    states, anchor, prior0 = (x.copy() for x in lc.prior_case(130))
    states, anchor, prior0 = states[:S], anchor[:S], prior0[:S]
    full, full_pc = dev_prior(eng, S, None, states, anchor, prior0)
    sub = np.arange(S - 1, -1, -1)[::2].astype(np.int32)                      # reverse order, every other state has no record
    idx = np.concatenate([[-1], sub[:20], [S], sub[20:], [-5, S + 3]]).astype(np.int32)      # skipped at the ends and inside a wavefront
    P = len(idx)
    live = (idx >= 0) & (idx < S)
    an, p0 = np.full((P, 16), np.nan), np.full((P, 136), np.nan)              # a skipped record is not read: NaN would show
    an[live], p0[live] = anchor[idx[live]], prior0[idx[live]]
    prior, pcost = dev_prior(eng, S, idx, states, an, p0)
    assert same_bits(prior[sub], full[sub]) and same_bits(pcost[sub], full_pc[sub])          # a record's bits: its own data only
    rest = np.setdiff1d(np.arange(S), sub)
    assert (prior[rest] == SENTINEL).all() and (pcost[rest] == SENTINEL).all()
    only_p, none = dev_prior(eng, S, idx, states, an, p0, want_cost=False)
    none2, only_c = dev_prior(eng, S, idx, states, an, p0, want_prior=False)
    assert none is None and none2 is None and same_bits(only_p, prior) and same_bits(only_c, pcost)
    hp, hc = dev_prior(eng, S, idx, states, an, p0, host=True)
    assert same_bits(hp, prior) and same_bits(hc, pcost)
    states[5, 7] = np.nan                                                     # NaN in one record reaches that record's outputs only
    prior0[9, 3] = np.nan
    bad, bad_pc = dev_prior(eng, S, None, states, anchor, prior0)
    others = ~np.isin(np.arange(S), (5, 9))
    assert same_bits(bad[others], full[others]) and same_bits(bad_pc[others], full_pc[others])
    assert np.isnan(bad_pc[5]) and np.isnan(bad[5, 120:135]).any() and same_bits(bad[5, :120], prior0[5, :120])
    assert np.isnan(bad_pc[9]) and np.isnan(bad[9, 120:135]).any()


# ------------------------------------------------------------------------------------------ chain_cost
def dev_cost(eng, call, chi2, pcost, host=False):
    dev = "cpu" if host else eng.device
    buf = torch.full((call.C + 1,), SENTINEL, dtype=torch.float64, device=dev)
    fn = eng.chain_cost_host if host else eng.chain_cost
    out = fn(_t(chi2, dev), _t(pcost, dev), S=call.S, out=buf[:call.C], **_kw(call, dev))
    if not host:
        torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and buf[call.C] == SENTINEL
    return buf[:call.C].cpu().numpy()


def test_cost_on_every_layout(eng, hl):
    worst = 0.0
    for name, counts, layout in lc.COST_LAYOUTS:
        b = cc.Batch(counts, seed=3, layout=layout)
        call = lc.cost_call(b)
        for negative in (False, True):
            chi2, pcost = lc.cost_terms(b, negative=negative)
            for pc in (pcost, None):
                got = dev_cost(eng, call, chi2 if b.G > 1 else None, pc)
                assert same_bits(got, lc.chain_costs(call, chi2, pc)), name                  # the documented shape, bit for bit
                assert same_bits(got, tl.twin_cost(hl, call, chi2 if b.G > 1 else None, pc)), name
                worst = max(worst, lc.cost_metric(got, call, chi2, pc))
            if negative:
                assert (got[b.count > 0] >= 0).all() and (dev_cost(eng, call, chi2 if b.G > 1 else None, pcost)[b.count > 0] < 0).all(), name
        zero = dev_cost(eng, call, chi2 if b.G > 1 else None, pcost)[b.count == 0]
        assert (zero == 0.0).all() and not np.signbit(zero).any()             # a chain without states: +0.0
        if name in ("ragged", "gaps", "dense 5x17"):
            assert same_bits(dev_cost(eng, call, chi2, pcost, host=True), dev_cost(eng, call, chi2, pcost)), name
    print("device, every layout: cost %.3g units (gate %.0f)" % (worst, lc.GATE_COST_DEVICE))
    assert worst <= lc.GATE_COST_DEVICE


def test_cost_nan_refused_chain_and_position(eng):
    b = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
    call = cc.Call.explicit(b)
    chi2, pcost = lc.cost_terms(b)
    good = dev_cost(eng, call, chi2, pcost)
    bad2 = chi2.copy()
    bad2[b.ffirst[5] + 16] = np.nan                                           # chain 5 (40 states), slot 0, second trip
    got = dev_cost(eng, call, bad2, pcost)
    assert np.isnan(got[5]) and same_bits(np.delete(got, 5), np.delete(good, 5))
    out = cc.clone(b)
    out.ffirst[5] = b.F - 3                                                   # 39 rows from F - 3 on: refused, nothing is read
    got = dev_cost(eng, cc.Call.explicit(out), chi2, pcost)
    assert np.isnan(got[5]) and same_bits(np.delete(got, 5), np.delete(good, 5))
    out.ffirst[5] = -1
    assert np.isnan(dev_cost(eng, cc.Call.explicit(out), chi2, pcost)[5])
    order = np.array([7, 3, 10, 4, 0, 5])                                     # other positions, another C: the same bits
    assert same_bits(dev_cost(eng, cc.Call.explicit(b, chains=order), chi2, pcost), good[order])


# ------------------------------------------------------------------------------------------ chain_accept
def dev_accept(eng, case, with_chi2=True, with_accepted=True, host=False):
    """chain_accept on copies of the case's arrays -> (cost, states, chi2, lam, phase, accepted) as accept_expected gives them."""
    dev = "cpu" if host else eng.device
    call = case.call
    cost, states, lam, phase = (_t(x.copy(), dev) for x in (case.cost, case.states, case.lam, case.phase))
    chi2 = _t(case.chi2.copy(), dev) if with_chi2 else None
    acc = torch.full((call.C,), 99, dtype=torch.int32, device=dev) if with_accepted else None
    fn = eng.chain_accept_host if host else eng.chain_accept
    fn(_t(case.chi2_new, dev), _t(case.pcost_new, dev), _t(case.trial, dev), cost, states, lam, phase, chi2=chi2, accepted=acc, params=case.params,
       **_kw(call, dev))
    if not host:
        torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (cost, states, chi2, lam, phase, acc))


def test_rule_table(eng):
    case, want = lc.rule_table()
    got = dev_accept(eng, case)
    for c, (rule, (acc, phase, lam)) in enumerate(zip(lc.RULES, want)):
        print("%-26s accepted %d phase %d lambda %g" % (rule[0], got[5][c], got[4][c], got[3][c]))
        assert (got[5][c], got[4][c], got[3][c]) == (acc, phase, lam), rule[0]
    check_accept(got, case.expected())                                        # accepted rows = the trial's, every sentinel elsewhere intact
    new = dev_cost(eng, case.call, case.chi2_new, case.pcost_new)
    assert same_bits(got[0][got[5] == 1], new[got[5] == 1])                   # new is cpi_chain_cost_batch's value, read back through cost
    check_accept(dev_accept(eng, case, with_chi2=False, with_accepted=False), case.expected(with_chi2=False))
    inside, _ = lc.rule_table(outside=False)                                  # the host form refuses rows outside; on the rest: the device form's bits
    check_accept(dev_accept(eng, inside, host=True), dev_accept(eng, inside))
    with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain 14 leave"):
        dev_accept(eng, case, host=True)


@pytest.mark.parametrize("layout", ["tile", "gaps", "reverse"])
def test_accept_ragged(eng, layout):
    case = lc.ragged_accept_case(layout)
    got = dev_accept(eng, case)
    check_accept(got, case.expected())
    n = case.call.b.count
    assert got[5].tolist() == [int(c % 2 == 0 and c != 5 and n[c] > 0) for c in range(case.call.C)]
    new = dev_cost(eng, case.call, case.chi2_new, case.pcost_new)
    assert same_bits(got[0][got[5] == 1], new[got[5] == 1])
    check_accept(dev_accept(eng, case, host=True), got)


def test_lm_cpp_facade(eng):
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_lm")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_lm.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "test_lm ok 5 4", p.stdout
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[-6:-1]])
    Cn, G = 5, 4                                                              # the chains of the program, through the module-level entries
    dev = eng.device
    states = np.zeros((Cn * G, 16))
    states[:, 3] = 1.0
    states[:, 4:] = np.arange(Cn * G)[:, None] + np.arange(4, 16)[None, :]
    anchor = states[0::G].copy()
    anchor[:, 4:] += 0.25 * (np.arange(Cn)[:, None] + 1)
    P0 = np.zeros((Cn, 16, 16))
    P0[:, np.arange(15), np.arange(15)] = np.arange(1, 16)
    k = np.arange(G - 1)[None, :] + 1 + np.arange(Cn)[:, None]
    chi2 = (2.0 * k).reshape(-1)
    chi2_new = (2.0 * k + np.where(np.arange(Cn) % 2, 4.0, -2.0)[:, None]).reshape(-1)
    prior, pcost = cpi_amd.prior_relinearize(_t(states, dev), _t(anchor, dev), _t(cc.pack_upper(P0), dev), idx=_t((np.arange(Cn) * G).astype(np.int32), dev))
    cost = cpi_amd.chain_cost(_t(chi2, dev), pcost, C=Cn, G=G)
    cost_new = cpi_amd.chain_cost(_t(chi2_new, dev), pcost, C=Cn, G=G)
    lam, phase = torch.ones(Cn, dtype=torch.float64, device=dev), torch.zeros(Cn, dtype=torch.int32, device=dev)
    st, after = _t(states, dev), cost.clone()
    cpi_amd.chain_accept(_t(chi2_new, dev), pcost, _t(states + 0.5, dev), after, st, lam, phase, C=Cn, G=G)
    torch.cuda.synchronize()
    mine = np.concatenate([prior.cpu().numpy()[0::G, 120:135], pcost.cpu().numpy()[0::G, None], cost.cpu().numpy()[:, None], cost_new.cpu().numpy()[:, None],
                           after.cpu().numpy()[:, None]], axis=1)
    assert same_bits(np.ascontiguousarray(mine), np.ascontiguousarray(got))


# ------------------------------------------------------------------------------------------ end to end
ITER, LAM0 = 12, 1e-3
MARG = (2, 5)             # the chains whose prior is a chain_marginalize row (non-zero eta0, anchored at the linearisation point)


@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


@pytest.fixture(scope="module")
def priors(eng, pipe):
    """(anchor [C, 16], prior0 [C, 136], prior_idx [C]): a Gaussian on every chain's first state (centre: the unperturbed state, eta0 = 0);
    chains 2 and 5 instead carry the row chain_marginalize gives for their first state at the perturbed states, anchored there."""
    C, G = pipe.C, pipe.G
    lam0 = 0.1 * cc.SCALES ** 2
    P0 = np.zeros((C, 16, 16))
    P0[:, np.arange(15), np.arange(15)] = lam0
    prior0 = _t(cc.pack_upper(P0), eng.device)
    anchor = pipe.pred[0::G].clone()
    rows = eng.chain_marginalize(pipe.hessian(eng), C=C, G=G, prior=pipe.prior, drop=0)
    for c in MARG:
        prior0[c] = rows[c]
        anchor[c] = pipe.states[c * G]
    torch.cuda.synchronize()
    assert (prior0[list(MARG), 120:135].abs().max(1).values > 0).all()
    return anchor, prior0, (torch.arange(C, device=eng.device) * G).to(torch.int32)


def run_lm(eng, pipe, priors, Rt=None, iterations=ITER, buffers=None, states=None, init=True, history=True):
    anchor, prior0, idx = priors
    st = pipe.states.clone() if states is None else states
    hist = torch.zeros((iterations + 1, pipe.C), dtype=torch.float64, device=eng.device) if history else None
    out = eng.chain_lm(1, pipe.meas, pipe.lin, None, st, pipe.Rt if Rt is None else Rt, pipe.C, pipe.G, idx_i=pipe.ii, idx_j=pipe.jj,
                       prior0=prior0, anchor=anchor, prior_idx=idx, lam=LAM0, iterations=iterations, cost_history=hist, buffers=buffers, init=init)
    return out + (hist,)


@pytest.fixture(scope="module")
def eager(eng, pipe, priors):
    out = run_lm(eng, pipe, priors)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def test_chain_lm_converges_to_the_cpu_loops_states(eng, pipe, priors, eager):
    C, G = pipe.C, pipe.G
    states, cost, lam, phase, hist = (t.cpu().numpy() for t in eager)
    print("cost per iteration (rows) and chain (columns):\n%s" % np.array2string(hist, precision=6, max_line_width=200))
    print("lambda %s\nphase %s" % (lam, phase))
    assert (np.diff(hist, axis=0) <= 0).all()                                 # non-increasing per chain
    assert (phase == lc.CONVERGED).all()
    assert same_bits(hist[-1], cost)
    anchor, prior0, _ = priors
    loop = lc.CpuLoop(anchor.cpu().numpy(), prior0.cpu().numpy())
    r_states, r_cost, r_lam, r_phase, r_hist = loop.run(pipe.states.cpu().numpy(), LAM0, ITER)
    print("the CPU loop: cost %s\nphase %s" % (r_cost, r_phase))
    assert (r_phase == lc.CONVERGED).all()
    # sigma at the final states: the undamped system there, factorised and inverted block by block
    st = eager[0]
    prior, _ = eng.prior_relinearize(st, anchor, prior0, idx=priors[2])
    ws = torch.empty((eng.chain_solve_workspace_doubles(C * G),), dtype=torch.float64, device=eng.device)
    status = torch.zeros((C,), dtype=torch.int32, device=eng.device)
    eng.chain_solve(eng.factor_hessian(1, pipe.meas, pipe.lin, None, st, pipe.Rt, pipe.ii, pipe.jj), C=C, G=G, prior=prior, status=status, workspace=ws)
    cov = eng.chain_marginals(ws, C=C, G=G, status=status).cpu().numpy()
    sigma = np.sqrt(cov[:, [cc.tri(i) + i for i in range(15)]])
    d = lc.oracle_local(states, r_states)
    worst = float(np.abs(d / sigma).max())
    print("final states against the CPU loop: %.3g sigma (gate %.3g), cost difference %.3g" % (worst, lc.GATE_FINAL_DEVICE, np.abs(cost - r_cost).max()))
    assert status.cpu().tolist() == [0] * C and worst <= lc.GATE_FINAL_DEVICE


def test_a_chain_with_a_nan_covariance_gives_up_alone(eng, pipe, priors, eager):
    C, G, bad = pipe.C, pipe.G, 3
    P = pipe.meas["P_sym"].clone()
    P[bad * (G - 1) + 2] = float("nan")
    Rt = eng.sqrt_information(P)
    states, cost, lam, phase, hist = run_lm(eng, pipe, priors, Rt=Rt)
    torch.cuda.synchronize()
    print("phase %s lambda %s" % (phase.cpu().tolist(), lam.cpu().tolist()))
    others = [c for c in range(C) if c != bad]
    assert phase[bad].item() == lc.GAVE_UP and (phase[others] == lc.CONVERGED).all()
    rows = slice(bad * G, (bad + 1) * G)
    assert torch.equal(states[rows], pipe.states[rows])                       # untouched
    keep = torch.ones(C * G, dtype=torch.bool, device=eng.device)
    keep[rows] = False
    assert torch.equal(states[keep], eager[0][keep])                          # the others: the bits of the run without it
    assert torch.equal(cost[others], eager[1][others]) and torch.equal(lam[others], eager[2][others])


def test_one_iteration_as_a_graph_replayed(eng, pipe, priors, eager):
    bufs = {}
    st = pipe.states.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_lm(eng, pipe, priors, iterations=1, buffers=bufs, states=st, history=False)      # warm-up on a side stream; fills bufs
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_lm(eng, pipe, priors, iterations=1, buffers=bufs, states=st, init=False, history=False)
    st.copy_(pipe.states)                                                     # back to the start: states, lambda, phase, then cost and chi2 (init)
    bufs["lam"].fill_(LAM0)
    bufs["phase"].zero_()
    run_lm(eng, pipe, priors, iterations=0, buffers=bufs, states=st, history=False)
    for _ in range(ITER):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st, eager[0]) and torch.equal(bufs["cost"], eager[1]) and torch.equal(bufs["lam"], eager[2]) and torch.equal(bufs["phase"], eager[3])
