"""GPU: cpi_chain_solve_batch against the longdouble reference of tests/chain_cases.py, at the smallest shapes where the kernel can go
wrong: a wavefront that is a quarter full, different trip counts inside one wavefront, chains of one, two and three states, explicit
first / ffirst with gaps and in reverse order, more than one workgroup.  Bits: a chain does not depend on its neighbours or on its
position; the host form is the device form; a failed or refused chain is NaN and alone.  The device's own hess: preintegrate ->
sqrt_information -> factor_hessian -> chain_solve -> retract -> factor_cost, eager and captured into one graph.
Both metrics of a comparison are printed before anything is asserted; the gates are those of tests/chain_cases.py."""
import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import chain_pipeline as cp

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def solve(eng, b, lam=None, diagonal=False, explicit=None, host=False, chains=None, G=None, with_prior=True):
    """chain_solve of batch b -> (delta [S, 15] numpy with the sentinel in rows nobody wrote, status [C]).  chains: solve only these
    (in this order) through explicit first / count / ffirst."""
    dev = "cpu" if host else eng.device
    explicit = b.explicit if explicit is None else explicit
    idx = np.arange(b.C) if chains is None else np.asarray(chains)
    kw = {}
    if explicit or chains is not None:
        kw = dict(first=_t(b.first[idx], dev), ffirst=_t(b.ffirst[idx], dev), count=_t(b.count[idx], dev))
    elif (b.count != b.G).any():
        kw = dict(count=_t(b.count, dev))
    out = torch.full((b.S, 15), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((len(idx),), 99, dtype=torch.int32, device=dev)
    lam_t = None if lam is None else _t(np.asarray(lam, dtype=np.float64)[idx], dev)
    fn = eng.chain_solve_host if host else eng.chain_solve
    fn(_t(b.hess, dev), C=len(idx), G=b.G if G is None else G, prior=_t(b.prior, dev) if with_prior else None, lam=lam_t, damping="diagonal" if diagonal else "identity",
       out=out, status=status, **kw)
    if not host:
        torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def untouched_rows(b, chains=None):
    m = np.ones(b.S, dtype=bool)
    for c in (range(b.C) if chains is None else chains):
        m[b.rows(c)] = False
    return m


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("prior_all", [False, True], ids=["prior_first", "prior_all"])
@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_against_the_longdouble_reference(eng, layout, prior_all):
    counts, how = cc.LAYOUTS[layout]
    b = cc.Batch(counts, seed=3, prior_all=prior_all, layout=how)
    worst = [0.0, 0.0]
    for dname, lam_v, diagonal in cc.DAMPINGS:
        lam = cc.lam_of(b, lam_v)
        ref = cc.Reference(b, lam, diagonal)
        ref.check_inputs()
        delta, status = solve(eng, b, lam, diagonal)
        a, bb = ref.metrics(delta)
        print("%s prior %s damping %s: cond max %.1e, (a) %.3e (b) %.3e" % (layout, "all" if prior_all else "first", dname, ref.cond.max(), a, bb))
        assert (status == 0).all(), status
        assert (delta[untouched_rows(b)] == SENTINEL).all()                  # rows of no chain are not written
        worst = [max(worst[0], a), max(worst[1], bb)]
    print("largest (a) %.3e (gate %.2e), (b) %.3e (gate %.2e)" % (worst[0], cc.GATE_BACKWARD_DEVICE, worst[1], cc.GATE_FORWARD_DEVICE))
    assert worst[0] <= cc.GATE_BACKWARD_DEVICE and worst[1] <= cc.GATE_FORWARD_DEVICE


def test_without_a_prior(eng):
    """prior == NULL: the blocks are the factors' alone, identity damping makes them definite; a chain of one state is lambda delta = 0."""
    b = cc.Batch(cc.RAGGED, seed=3)
    lam = cc.lam_of(b, 3.0)
    ref = cc.Reference(b, lam, False, with_prior=False)
    ref.check_inputs()
    delta, status = solve(eng, b, lam, False, with_prior=False)
    host, sh = solve(eng, b, lam, False, with_prior=False, host=True)
    a, bb = ref.metrics(delta)
    print("no prior, identity damping: cond max %.1e, (a) %.3e (b) %.3e" % (ref.cond.max(), a, bb))
    assert (status == 0).all() and a <= cc.GATE_BACKWARD_DEVICE and bb <= cc.GATE_FORWARD_DEVICE
    assert np.array_equal(delta, host) and np.array_equal(status, sh)
    assert (delta[untouched_rows(b)] == SENTINEL).all()
    for c in range(b.C):
        if b.count[c] == 1:
            assert (delta[b.rows(c)] == 0.0).all(), c


# ------------------------------------------------------------------------------------------ 2. bits do not depend on the neighbours
@pytest.mark.parametrize("diagonal", [False, True], ids=["identity", "diagonal"])
def test_a_chain_does_not_depend_on_its_neighbours_or_its_position(eng, diagonal):
    b = cc.Batch(cc.RAGGED, seed=3, prior_all=True)
    lam = cc.lam_of(b, 0.25)
    whole, status = solve(eng, b, lam, diagonal)
    assert (status == 0).all()
    for c in range(b.C):                                                      # every chain alone, C = 1
        alone, st = solve(eng, b, lam, diagonal, chains=[c])
        assert st.tolist() == [0] and np.array_equal(alone[b.rows(c)], whole[b.rows(c)]), c
        assert (alone[untouched_rows(b, [c])] == SENTINEL).all(), c
        short, st = solve(eng, b, lam, diagonal, chains=[c], G=max(int(b.count[c]), 1))   # ... and with G = its own length
        assert np.array_equal(short[b.rows(c)], whole[b.rows(c)]), c
    perm = np.random.default_rng(1).permutation(b.C)
    mixed, status = solve(eng, b, lam, diagonal, chains=perm)
    assert (status == 0).all() and np.array_equal(mixed, whole)
    none, _ = solve(eng, b, None, diagonal)                                   # lambda NULL = zeros
    zeros, _ = solve(eng, b, np.zeros(b.C), diagonal)
    assert np.array_equal(none, zeros)


# ------------------------------------------------------------------------------------------ 3. the host form
@pytest.mark.parametrize("layout", ["ragged", "reverse", "one_1"])
def test_the_host_form_is_the_device_form(eng, layout):
    counts, how = cc.LAYOUTS[layout]
    b = cc.Batch(counts, seed=3, prior_all=False, layout=how)
    for dname, lam_v, diagonal in cc.DAMPINGS:
        lam = cc.lam_of(b, lam_v)
        dev, sd = solve(eng, b, lam, diagonal)
        host, sh = solve(eng, b, lam, diagonal, host=True)
        assert np.array_equal(sd, sh) and np.array_equal(dev, host), (layout, dname)
    with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain 5 leave"):
        bad = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
        bad.ffirst[5] = bad.F - 3
        solve(eng, bad, host=True)


# ------------------------------------------------------------------------------------------ 4. a failed chain is NaN and alone
def test_a_failed_chain_is_nan_and_alone(eng):
    b = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
    good, status = solve(eng, b)
    assert (status == 0).all()
    b.prior[b.first[4] + 3, 2 + 2 * 3 // 2] = -1e9                           # entry (2, 2) of the block of state 3 of chain 4: indefinite
    b.ffirst[6] = b.F - 1                                                     # chain 6 (5 states): its factor rows leave [0, F)
    bad, status = solve(eng, b)
    assert status[4] == 4 and status[6] == -1 and [int(s) for k, s in enumerate(status) if k not in (4, 6)] == [0] * 9, status
    assert np.isnan(bad[b.rows(4)]).all() and np.isnan(bad[b.rows(6)]).all()
    for c in range(b.C):
        if c not in (4, 6):
            assert np.array_equal(bad[b.rows(c)], good[b.rows(c)]), c
    assert (bad[untouched_rows(b)] == SENTINEL).all()


# ------------------------------------------------------------------------------------------ 5. / 6. the device's own hess
class Pipeline:
    """The chains of tests/chain_pipeline.py on the device: preintegrate -> sqrt_information -> the predicted chain -> states retracted
    from it by the seeded step; the prior of every chain's first state is centred on the unperturbed state."""
    C, G = cp.C, cp.G

    def __init__(self, eng):
        C, G = self.C, self.G
        dev = eng.device
        x = {k: v.to(dev) for k, v in cp.inputs().items()}
        self.lin = x["lin"]
        self.meas = eng.preintegrate(x["knots"], x["lin"], x["q"], eng.make_params(1), want=("mean", "jac", "cov_sym"))
        self.Rt = eng.sqrt_information(self.meas["P_sym"])
        self.ii, self.jj = (t.to(dev) for t in eng.chain_indices(C, G))
        assert np.array_equal(self.ii.cpu().numpy(), cp.indices()[0]) and np.array_equal(self.jj.cpu().numpy(), cp.indices()[1])
        pred = torch.zeros((C * G, 16), dtype=torch.float64, device=dev)
        pred[0::G] = x["x0"]
        first_factor = torch.arange(C, device=dev) * (G - 1)
        for k in range(G - 1):                                                # state k + 1 of every chain from state k
            sub = {n: v[first_factor + k].contiguous() for n, v in self.meas.items() if not n.startswith("_")}
            pred[k + 1::G] = eng.predict(1, sub, pred[k::G].contiguous())
        self.pred = pred
        self.states = eng.retract(pred, x["step"])
        xi0 = eng.local_coordinates(self.states[0::G].contiguous(), pred[0::G].contiguous())     # where the prior's centre sits, seen from the state
        torch.cuda.synchronize()
        self.prior = _t(cp.packed_prior(xi0.cpu().numpy()), dev)

    def hessian(self, eng, out=None):
        return eng.factor_hessian(1, self.meas, self.lin, None, self.states, self.Rt, self.ii, self.jj, out=out)

    def cost(self, eng, states, out=None):
        return eng.factor_cost(1, self.meas, self.lin, None, states, self.Rt, self.ii, self.jj, out=out)


@pytest.fixture(scope="module")
def pipe(eng):
    return Pipeline(eng)


def test_the_step_from_the_devices_own_hess(eng, pipe):
    C, G = pipe.C, pipe.G
    hess = pipe.hessian(eng)
    status = torch.full((C,), 99, dtype=torch.int32, device=eng.device)
    delta = eng.chain_solve(hess, C=C, G=G, prior=pipe.prior, status=status)
    before = pipe.cost(eng, pipe.states)["total"].item()
    after = pipe.cost(eng, eng.retract(pipe.states, delta))["total"].item()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * C
    b = cc.Batch.from_arrays([G] * C, np.arange(C) * G, np.arange(C) * (G - 1), hess.cpu().numpy(), pipe.prior.cpu().numpy())
    ref = cc.Reference(b)
    ref.check_inputs()
    a, bb = ref.metrics(delta.cpu().numpy())
    print("device hess: cond max %.1e, (a) %.3e (gate %.2e), (b) %.3e (gate %.2e); cost before %.6e, after %.6e"
          % (ref.cond.max(), a, cc.GATE_BACKWARD_DEVICE, bb, cc.GATE_FORWARD_DEVICE, before, after))
    assert a <= cc.GATE_BACKWARD_DEVICE and bb <= cc.GATE_FORWARD_DEVICE
    assert after < before


def test_the_iteration_captures_into_one_graph(eng, pipe):
    """factor_hessian -> chain_solve -> retract -> factor_cost captured once and replayed twice: the bits of the eager calls."""
    C, G = pipe.C, pipe.G
    S, F = C * G, C * (G - 1)
    dev = eng.device
    e_hess = pipe.hessian(eng)
    e_status = torch.zeros((C,), dtype=torch.int32, device=dev)
    e_delta = eng.chain_solve(e_hess, C=C, G=G, prior=pipe.prior, lam=0.5, damping="diagonal", status=e_status)
    e_trial = eng.retract(pipe.states, e_delta)
    e_cost = pipe.cost(eng, e_trial)
    torch.cuda.synchronize()
    hess = torch.empty((F, 496), dtype=torch.float64, device=dev)
    delta = torch.empty((S, 15), dtype=torch.float64, device=dev)
    status = torch.empty((C,), dtype=torch.int32, device=dev)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    lam = torch.full((1,), 0.5, dtype=torch.float64, device=dev)              # one element: expanded on the device, no host read
    trial = torch.empty_like(pipe.states)
    cost = {k: torch.zeros_like(v) for k, v in e_cost.items() if k != "total"}

    def call():
        pipe.hessian(eng, out=hess)
        eng.chain_solve(hess, C=C, G=G, prior=pipe.prior, lam=lam, damping="diagonal", out=delta, status=status, workspace=ws)
        eng.retract(pipe.states, delta, out=trial)
        pipe.cost(eng, trial, out=cost)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                                # warm-up on a side stream, as graph capture requires
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for v in (hess, delta, trial, cost["chi2"]):
            v.fill_(-1.0)
        status.fill_(99)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(hess, e_hess) and torch.equal(delta, e_delta) and torch.equal(status, e_status) and torch.equal(trial, e_trial)
        assert torch.equal(cost["chi2"], e_cost["chi2"]) and torch.equal(cost["total"], e_cost["total"])


# ------------------------------------------------------------------------------------------ 7. more than one workgroup
def test_many_chains(eng):
    b = cc.Batch([5] * 1000, seed=5)
    ref = cc.Reference(b)
    ref.check_inputs()
    delta, status = solve(eng, b)
    a, bb = ref.metrics(delta)
    print("C = 1000, G = 5: (a) %.3e (gate %.2e), (b) %.3e (gate %.2e)" % (a, cc.GATE_BACKWARD_DEVICE, bb, cc.GATE_FORWARD_DEVICE))
    assert (status == 0).all() and a <= cc.GATE_BACKWARD_DEVICE and bb <= cc.GATE_FORWARD_DEVICE
    assert np.array_equal(cpi_amd.chain_solve(_t(b.hess, eng.device), C=b.C, G=b.G, prior=_t(b.prior, eng.device)).cpu().numpy(), delta)
