"""GPU: cpi_chain_marginals_batch -- the device solve feeding the device marginals -- against the longdouble dense inverse of
tests/marginals_cases.py, at the smallest shapes where the kernel can go wrong: a wavefront that is a quarter full, different trip
counts inside one wavefront, chains of one, two and three states, explicit first with gaps and in reverse order, more than one
workgroup with a last wavefront one chain short.  Bits: a chain does not depend on its neighbours or on its position; the host form
is the device form; a failed chain is NaN and alone.  The device's own hess: the marginals whiten a carried prior, and
factor_hessian -> chain_solve -> chain_marginals replays from one graph.
The metric of a comparison is printed before anything is asserted; the gate is that of tests/marginals_cases.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import chain_pipeline as cp
from tests import marginals_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def marginals(eng, b, lam=None, chains=None, use_status=True, host=False, cross=True):
    """chain_solve (identity damping lam) then chain_marginals of batch b -> (cov [S, 120], cross [S, 225], status [C]) as numpy, NaN in
    what nobody wrote.  chains: only these (in this order) through explicit first / count / ffirst."""
    dev = "cpu" if host else eng.device
    idx = np.arange(b.C) if chains is None else np.asarray(chains)
    kw = {}
    if b.explicit or chains is not None:
        kw = dict(first=_t(b.first[idx], dev), count=_t(b.count[idx], dev))
    elif (b.count != b.G).any():
        kw = dict(count=_t(b.count, dev))
    cov = torch.full((b.S, 120), float("nan"), dtype=torch.float64, device=dev)
    crs = torch.full((b.S, 225), float("nan"), dtype=torch.float64, device=dev) if cross else None
    status = torch.full((len(idx),), 99, dtype=torch.int32, device=dev)
    hess, prior = _t(b.hess, dev), _t(b.prior, dev)
    if host:
        assert lam is None
        ff = dict(ffirst=_t(b.ffirst[idx], dev)) if "first" in kw else {}
        eng.chain_marginals_host(hess, C=len(idx), G=b.G, prior=prior, cross=crs if cross else False, out=cov, status=status, **kw, **ff)
    else:
        ff = dict(ffirst=_t(b.ffirst[idx], dev)) if "first" in kw else {}
        ws = torch.full((eng.chain_solve_workspace_doubles(b.S),), float("nan"), dtype=torch.float64, device=dev)
        lam_t = None if lam is None else _t(np.asarray(lam, dtype=np.float64)[idx], dev)
        eng.chain_solve(hess, C=len(idx), G=b.G, prior=prior, lam=lam_t, status=status, workspace=ws, out=torch.empty((b.S, 15), dtype=torch.float64, device=dev),
                        **kw, **ff)
        eng.chain_marginals(ws, C=len(idx), G=b.G, status=status if use_status else None, out=cov, cross=crs, **kw)
        torch.cuda.synchronize()
    return cov.cpu().numpy(), (crs.cpu().numpy() if cross else None), status.cpu().numpy()


def check_unwritten(b, cov, cross, chains=None):
    none = mc.untouched_rows(b, chains)
    assert np.isnan(cov[none]).all() and np.isnan(cross[none]).all()          # rows of no chain
    assert np.isnan(cross[mc.last_rows(b, chains)]).all()                     # the cross row of a chain's last state
    last = np.zeros(b.S, dtype=bool)
    last[mc.last_rows(b, chains)] = True
    assert np.isfinite(cov[~none]).all() and np.isfinite(cross[~none & ~last]).all()


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("prior_all", [False, True], ids=["prior_first", "prior_all"])
@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_against_the_longdouble_inverse(eng, layout, prior_all):
    worst = 0.0
    for lam_v in (None, 3.0):                                                 # undamped, and the damped matrix's own inverse
        b, lam, ref = mc.case(layout, prior_all, lam_v)
        cov, cross, status = marginals(eng, b, lam)
        m = ref.metric(cov, cross)
        print("%s prior %s lambda %s: cond max %.1e, metric %.3e" % (layout, "all" if prior_all else "first", lam_v, ref.cond.max(), m))
        assert (status == 0).all(), status
        check_unwritten(b, cov, cross)
        M = mc.unpack_cov(cov[~mc.untouched_rows(b)])
        assert np.isfinite(np.linalg.cholesky(M)).all()
        worst = max(worst, m)
    print("largest metric %.3e (floor %.3e, gate %.2e)" % (worst, mc.FLOOR_DEVICE, mc.GATE_DEVICE))
    assert worst <= mc.GATE_DEVICE


# ------------------------------------------------------------------------------------------ 2. more than one workgroup; bits
def test_many_chains_and_a_chain_alone_or_elsewhere(eng):
    b = cc.Batch([5] * 1031, seed=5)                                          # 258 wavefronts, the last one chain short
    ref = mc.Reference(b)
    ref.check_inputs()
    cov, cross, status = marginals(eng, b)
    m = ref.metric(cov, cross)
    print("C = 1031, G = 5: metric %.3e (gate %.2e)" % (m, mc.GATE_DEVICE))
    assert (status == 0).all() and m <= mc.GATE_DEVICE
    check_unwritten(b, cov, cross)
    for c in (0, 514, 1027, 1028, 1029, 1030):                                # alone, C = 1: its own bits and nothing else written
        one, onex, st = marginals(eng, b, chains=[c])
        assert st.tolist() == [0] and np.array_equal(one[b.rows(c)], cov[b.rows(c)]) and np.array_equal(onex[b.rows(c)][:-1], cross[b.rows(c)][:-1]), c
        check_unwritten(b, one, onex, [c])
    perm = np.random.default_rng(1).permutation(b.C)                          # every chain at another position
    mixed, mixedx, st = marginals(eng, b, chains=perm)
    assert (st == 0).all() and np.array_equal(mixed, cov) and np.array_equal(mixedx, cross, equal_nan=True)
    assert np.array_equal(cpi_amd.chain_marginals(*_solved(eng, b), C=b.C, G=b.G).cpu().numpy(), cov)   # the module-level entry, cov alone


def _solved(eng, b):
    ws = torch.empty((eng.chain_solve_workspace_doubles(b.S),), dtype=torch.float64, device=eng.device)
    eng.chain_solve(_t(b.hess, eng.device), C=b.C, G=b.G, prior=_t(b.prior, eng.device), workspace=ws)
    return (ws,)


def test_a_ragged_chain_does_not_depend_on_its_wavefront_mates(eng):
    b, _, _ = mc.case("reverse", True)
    cov, cross, status = marginals(eng, b)
    assert (status == 0).all()
    for c in range(b.C):
        if b.count[c] > 0:
            one, onex, _ = marginals(eng, b, chains=[c])
            assert np.array_equal(one[b.rows(c)], cov[b.rows(c)]) and np.array_equal(onex[b.rows(c)], cross[b.rows(c)], equal_nan=True), c


# ------------------------------------------------------------------------------------------ 3. failed chains
def test_a_failed_chain_is_nan_and_alone(eng):
    """The non-positive-definite construction of tests/test_gpu_chain.py: arithmetic on NaN, not a fault."""
    b = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
    good, goodx, status = marginals(eng, b)
    assert (status == 0).all()
    b.prior[b.first[4] + 3, 2 + 2 * 3 // 2] = -1e9                           # entry (2, 2) of the block of state 3 of chain 4: indefinite
    b.ffirst[6] = b.F - 1                                                     # chain 6 (5 states): its factor rows leave [0, F)
    bad, badx, status = marginals(eng, b)
    assert status[4] == 4 and status[6] == -1 and [int(s) for k, s in enumerate(status) if k not in (4, 6)] == [0] * 9, status
    for c in (4, 6):
        assert np.isnan(bad[b.rows(c)]).all() and np.isnan(badx[b.rows(c)]).all()
    for c in range(b.C):
        if c not in (4, 6):
            assert np.array_equal(bad[b.rows(c)], good[b.rows(c)]) and np.array_equal(badx[b.rows(c)], goodx[b.rows(c)], equal_nan=True), c
    assert np.isnan(bad[mc.untouched_rows(b)]).all()


def test_status_none_computes_every_chain(eng):
    b, _, ref = mc.case("ragged", False)
    cov, cross, _ = marginals(eng, b)
    free, freex, _ = marginals(eng, b, use_status=False)
    assert np.array_equal(free, cov, equal_nan=True) and np.array_equal(freex, cross, equal_nan=True)
    only, none, _ = marginals(eng, b, cross=False)                            # cross NULL: cov alone, the same bits
    assert none is None and np.array_equal(only, cov, equal_nan=True)


# ------------------------------------------------------------------------------------------ 4. the host form
@pytest.mark.parametrize("layout", ["ragged", "reverse", "one_1"])
def test_the_host_form_is_the_device_form(eng, layout):
    b, _, _ = mc.case(layout, False)
    dev, devx, sd = marginals(eng, b)
    host, hostx, sh = marginals(eng, b, host=True)
    assert np.array_equal(sd, sh) and np.array_equal(dev, host, equal_nan=True) and np.array_equal(devx, hostx, equal_nan=True)
    if layout == "ragged":
        bad = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
        bad.ffirst[5] = bad.F - 3
        with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain 5 leave"):
            marginals(eng, bad, host=True)


# ------------------------------------------------------------------------------------------ 5. / 6. the device's own hess
@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


def test_a_marginal_whitens_a_carried_prior(eng, pipe):
    """eng.sqrt_information(cov) of every state is the R of a prior with that covariance: R^T R cov = I, at the gate of
    tests/test_gpu_whitening.py (1e-7, there on R P R^T)."""
    C, G = pipe.C, pipe.G
    S = C * G
    hess = pipe.hessian(eng)
    status = torch.full((C,), 99, dtype=torch.int32, device=eng.device)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=eng.device)
    eng.chain_solve(hess, C=C, G=G, prior=pipe.prior, status=status, workspace=ws)
    cov, cross = eng.chain_marginals(ws, C=C, G=G, status=status, cross=True)
    Rt = eng.sqrt_information(cov)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * C
    b = cc.Batch.from_arrays([G] * C, np.arange(C) * G, np.arange(C) * (G - 1), hess.cpu().numpy(), pipe.prior.cpu().numpy())
    ref = mc.Reference(b)
    ref.check_inputs()
    m = ref.metric(cov.cpu().numpy(), cross.cpu().numpy())
    R = cpi_amd.unpack_tri(Rt).cpu().numpy().reshape(S, 15, 15).transpose(0, 2, 1)     # column-major -> [row][col]
    P = mc.unpack_cov(cov.cpu().numpy())
    e_sym = np.abs(np.einsum("fij,fjk,flk->fil", R, P, R) - np.eye(15)).max()
    e_lit = np.abs(np.einsum("fji,fjk,fkl->fil", R, R, P) - np.eye(15)).max()
    print("device hess: cond max %.1e, metric %.3e (gate %.2e); |R cov R^T - I| %.3e, |R^T R cov - I| %.3e (gate 1e-7)"
          % (ref.cond.max(), m, mc.GATE_DEVICE, e_sym, e_lit))
    assert m <= mc.GATE_DEVICE
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diagonal(R, axis1=1, axis2=2) > 0)
    assert e_sym < 1e-7 and e_lit < 1e-7


def test_hessian_solve_marginals_capture_into_one_graph(eng, pipe):
    """factor_hessian -> chain_solve(lam=None) -> chain_marginals captured once; replayed, and replayed again after the states changed
    in place: the bits of the eager calls at those states."""
    C, G = pipe.C, pipe.G
    S, F = C * G, C * (G - 1)
    dev = eng.device
    states_a = pipe.states.clone()
    states_b = eng.retract(states_a, 0.1 * _t(cp.inputs()["step"].numpy(), dev))
    x = states_a.clone()
    saved, pipe.states = pipe.states, x

    def run(hess, delta, status, ws, cov, cross):
        pipe.hessian(eng, out=hess)
        eng.chain_solve(hess, C=C, G=G, prior=pipe.prior, out=delta, status=status, workspace=ws)
        eng.chain_marginals(ws, C=C, G=G, status=status, out=cov, cross=cross)

    def buffers():
        return (torch.empty((F, 496), dtype=torch.float64, device=dev), torch.empty((S, 15), dtype=torch.float64, device=dev),
                torch.empty((C,), dtype=torch.int32, device=dev), torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev),
                torch.empty((S, 120), dtype=torch.float64, device=dev), torch.empty((S, 225), dtype=torch.float64, device=dev))
    try:
        eager = {}
        for name, st in (("a", states_a), ("b", states_b)):
            x.copy_(st)
            eager[name] = buffers()
            eager[name][5].fill_(-1.0)                                        # the cross rows of last states are not written
            run(*eager[name])
        torch.cuda.synchronize()
        assert not torch.equal(eager["a"][4], eager["b"][4])
        x.copy_(states_a)
        bufs = buffers()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            run(*bufs)                                                        # warm-up on a side stream, as graph capture requires
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run(*bufs)
        for name, st in (("a", states_a), ("b", states_b), ("a", states_a)):
            x.copy_(st)
            for v in (bufs[0], bufs[1], bufs[4], bufs[5]):
                v.fill_(-1.0)
            bufs[2].fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            for k in (0, 1, 2, 4, 5):
                assert torch.equal(bufs[k], eager[name][k]), (name, k)
            assert bufs[2].cpu().tolist() == [0] * C
    finally:
        pipe.states = saved


# ------------------------------------------------------------------------------------------ 7. the C++ facade
def test_marginals_cpp_facade():
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_marginals")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_marginals.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.splitlines()[-1] == "test_marginals ok 5 4", p.stdout
