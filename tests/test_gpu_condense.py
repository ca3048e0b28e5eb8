"""GPU: cpi_chain_condense_batch / cpi_chain_expand_batch against the longdouble references of tests/condense_cases.py, at the smallest
shapes where the kernels change path: counts [0, 1, 2, 3, K, K + 1, K + 2, 2K, 2K + 1, 2K + 2] for K in {1, 2, 4, 7} (no interior, one
interior, a tail segment of one factor, exact multiples, a chain that is a single segment) in the layouts tile / gaps / reverse,
chains of 5 and 6 segments whose segments share wavefronts, one chain of 100 states at K = 12 beside short ones, both dampings with a
lambda per chain, with and without priors; the rows nothing owns hold NaN (cc.Batch).
(i) delta against the longdouble reference; (ii) chain_solve_segmented against chain_solve; (iii) the reduced solve's marginals are the
full chain's at the separators; (iv) a failed interior; (v) a chain's bits do not depend on C or on its position; (vi) the three calls
replay from one graph; (vii) the refusals; the host forms and the C++ facade are the device forms.
The metrics of a comparison are printed before anything is asserted; the gates are those of tests/condense_cases.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import condense_cases as cd
from tests import marginals_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kw(b, dev):
    """first / count / ffirst of a batch as the entries take them."""
    if b.explicit:
        return dict(first=_t(b.first, dev), count=_t(b.count, dev), ffirst=_t(b.ffirst, dev))
    return dict(count=_t(b.count, dev)) if (b.count != b.G).any() else {}


def run(eng, b, K, lam, diagonal, with_prior=True, host=False, marginals=False, hess=None, prior=None):
    """condense -> chain_solve of the reduced chains -> expand, call by call, every output pre-filled with a sentinel; numpy results."""
    dev = "cpu" if host else eng.device
    Gr = cd.reduced_states(b.G, K)
    f64 = lambda *s: torch.full(s, cd.SENTINEL, dtype=torch.float64, device=dev)
    i32 = lambda n: torch.full((n,), 99, dtype=torch.int32, device=dev)
    kw = _kw(b, dev)
    damping = "diagonal" if diagonal else "identity"
    pr = _t(b.prior if prior is None else prior, dev) if with_prior else None
    seg = i32(b.C * (Gr - 1))
    ws = torch.full((eng.chain_condense_workspace_doubles(b.S),), float("nan"), dtype=torch.float64, device=dev)
    fn = eng.chain_condense_host if host else eng.chain_condense
    rhess, rprior, rcount, gr, ws = fn(_t(b.hess if hess is None else hess, dev), K, C=b.C, G=b.G, prior=pr, lam=_t(lam, dev), damping=damping, S=b.S,
                                       rhess=f64(b.C * (Gr - 1), 496), rprior=f64(b.C * Gr, 136), rcount=i32(b.C), status=seg, workspace=ws, **kw)
    assert gr == Gr
    status = i32(b.C)
    rdelta = f64(b.C * Gr, 15)
    res = {}
    if host:
        eng.chain_solve_host(rhess if Gr > 1 else None, C=b.C, G=Gr, count=rcount, prior=rprior, out=rdelta, status=status)
    else:
        sws = torch.full((eng.chain_solve_workspace_doubles(b.C * Gr),), float("nan"), dtype=torch.float64, device=dev)
        eng.chain_solve(rhess if Gr > 1 else None, C=b.C, G=Gr, count=rcount, prior=rprior, out=rdelta, status=status, workspace=sws)
        if marginals:
            cov, cross = eng.chain_marginals(sws, C=b.C, G=Gr, count=rcount, status=status, cross=True)
            res.update(cov=cov.cpu().numpy(), cross=cross.cpu().numpy())
    ekw = {k: v for k, v in kw.items() if k != "ffirst"}
    delta = (eng.chain_expand_host if host else eng.chain_expand)(rdelta, ws, K, C=b.C, G=b.G, out=f64(b.S, 15), **ekw)
    if not host:
        torch.cuda.synchronize()
    res.update(rhess=rhess.cpu().numpy(), rprior=rprior.cpu().numpy(), rcount=rcount.cpu().numpy(), seg_status=seg.cpu().numpy(),
               status=status.cpu().numpy(), rdelta=rdelta.cpu().numpy(), delta=delta.cpu().numpy())
    return res


def solve_plain(eng, b, lam, diagonal, with_prior=True):
    dev = eng.device
    status = torch.full((b.C,), 99, dtype=torch.int32, device=dev)
    delta = eng.chain_solve(_t(b.hess, dev), C=b.C, G=b.G, prior=_t(b.prior, dev) if with_prior else None, lam=_t(lam, dev),
                            damping="diagonal" if diagonal else "identity", status=status,
                            out=torch.full((b.S, 15), cd.SENTINEL, dtype=torch.float64, device=dev), **_kw(b, dev))
    torch.cuda.synchronize()
    return delta.cpu().numpy(), status.cpu().numpy()


WORST = np.zeros(4)


# ------------------------------------------------------------------------------------------ (i) against the reference
@pytest.mark.parametrize("name,k", cd.all_cases())
def test_against_the_longdouble_references(eng, name, k):
    case = cd.case(name, k)
    res = run(eng, case.batch, case.K, case.lam, case.diagonal, case.with_prior)
    WORST[:] = np.maximum(WORST, case.check(res, cd.GATES_DEVICE))
    print("largest so far: (a) %.3e (b) %.3e (r) %.3e (c) %.3e; gates %s" % (*WORST, cd.GATES_DEVICE))
    b, Gr = case.batch, case.Gr
    for c in range(b.C):                                                     # rows of reduced slots beyond m_c are not written
        m = cd.reduced_states(int(b.count[c]), case.K)
        assert (res["rprior"][c * Gr + m:(c + 1) * Gr] == cd.SENTINEL).all()
        assert (res["rhess"][c * (Gr - 1) + max(m - 1, 0):(c + 1) * (Gr - 1)] == cd.SENTINEL).all()


# ------------------------------------------------------------------------------------------ (ii) against chain_solve
@pytest.mark.parametrize("name", ["k4_gaps", "k7_reverse", "many", "long"])
def test_segmented_and_plain_solve_agree(eng, name):
    for k in range(len(cd.CASES[name][4])):
        case = cd.case(name, k)
        b, dev = case.batch, eng.device
        status = torch.full((b.C,), 99, dtype=torch.int32, device=dev)
        delta, st = eng.chain_solve_segmented(_t(b.hess, dev), case.K, C=b.C, G=b.G, prior=_t(b.prior, dev) if case.with_prior else None,
                                              lam=_t(case.lam, dev), damping="diagonal" if case.diagonal else "identity", status=status,
                                              out=torch.full((b.S, 15), cd.SENTINEL, dtype=torch.float64, device=dev), **_kw(b, dev))
        plain, st2 = solve_plain(eng, b, case.lam, case.diagonal, case.with_prior)
        assert st is status and (status.cpu().numpy() == 0).all() and (st2 == 0).all()
        delta = delta.cpu().numpy()
        worst = 0.0
        for c in case.full.A:
            x = case.full.x[c]
            if np.any(x):
                d = np.abs(delta[b.rows(c)] - plain[b.rows(c)]).max() / float(np.abs(x).max())
                worst = max(worst, d / (case.full.cond[c] * cc.EPS_HALF))
        gate = cd.GATES_DEVICE[1] + cc.GATE_FORWARD_DEVICE
        print("%s: |segmented - plain| %.3e of cond 2^-53 (gate %.2e)" % (case.name, worst, gate))
        assert worst <= gate
        res = run(eng, b, case.K, case.lam, case.diagonal, case.with_prior)  # the three calls one by one: the same bits
        assert np.array_equal(res["delta"], delta)


# ------------------------------------------------------------------------------------------ (iii) the reduced chain's marginals
@pytest.mark.parametrize("name,k", [("k1_gaps", 0), ("k4_tile", 2), ("k7_reverse", 1), ("many", 0)])
def test_the_reduced_marginals_are_the_separators(eng, name, k):
    case = cd.case(name, k)
    b, Gr, K = case.batch, case.Gr, case.K
    ref = mc.Reference(b, case.lam, case.diagonal, with_prior=case.with_prior)      # the inverse of the DAMPED matrix: what was condensed
    ref.check_inputs()
    res = run(eng, b, K, case.lam, case.diagonal, case.with_prior, marginals=True)
    worst = 0.0
    for c in ref.A:
        n = int(b.count[c])
        seps = cd.separators(n, K)
        D = ref.diag[c][seps]
        sd = np.sqrt(np.einsum("sii->si", D))
        got = mc.unpack_cov(res["cov"][c * Gr:c * Gr + len(seps)]).astype(np.longdouble)
        e = float((np.abs(got - D) / (sd[:, :, None] * sd[:, None, :])).max())
        if K == 1 and n > 1:
            gx = mc.unpack_cross(res["cross"][c * Gr:c * Gr + n - 1]).astype(np.longdouble)
            e = max(e, float((np.abs(gx - ref.cross[c]) / (sd[:-1, :, None] * sd[1:, None, :])).max()))
        worst = max(worst, e / (ref.cond[c] * cc.EPS_HALF))
    print("%s: the reduced marginals against the full inverse at the separators: %.3e (gate %.2e)" % (case.name, worst, mc.GATE_DEVICE))
    assert worst <= mc.GATE_DEVICE


# ------------------------------------------------------------------------------------------ (iv) a failed interior
def test_a_failed_interior_fails_its_segment_and_its_chain_alone(eng):
    good, bad, K, chain, slot, code = cd.failure_plan()
    r0, r1 = run(eng, good, K, None, False), run(eng, bad, K, None, False)
    Gr = cd.reduced_states(good.G, K)
    want = np.zeros(good.C * (Gr - 1), np.int32)
    want[chain * (Gr - 1) + slot] = code
    assert np.array_equal(r1["seg_status"], want) and (r0["seg_status"] == 0).all()
    assert np.isnan(r1["rhess"][chain * (Gr - 1) + slot]).all()
    assert (r1["status"] != 0).tolist() == [c == chain for c in range(good.C)]
    assert np.isnan(r1["delta"][good.rows(chain)]).all()
    others = np.ones(good.S, dtype=bool)
    others[good.rows(chain)] = False
    assert np.array_equal(r1["delta"][others], r0["delta"][others])
    keep = np.ones(good.C * (Gr - 1), dtype=bool)
    keep[chain * (Gr - 1) + slot] = False
    assert np.array_equal(r1["rhess"][keep], r0["rhess"][keep]) and np.array_equal(r1["rprior"], r0["rprior"])


def test_a_refused_chain_is_nan_and_alone(eng):
    b = cc.Batch([6, 9, 3], seed=5, prior_all=True, layout="gaps")
    r0 = run(eng, b, 2, None, False)
    far = cc.clone(b)
    far.ffirst[1] = b.F - 3                                                  # chain 1 (9 states): its factor rows leave [0, F)
    r1 = run(eng, far, 2, None, False)
    Gr = cd.reduced_states(b.G, 2)
    seg = r1["seg_status"].reshape(b.C, Gr - 1)
    assert seg[1].tolist() == [-1] * 4 and (seg[[0, 2]] == 0).all()
    assert r1["status"][1] != 0 and r1["status"][0] == 0 and r1["status"][2] == 0
    assert np.isnan(r1["delta"][b.rows(1)]).all()
    for c in (0, 2):
        assert np.array_equal(r1["delta"][b.rows(c)], r0["delta"][b.rows(c)])


# ------------------------------------------------------------------------------------------ (v) bits
def test_a_chain_does_not_depend_on_c_or_on_its_position(eng):
    case = cd.case("many", 2)
    b, K, Gr = case.batch, case.K, case.Gr
    whole = run(eng, b, K, case.lam, case.diagonal)
    for c in (0, 2, 3):
        n = int(b.count[c])
        one = cc.Batch.from_arrays([n], [1], [2], np.concatenate([np.full((2, 496), np.nan), b.chain(c)[0]]),
                                   np.concatenate([np.full((1, 136), np.nan), b.chain(c)[1]]))
        one.G = b.G                                                          # the same G, so the same Gr
        r = run(eng, one, K, case.lam[c:c + 1], case.diagonal)
        m = cd.reduced_states(n, K)
        assert np.array_equal(r["delta"][1:], whole["delta"][b.rows(c)]), c
        assert np.array_equal(r["rhess"][:m - 1], whole["rhess"][c * (Gr - 1):c * (Gr - 1) + m - 1]), c
        assert np.array_equal(r["rprior"][:m], whole["rprior"][c * Gr:c * Gr + m]), c


# ------------------------------------------------------------------------------------------ (vi) one graph
def test_the_three_calls_replay_from_one_graph(eng):
    case = cd.case("many", 1)
    b, dev = case.batch, eng.device
    hess, prior, lam, count = _t(b.hess, dev), _t(b.prior, dev), _t(case.lam, dev), _t(b.count, dev)

    def buffers():
        bufs = eng.chain_condense_buffers(b.C, b.G, b.S, case.K)
        for t in bufs.values():
            t.fill_(-1.0 if t.dtype == torch.float64 else 99)
        return bufs, torch.full((b.S, 15), -1.0, dtype=torch.float64, device=dev)

    def go(bufs, out):
        eng.chain_solve_segmented(hess, case.K, C=b.C, G=b.G, count=count, prior=prior, lam=lam, out=out, buffers=bufs)

    eager = buffers()
    go(*eager)
    torch.cuda.synchronize()
    assert (eager[0]["status"].cpu().numpy() == 0).all()
    a_, b_ = case.full.metrics(eager[1].cpu().numpy())
    assert b_ <= cd.GATES_DEVICE[1]
    bufs = buffers()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        go(*bufs)                                                            # warm-up on a side stream, as graph capture requires
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        go(*bufs)
    for t in list(bufs[0].values()) + [bufs[1]]:
        t.fill_(-1.0 if t.dtype == torch.float64 else 99)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bufs[1], eager[1])
    for name in ("rhess", "rprior", "rcount", "seg_status", "status", "rdelta"):
        assert torch.equal(bufs[0][name], eager[0][name]), name


# ------------------------------------------------------------------------------------------ (vii) refusals; the host forms; the facade
def test_refusals(eng):
    b = cc.Batch([5, 4], seed=3, prior_all=True)
    dev = eng.device
    hess, prior = _t(b.hess, dev), _t(b.prior, dev)
    with pytest.raises(AssertionError):
        eng.chain_condense(hess, 0, C=b.C, G=b.G, prior=prior)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    Gr = cd.reduced_states(b.G, 2)
    ws = f64(eng.chain_condense_workspace_doubles(b.S))
    args = (eng.ctx, b.C, b.G, b.S, b.F, None, None, None, hess.data_ptr(), prior.data_ptr(), None, 0)
    rh, rp, rc = f64(b.C * (Gr - 1), 496), f64(b.C * Gr, 136), torch.zeros(b.C, dtype=torch.int32, device=dev)
    lib = eng.lib
    for K, rh_, ws_, text in ((0, rh, ws, "K (the factors"), (2, hess, ws, "overlaps"), (2, rh, None, "workspace is NULL")):
        rc_ = lib.cpi_chain_condense_batch(*args, K, rh_.data_ptr(), rp.data_ptr(), rc.data_ptr(), None, None if ws_ is None else ws_.data_ptr())
        assert rc_ == 1 and text in lib.cpi_last_error(eng.ctx).decode(), text
    rd = f64(b.C * Gr, 15)
    rc_ = lib.cpi_chain_expand_batch(eng.ctx, b.C, b.G, b.S, None, None, 2, rd.data_ptr(), ws.data_ptr(), ws.data_ptr())
    assert rc_ == 1 and "overlaps" in lib.cpi_last_error(eng.ctx).decode()
    assert lib.cpi_chain_condense_batch(eng.ctx, 0, b.G, 0, 0, None, None, None, None, None, None, 0, 2, None, None, None, None, None) == 0    # C == 0: a no-op
    g = cc.Batch([5, 4], seed=3, prior_all=True, layout="gaps")
    g.ffirst[1] = g.F - 1
    with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain 1 leave"):
        run(eng, g, 2, None, False, host=True)


@pytest.mark.parametrize("name,k", [("k2_gaps", 2), ("k7_tile", 1), ("many", 3)])
def test_the_host_forms_are_the_device_forms(eng, name, k):
    case = cd.case(name, k)
    dev = run(eng, case.batch, case.K, case.lam, case.diagonal, case.with_prior)
    host = run(eng, case.batch, case.K, case.lam, case.diagonal, case.with_prior, host=True)
    for key in ("rhess", "rprior", "rcount", "seg_status", "status", "delta"):
        assert np.array_equal(dev[key], host[key]), key


def test_condense_cpp_facade(eng):
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_condense")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_condense.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "test_condense ok 3 12 4", p.stdout
    Cn, G, K = 3, 12, 4
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[-1 - Cn * G:-1]])
    P = np.zeros((Cn * G, 16, 16))
    P[0::G, np.arange(15), np.arange(15)] = 1.0
    P[0::G, :15, 15] = P[0::G, 15, :15] = np.arange(1, 16)[None, :] + np.arange(Cn)[:, None]
    H = np.zeros((31, 31))
    H[:30, :30] = np.block([[np.eye(15), -np.eye(15)], [-np.eye(15), np.eye(15)]])
    hess = np.tile(cc.pack_upper(H), (Cn * (G - 1), 1))
    delta, status = cpi_amd.chain_solve_segmented(_t(hess, eng.device), K, C=Cn, G=G, prior=_t(cc.pack_upper(P), eng.device))   # the module-level entry
    assert (status.cpu().numpy() == 0).all() and np.array_equal(delta.cpu().numpy(), got)
