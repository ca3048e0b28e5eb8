"""GPU: cpi_state_between_batch against the references of tests/between_cases.py at the smallest shapes that cross a wavefront of four
factors and a lane group of sixteen (F in 1, 3, 4, 5, 9; 0, 1, 2 and 17 measurements per factor; chained and explicit indices,
positions of 5e6 m, float32-rounded quaternions), the in-place, cost-only and host forms and the C++ facade against the out-of-place
device form bit for bit, and Engine.chain_lm(betweens=...) end to end on the chains of tests/chain_pipeline.py cut to 2 .. 6 states and
whole: eager and as one captured graph.  The figures of a comparison are printed before anything is asserted; the gates are those of
tests/between_cases.py.

The device is held to the reference's gates, not to the host twin's bits: quat_2_Rot and the quaternion product are contracted and
normalised differently on the device (a reciprocal square root; tests/test_gpu_lm.py).  Every test of this file fails where the entry
does not exist."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import between_cases as bc
from tests import chain_cases as cc
from tests import fix_cases as fx
from tests import lm_cases as lc
from tests.test_lm_cpu import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -7.0


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _banded(n, cols, dev, fill=None, odd=False):
    """An output of n rows between two guard rows, NaN-filled (or holding `fill`: the in-place form) -> (the buffer, the view).  odd: the
    view starts at an address that is 8 but not 16 bytes aligned."""
    width = int(np.prod(cols, dtype=np.int64))
    shift = (width + 1) % 2 if odd else 0
    flat = torch.full(((n + 2) * width + shift,), GUARD, dtype=torch.float64, device=dev)
    buf = flat[shift:].view((n + 2,) + cols)
    buf[1:n + 1] = float("nan") if fill is None else _t(fill, dev)
    assert not odd or buf[1:n + 1].data_ptr() % 16 == 8
    return buf, buf[1:n + 1]


def dev_between(eng, c, weight=True, base=True, rows=True, cost=True, chi2_m=True, host=False, inplace=False, z=None, alias=None, bases=None,
                padded=None, wrap=None):
    """state_between on case c -> (hess [F, 496], chi2 [F], chi2_m [M]) as numpy (None where not asked for), outputs between guard rows.
    alias = (hess in place, chi2 in place) and bases = (hess_base given, chi2_base given) where the two arrays differ (inplace and base
    set both).  padded: a between_edge_checks.Padded of the case -- z, R, weight, the states and chi2_m are the interiors of its arrays,
    the inputs are compared with what they were, and chi2_m comes back as the WHOLE buffer [M + 2 PAD].  wrap: what every float64 input
    goes through (tests/test_gpu_lm_edges.odd); the outputs then start at 8 mod 16 as well."""
    dev = "cpu" if host else eng.device
    a_h, a_c = (inplace, inplace) if alias is None else alias
    b_h, b_c = (base, base) if bases is None else bases
    odd = wrap is not None
    w = (lambda t: t) if wrap is None else wrap
    hb, hv = _banded(c.F, (496,), dev, c.base if a_h else None, odd) if rows else (None, None)
    cb, cv = _banded(c.F, (), dev, c.chi2_base if a_c else None, odd) if cost else (None, None)
    xb, xv = _banded(c.M, (), dev, None, odd) if chi2_m else (None, None)
    fn = eng.state_between_host if host else eng.state_between
    b_rows = (hv if a_h else w(_t(c.base, dev))) if b_h and rows else None
    b_chi2 = (cv if a_c else w(_t(c.chi2_base, dev))) if b_c and cost else None
    states, zt, Rt, wt = (w(_t(a, dev)) for a in (c.states, c.z if z is None else z, c.R, c.weight))
    if padded is not None:
        p = padded
        big = {k: _t(v, dev) for k, v in p.big.items()}
        states, zt, Rt, wt = big["states"][p.PADS:p.PADS + c.S], big["z"][p.PAD:p.PAD + c.M], big["R"][p.PAD:p.PAD + c.M], big["weight"][p.PAD:p.PAD + c.M]
        xb, xv = big["chi2_m"], big["chi2_m"][p.PAD:p.PAD + c.M]
    got = fn(states, bc.KINDS[c.kind] if c.F % 2 else c.kind, zt, Rt, _t(c.mfirst, dev), idx_i=_t(c.idx_i, dev), idx_j=_t(c.idx_j, dev),
             weight=wt if weight else None, hess_base=b_rows, chi2_base=b_chi2, out=hv, chi2=cv, chi2_m=xv, want_rows=rows, want_cost=cost)
    if not host:
        torch.cuda.synchronize()
    assert (got[0] is None) == (not rows) and (got[1] is None) == (not cost)
    if padded is not None:
        assert all(same_bits(big[k].cpu().numpy(), v) for k, v in padded.big.items() if k != "chi2_m"), "an input was written"
        for buf, n in ((hb, c.F), (cb, c.F)):
            assert buf is None or ((buf[0] == GUARD).all() and (buf[n + 1] == GUARD).all())
        return tuple(None if v is None else v.cpu().numpy() for v in (hv, cv, xb))
    for buf, n in ((hb, c.F), (cb, c.F), (xb, c.M)):
        assert buf is None or ((buf[0] == GUARD).all() and (buf[n + 1] == GUARD).all())
    return tuple(None if v is None else v.cpu().numpy() for v in (hv, cv, xv))


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_against_the_reference(eng, kind):
    worst = {}
    for name, c in bc.all_cases(kind):
        for weight, base in ((True, True), (False, False)):
            hess, chi2, chi2_m = dev_between(eng, c, weight, base)
            assert not np.isnan(hess).any() and not np.isnan(chi2).any() and not np.isnan(chi2_m).any(), name   # every factor and measurement is written
            m = bc.metrics(hess, chi2, chi2_m, bc.reference(c, weight, base))
            print("device, %s, %s, weight %d base %d: %s" % (bc.KINDS[kind], name, weight, base, ", ".join("%s %.3g" % kv for kv in sorted(m.items()))))
            for k, v in m.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("device, %s: %s (gates %s)" % (bc.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), bc.GATE_DEVICE))
    for k, v in worst.items():
        assert v <= bc.GATE_DEVICE[k], (k, v)


# ------------------------------------------------------------------------------------------ 2. untouched data and the forms
@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_untouched_data_and_form_equivalences(eng, kind):
    for variant in ("chain", "explicit"):
        c = bc.case(kind, 9, variant)
        hess, chi2, chi2_m = dev_between(eng, c)
        none = c.counts == 0
        rest = np.setdiff1d(np.arange(496), bc.touched(kind))
        assert same_bits(hess[none], c.base[none]) and same_bits(chi2[none], c.chi2_base[none])          # factors without measurements
        assert same_bits(np.ascontiguousarray(hess[:, rest]), np.ascontiguousarray(c.base[:, rest]))     # entries outside the touched set
        assert (hess[~none][:, bc.touched(kind)] != c.base[~none][:, bc.touched(kind)]).all()
        z_hess, z_chi2, _ = dev_between(eng, c, base=False)
        assert (z_hess[none] == 0.0).all() and (z_chi2[none] == 0.0).all() and (z_hess[:, rest] == 0.0).all()
        i_hess, i_chi2, i_m = dev_between(eng, c, inplace=True)                                          # in place: the out-of-place call's bits
        assert same_bits(i_hess, hess) and same_bits(i_chi2, chi2) and same_bits(i_m, chi2_m)
        nothing, c_chi2, c_m = dev_between(eng, c, rows=False)                                           # cost only
        assert nothing is None and same_bits(c_chi2, chi2) and same_bits(c_m, chi2_m)
        _, ci_chi2, _ = dev_between(eng, c, rows=False, inplace=True, chi2_m=False)
        assert same_bits(ci_chi2, chi2)
        h_hess, h_chi2, h_m = dev_between(eng, c, host=True)                                             # the host form
        assert same_bits(h_hess, hess) and same_bits(h_chi2, chi2) and same_bits(h_m, chi2_m)
        hi_hess, hi_chi2, _ = dev_between(eng, c, host=True, inplace=True)
        assert same_bits(hi_hess, hess) and same_bits(hi_chi2, chi2)
        only_m = dev_between(eng, c, rows=False, cost=False)[2]
        assert same_bits(only_m, chi2_m)
    c = bc.case(kind, 9)
    hess, chi2, chi2_m = dev_between(eng, c)
    for F in (1, 3, 4, 5):                                                                              # a factor's bits: its own data only
        o, p, x2 = dev_between(eng, bc.case(kind, F))
        assert same_bits(o, hess[:F]) and same_bits(p, chi2[:F]) and same_bits(x2, chi2_m[:len(x2)]), F
    if bc.ROT[kind]:                                                                                    # z and -z: one rotation
        z = c.z.copy()
        z[:, :4] = -z[:, :4]
        o, p, x2 = dev_between(eng, c, z=z)
        assert np.array_equal(o, hess) and np.array_equal(p, chi2) and np.array_equal(x2, chi2_m)


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_a_nan_measurement_poisons_its_own_factor_only(eng, kind):
    c = bc.case(kind, 9)
    hess, chi2, chi2_m = dev_between(eng, c)
    rest = np.setdiff1d(np.arange(496), bc.touched(kind))
    for col in (0, bc.ZN[kind] - 1):
        bad = c.z.copy()
        m = int(c.mfirst[5]) + 3
        bad[m, col] = np.nan
        for inplace in (False, True):
            o, p, x2 = dev_between(eng, c, z=bad, inplace=inplace)
            keep = np.arange(c.F) != 5
            assert same_bits(o[keep], hess[keep]) and same_bits(p[keep], chi2[keep])
            assert np.isnan(p[5]) and np.isnan(o[5, 495]) and np.isnan(x2[m]) and same_bits(np.delete(x2, m), np.delete(chi2_m, m))
            assert same_bits(np.ascontiguousarray(o[5, rest]), np.ascontiguousarray(c.base[5, rest]))
    if bc.ROT[kind]:                                                                                    # a zero-norm quaternion gives NaN
        bad = c.z.copy()
        bad[0, :4] = 0.0
        o, p, x2 = dev_between(eng, c, z=bad)
        assert np.isnan(p[0]) and np.isnan(x2[0]) and same_bits(o[1:], hess[1:])


def test_no_measurements_at_all(eng):
    """M = 0: the base comes back, or zeros; F = 0 is a no-op."""
    c = bc.case(2, 5).head(5)
    c.mfirst, c.counts, c.M = np.zeros(6, dtype=np.int64), np.zeros(5, dtype=np.int64), 0
    c.z, c.R, c.weight = np.zeros((0, 7)), np.zeros((0, 21)), np.zeros(0)
    hess, chi2, _ = dev_between(eng, c, chi2_m=False)
    assert same_bits(hess, c.base) and same_bits(chi2, c.chi2_base)
    hess, chi2, _ = dev_between(eng, c, base=False, chi2_m=False)
    assert (hess == 0.0).all() and (chi2 == 0.0).all()
    dev = eng.device
    out, x2 = eng.state_between(torch.zeros((1, 16), dtype=torch.float64, device=dev), "pose", _t(c.z, dev), _t(c.R, dev),
                                torch.zeros((1,), dtype=torch.int64, device=dev))
    assert out.shape == (0, 496) and x2.shape == (0,)
    # the C entries themselves at F = 0 with the engine's live context (the Engine returns before them): CPI_OK, nothing is written
    st, mf = torch.zeros((1, 16), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev)
    guard = torch.full((496,), GUARD, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert eng.lib.cpi_state_between_batch(eng.ctx, 0, 0, 2, p(mf), p(st), 1, None, None, None, None, None, None, None, p(guard), None, None) == 0
    torch.cuda.synchronize()
    assert (guard == GUARD).all()
    h_st, h_mf, h_guard = st.cpu(), mf.cpu(), guard.cpu()
    assert eng.lib.cpi_state_between_batch_host(eng.ctx, 0, 0, 2, p(h_mf), p(h_st), 1, None, None, None, None, None, None, None, p(h_guard), None,
                                                None) == 0
    assert (h_guard == GUARD).all()


# ------------------------------------------------------------------------------------------ 3. end to end
ITER, LAM0 = 12, 1e-3


@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


@pytest.fixture(scope="module", params=["ragged", "dense"])
def problem(eng, pipe, request):
    """One end-to-end case as a dict.  "ragged": eight chains of 2, 3, 4, 5, 6, 6, 3, 2 states (fx.RAGGED_COUNTS) with explicit first /
    count / ffirst and compacted factor rows; "dense": the eight chains of six.  A Gaussian prior on every chain's first state, centred
    on the unperturbed state, and the betweens of bc.e2e_betweens at the device's unperturbed states: a relative pose on every factor, a
    body-frame displacement on every second one."""
    return make_problem(eng, pipe, request.param == "ragged")


def make_problem(eng, pipe, ragged):
    """The dict of the fixture `problem` (tests/test_gpu_between_edges.py takes one layout at a time)."""
    C, G, dev = pipe.C, pipe.G, eng.device
    L = fx.layout(ragged)
    P0 = np.zeros((C, 16, 16))
    P0[:, np.arange(15), np.arange(15)] = 0.1 * cc.SCALES ** 2
    first = _t(L["first"], dev)
    betweens = bc.e2e_betweens(pipe.pred.cpu().numpy(), L)
    on_dev = [dict(kind=b["kind"], z=_t(b["z"], dev), R=_t(b["R"], dev), mfirst=_t(b["mfirst"], dev)) for b in betweens]
    own = np.repeat(np.arange(len(L["fi"])), np.diff(betweens[1]["mfirst"]))   # fix_offsets from the factor of every displacement: the same mfirst
    assert torch.equal(eng.fix_offsets(_t(own, dev), len(L["fi"])), on_dev[1]["mfirst"])
    keep = _t(L["keep"], dev)
    chain = dict(first=first, count=_t(L["count"], dev), ffirst=_t(L["ffirst"], dev)) if ragged else {}
    ii, jj = eng.chain_indices(C, G, chain.get("first"), chain.get("count"))
    assert np.array_equal(ii.cpu().numpy(), L["fi"]) and np.array_equal(jj.cpu().numpy(), L["fj"])
    return dict(layout=L, ragged=ragged, anchor=pipe.pred[first].contiguous(), prior0=_t(cc.pack_upper(P0), dev), idx=first.to(torch.int32),
                betweens=betweens, on_dev=on_dev, chain=chain, ii=ii.to(dev), jj=jj.to(dev), lin=pipe.lin[keep].contiguous(),
                Rt=pipe.Rt[keep].contiguous(), meas={n: v[keep].contiguous() for n, v in pipe.meas.items() if not n.startswith("_")})


def run_lm(eng, pipe, pb, betweens=True, iterations=ITER, buffers=None, states=None, init=True):
    st = pipe.states.clone() if states is None else states
    idx = {} if pb["ragged"] else dict(idx_i=pb["ii"], idx_j=pb["jj"])      # ragged: chain_lm forms the factor indices itself
    return eng.chain_lm(1, pb["meas"], pb["lin"], None, st, pb["Rt"], pipe.C, pipe.G, prior0=pb["prior0"], anchor=pb["anchor"], prior_idx=pb["idx"],
                        lam=LAM0, iterations=iterations, buffers=buffers, init=init, betweens=pb["on_dev"] if betweens else None, **idx, **pb["chain"])


@pytest.fixture(scope="module")
def eager(eng, pipe, problem):
    out = run_lm(eng, pipe, problem)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def test_chain_lm_with_betweens_converges_to_the_cpu_loops_states(eng, pipe, problem, eager):
    C, G, pb = pipe.C, pipe.G, problem
    member = pb["layout"]["member"]
    states, cost, lam, phase = (t.cpu().numpy() for t in eager)
    print("%s: cost %s\nlambda %s\nphase %s" % ("ragged" if pb["ragged"] else "dense", cost, lam, phase))
    assert (phase == lc.CONVERGED).all()
    assert np.array_equal(states[~member], pipe.states.cpu().numpy()[~member])                # a state of no chain is never moved
    anchor, prior0, start = pb["anchor"].cpu().numpy(), pb["prior0"].cpu().numpy(), pipe.states.cpu().numpy()
    loop = bc.BetweenLoop(anchor, prior0, pb["betweens"], pb["layout"])
    r_states, r_cost, r_lam, r_phase, r_hist = loop.run(start, LAM0, ITER)
    print("the CPU loop: cost %s\nphase %s" % (r_cost, r_phase))
    assert (r_phase == lc.CONVERGED).all()
    # sigma at the final states: the undamped system there with the prior and the betweens, factorised and inverted block by block
    st = eager[0]
    rows, _ = eng.prior_relinearize(st, pb["anchor"], pb["prior0"], idx=pb["idx"])
    ws = torch.empty((eng.chain_solve_workspace_doubles(C * G),), dtype=torch.float64, device=eng.device)
    status = torch.zeros((C,), dtype=torch.int32, device=eng.device)
    hess = eng.factor_hessian(1, pb["meas"], pb["lin"], None, st, pb["Rt"], pb["ii"], pb["jj"])
    for b in pb["on_dev"]:
        eng.state_between(st, b["kind"], b["z"], b["R"], b["mfirst"], pb["ii"], pb["jj"], hess_base=hess, out=hess, want_cost=False)
    eng.chain_solve(hess, C=C, G=G, prior=rows, status=status, workspace=ws, **pb["chain"])
    cov = torch.full((C * G, 120), float("nan"), dtype=torch.float64, device=eng.device)
    eng.chain_marginals(ws, C=C, G=G, status=status, out=cov, first=pb["chain"].get("first"), count=pb["chain"].get("count"))
    sigma = np.sqrt(cov.cpu().numpy()[member][:, [cc.tri(i) + i for i in range(15)]])
    worst = float(np.abs(lc.oracle_local(states[member], r_states[member]) / sigma).max())
    print("final states against the CPU loop: %.3g sigma (gate %.3g), cost difference %.3g" % (worst, bc.GATE_FINAL_DEVICE, np.abs(cost - r_cost).max()))
    assert status.cpu().tolist() == [0] * C and worst <= bc.GATE_FINAL_DEVICE
    # the betweens act: the same loop without them, evaluated on the same objective, ends higher -- on the device and on the CPU
    plain = run_lm(eng, pipe, pb, betweens=False)[0]
    torch.cuda.synchronize()
    obj_with, obj_plain = loop.objective(states), loop.objective(plain.cpu().numpy())
    without = bc.BetweenLoop(anchor, prior0, pb["betweens"], pb["layout"], evaluate=False)
    obj_cpu_plain = without.objective(without.run(start, LAM0, ITER)[0])
    print("the objective with the betweens %s\nwithout them (device) %s\nwithout them (CPU loop) %s" % (obj_with, obj_plain, obj_cpu_plain))
    assert np.abs(obj_with - cost).max() <= 1e-9 * np.abs(cost).max()
    assert (obj_with < obj_plain).all() and (obj_with < obj_cpu_plain).all()


def test_one_iteration_with_betweens_as_a_graph_replayed(eng, pipe, problem, eager):
    bufs = {}
    st = pipe.states.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_lm(eng, pipe, problem, iterations=1, buffers=bufs, states=st)                     # warm-up on a side stream; fills bufs
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_lm(eng, pipe, problem, iterations=1, buffers=bufs, states=st, init=False)
    st.copy_(pipe.states)                                                     # back to the start: states, lambda, phase, then cost and chi2 (init)
    bufs["lam"].fill_(LAM0)
    bufs["phase"].zero_()
    run_lm(eng, pipe, problem, iterations=0, buffers=bufs, states=st)
    for _ in range(ITER):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st, eager[0]) and torch.equal(bufs["cost"], eager[1]) and torch.equal(bufs["lam"], eager[2]) and torch.equal(bufs["phase"], eager[3])
    assert "fix_rows" not in bufs                                             # the betweens are in place: no buffer of their own


def test_chain_lm_without_betweens_is_what_it_was(eng, pipe, problem):
    """betweens=None and betweens=[] issue the launches of a call without the argument: the same bits."""
    idx = {} if problem["ragged"] else dict(idx_i=problem["ii"], idx_j=problem["jj"])
    runs = []
    for kw in ({}, dict(betweens=None), dict(betweens=[])):
        st = pipe.states.clone()
        out = eng.chain_lm(1, problem["meas"], problem["lin"], None, st, problem["Rt"], pipe.C, pipe.G, prior0=problem["prior0"], anchor=problem["anchor"],
                           prior_idx=problem["idx"], lam=LAM0, iterations=3, **kw, **idx, **problem["chain"])
        torch.cuda.synchronize()
        runs.append(tuple(t.clone() for t in out))
    assert all(torch.equal(a, b) for r in runs[1:] for a, b in zip(r, runs[0]))


# ------------------------------------------------------------------------------------------ 4. C++
def test_between_cpp_facade(eng):
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_between")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_between.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "test_between ok 7 6", p.stdout
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[-8:-1]])
    F, dev = 7, eng.device                                                    # the inputs of the program, through the module-level entries
    S = F + 1
    states = np.zeros((S, 16))
    states[np.arange(S), np.arange(S) % 3] = 0.6
    states[:, 3] = 0.8
    states[:, 4:] = 0.25 * ((np.arange(S)[:, None] * 7 + np.arange(4, 16)[None, :] * 3) % 11) - 1.0
    base = ((np.arange(F * 496) * 13) % 17 - 8.0).reshape(F, 496)
    counts = np.arange(F) % 3
    own = np.repeat(np.arange(F), counts)
    M = len(own)
    z = np.array([[0.0, 0.28, 0.0, 0.96, 0.5 * (m + 1), -0.25, 0.125 * m] for m in range(M)])
    R = np.array([[(2.0 + c) if r == c else 0.25 * ((r + c + m) % 3) for c in range(6) for r in range(c + 1)] for m in range(M)])
    w = 0.5 + 0.25 * np.arange(M)
    rows, chi2 = cpi_amd.state_between(_t(states, dev), "pose", _t(z, dev), _t(R, dev), cpi_amd.fix_offsets(_t(own, dev), F), weight=_t(w, dev),
                                       hess_base=_t(base, dev), chi2_base=_t(np.arange(1.0, F + 1), dev))
    torch.cuda.synchronize()
    mine = np.concatenate([chi2.cpu().numpy()[:, None], rows.cpu().numpy()[:, bc.touched(2)]], axis=1)
    assert same_bits(np.ascontiguousarray(mine), np.ascontiguousarray(got))
