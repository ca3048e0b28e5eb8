"""GPU: cpi_state_fix_batch against the references of tests/fix_cases.py at the smallest shapes that cross a wavefront of four states and
a lane group of sixteen (S in 1, 3, 4, 5, 9; 0, 1, 2 and 17 fixes per state), the host form and the C++ facade against the device form
bit for bit, the old route through prior_relinearize, chaining through base, and Engine.chain_lm(fixes=...) end to end on the chains of
tests/chain_pipeline.py cut to 2 .. 6 states (explicit first / count / ffirst) and whole: eager, without the fixes, and as one captured
graph.  The figures of a comparison are printed before anything is asserted; the gates are those of tests/fix_cases.py.

The position and velocity kinds are the host twin's bits; the rotation kinds are not (the quaternion product normalises with a
reciprocal square root on the device and a square root and a division on the host: tests/test_gpu_lm.py), so they are held to the
reference's gates alone."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import fix_cases as fx
from tests import lm_cases as lc
from tests import test_fix_cpu as tf
from tests.test_lm_cpu import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -7.0


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


@pytest.fixture(scope="module")
def hf():
    if (not os.path.exists(tf._LIB)) or os.path.getmtime(tf._LIB) < max(os.path.getmtime(p) for p in (tf._SRC, tf._MATH)):
        tf.tm._build(tf._SRC, tf._LIB)
    return tf._bind(tf._LIB)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _banded(n, cols, dev):
    """A NaN-filled output of n rows between two guard rows -> (the whole buffer, the view the entry gets)."""
    buf = torch.full((n + 2,) + cols, GUARD, dtype=torch.float64, device=dev)
    buf[1:n + 1] = float("nan")
    return buf, buf[1:n + 1]


def dev_fix(eng, c, weight=True, base=True, rows=True, cost=True, chi2=True, host=False, z=None, states=None, base_rows=None, base_pcost=None):
    """state_fix on case c -> (out [S, 136], pcost [S], chi2 [M]) as numpy (None where not asked for), outputs NaN-filled with guard bands."""
    dev = "cpu" if host else eng.device
    ob, ov = _banded(c.S, (136,), dev) if rows else (None, None)
    pb, pv = _banded(c.S, (), dev) if cost else (None, None)
    xb, xv = _banded(c.M, (), dev) if chi2 else (None, None)
    fn = eng.state_fix_host if host else eng.state_fix
    b_rows = (c.base if base_rows is None else base_rows) if base else None
    b_pc = (c.pcost_base if base_pcost is None else base_pcost) if base else None
    got = fn(_t(c.states if states is None else states, dev), fx.KINDS[c.kind] if c.S % 2 else c.kind, _t(c.z if z is None else z, dev), _t(c.R, dev),
             _t(c.mfirst, dev), weight=_t(c.weight, dev) if weight else None, base=_t(b_rows, dev), pcost_base=_t(b_pc, dev), out=ov, pcost=pv,
             chi2=xv, want_rows=rows, want_cost=cost)
    if not host:
        torch.cuda.synchronize()
    assert (got[0] is None) == (not rows) and (got[1] is None) == (not cost)
    for buf, n in ((ob, c.S), (pb, c.S), (xb, c.M)):
        assert buf is None or ((buf[0] == GUARD).all() and (buf[n + 1] == GUARD).all())
    return tuple(None if v is None else v.cpu().numpy() for v in (ov, pv, xv))


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_against_the_reference(eng, hf, kind):
    worst = {}
    for S in fx.SIZES:
        c = fx.case(kind, S)
        for weight, base in ((True, True), (False, False)):
            out, pcost, chi2 = dev_fix(eng, c, weight, base)
            assert not np.isnan(out).any() and not np.isnan(pcost).any() and not np.isnan(chi2).any(), S    # every state and every fix is written
            assert (out[:, 135] == 0.0).all()
            for k, v in fx.metrics(out, pcost, chi2, fx.reference(c, weight, base)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if kind < 2:                                                      # no quaternion in it: the twin's bits
                t_out, t_pc, t_chi2 = tf.twin(hf, c, weight, base)
                assert same_bits(out, t_out) and same_bits(pcost, t_pc) and same_bits(chi2, t_chi2), (S, weight, base)
    print("device, %s: %s (gates %s)" % (fx.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), fx.GATE_DEVICE))
    for k, v in worst.items():
        assert v <= fx.GATE_DEVICE[k], (k, v)


def test_no_fixes_at_all(eng):
    """M = 0: the base comes back (entry 135 as 0.0), or zeros."""
    c = fx.case(0, 5).head(5)
    c.mfirst, c.counts, c.M = np.zeros(6, dtype=np.int64), np.zeros(5, dtype=np.int64), 0
    c.z, c.R, c.weight = np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0)
    out, pcost, _ = dev_fix(eng, c, chi2=False)
    assert same_bits(out[:, :135], c.base[:, :135]) and (out[:, 135] == 0.0).all() and same_bits(pcost, c.pcost_base)
    out, pcost, _ = dev_fix(eng, c, base=False, chi2=False)
    assert (out == 0.0).all() and (pcost == 0.0).all()


# ------------------------------------------------------------------------------------------ 2. orientation branches
@pytest.mark.parametrize("kind", [2, 3], ids=fx.KINDS[2:])
def test_orientation_branches(eng, kind):
    c = fx.case(kind, 9)
    out, pcost, chi2 = dev_fix(eng, c)
    z = c.z.copy()
    z[:, :4] = -z[:, :4]                                                      # every fix on the other side of qd.w = 0
    o, p, x2 = dev_fix(eng, c, z=z)
    assert np.array_equal(o, out) and np.array_equal(p, pcost) and np.array_equal(x2, chi2)
    st = c.states.copy()
    st[:, :4] = -st[:, :4]                                                    # a negated state quaternion
    o, p, x2 = dev_fix(eng, c, states=st)
    assert np.array_equal(o, out) and np.array_equal(p, pcost) and np.array_equal(x2, chi2)
    for angle in (1e-9, 1.0, 3.1):                                            # every fix at one residual rotation
        ca = fx.Case(kind, fx.COUNTS[:5], seed=5, angle=angle)
        m = fx.metrics(*dev_fix(eng, ca), fx.reference(ca))
        print("%s, residual rotation %g rad: %s" % (fx.KINDS[kind], angle, ", ".join("%s %.3g" % kv for kv in sorted(m.items()))))
        for k, v in m.items():
            assert v <= fx.GATE_DEVICE[k], (angle, k, v)


# ------------------------------------------------------------------------------------------ 3. exact properties
@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_exact_properties(eng, kind):
    c = fx.case(kind, 9)
    out, pcost, chi2 = dev_fix(eng, c)
    none = c.counts == 0
    assert none.sum() == 3 and same_bits(out[none, :135], c.base[none, :135]) and same_bits(pcost[none], c.pcost_base[none])
    z_out, z_pc, _ = dev_fix(eng, c, base=False)
    assert (z_out[none] == 0.0).all() and (z_pc[none] == 0.0).all()
    w0 = c.head(9)                                                            # weight 0: the base as numbers, chi2 still the unweighted value
    w0.weight = np.zeros(c.M)
    o0, p0, c0 = dev_fix(eng, w0)
    assert np.array_equal(o0[:, :135], c.base[:, :135]) and np.array_equal(p0, c.pcost_base) and same_bits(c0, chi2)
    for S in (1, 3, 4, 5):                                                    # a state's bits: not S
        o, p, x2 = dev_fix(eng, fx.case(kind, S))
        assert same_bits(o, out[:S]) and same_bits(p, pcost[:S]) and same_bits(x2, chi2[:len(x2)]), S
    mv = fx.Case.head(c, 9)                                                   # ... nor where it sits: the states in reverse order
    order = np.arange(8, -1, -1)
    fixes = np.concatenate([np.arange(c.mfirst[s], c.mfirst[s + 1]) for s in order]).astype(np.int64)
    mv.counts = c.counts[order]
    mv.mfirst = fx.offsets(mv.counts)
    mv.states, mv.base, mv.pcost_base = c.states[order], c.base[order], c.pcost_base[order]
    mv.z, mv.R, mv.weight = c.z[fixes], c.R[fixes], c.weight[fixes]
    o, p, x2 = dev_fix(eng, mv)
    assert same_bits(o, np.ascontiguousarray(out[order])) and same_bits(p, np.ascontiguousarray(pcost[order])) and same_bits(x2, np.ascontiguousarray(chi2[fixes]))
    h_out, h_pc, h_chi2 = dev_fix(eng, c, host=True)                          # the _host form: the device form's bits
    assert same_bits(h_out, out) and same_bits(h_pc, pcost) and same_bits(h_chi2, chi2)
    n_out, pc_only, chi_only = dev_fix(eng, c, rows=False)                    # without rows: the same pcost bits
    assert n_out is None and same_bits(pc_only, pcost) and same_bits(chi_only, chi2)
    r_only, n_pc, _ = dev_fix(eng, c, cost=False, chi2=False)
    assert n_pc is None and same_bits(r_only, out)
    with pytest.raises(cpi_amd.CpiError, match="the fixes of state 2 "):
        bad = c.head(9)
        bad.mfirst = c.mfirst.copy()
        bad.mfirst[3] = bad.mfirst[2] - 1
        dev_fix(eng, bad, host=True)


# ------------------------------------------------------------------------------------------ 4. the old route
@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_one_fix_is_the_gaussian_record_of_prior_relinearize(eng, kind):
    """One fix on a state, weight 1, no base = prior_relinearize of the record Lam = S^T R^T R S, eta0 = 0, anchored at the state with z put
    in.  Lam: R^T R formed here in float64 against the entry's fma chains; eta and pcost: two summation orders of the same terms.  Both
    inside the device gates in the units of the reference."""
    c = fx.case(kind, 9)
    ms = [int(c.mfirst[s]) for s in range(c.S) if c.counts[s] == 1] + [int(c.mfirst[0]) + 4, int(c.mfirst[5]) + 3]
    one = fx.Case.head(c, 9)
    one.S, one.M = len(ms), len(ms)
    recs = [fx.gaussian_record(c, m) for m in ms]
    one.states = np.stack([c.states[s] for s, _, _ in recs])
    one.z, one.R, one.weight = c.z[ms], c.R[ms], np.ones(len(ms))
    one.counts, one.mfirst = np.ones(len(ms), dtype=np.int64), np.arange(len(ms) + 1, dtype=np.int64)
    one.base, one.pcost_base = np.zeros((one.S, 136)), np.zeros(one.S)
    out, pcost, _ = dev_fix(eng, one, weight=False, base=False)
    dev = eng.device
    prior, pc = eng.prior_relinearize(_t(one.states, dev), _t(np.stack([a for _, a, _ in recs]), dev), _t(np.stack([p for _, _, p in recs]), dev))
    torch.cuda.synchronize()
    m = fx.metrics(prior.cpu().numpy(), pc.cpu().numpy(), None, dict(fx.reference(one, False, False), out=out.astype(fx.LD), pcost=pcost.astype(fx.LD)))
    print("%s: the old route against the new one: %s (gates %s)" % (fx.KINDS[kind], m, fx.GATE_DEVICE))
    assert m["Lam"] <= fx.GATE_DEVICE["Lam"] and m["eta"] <= fx.GATE_DEVICE["eta"] and m["pcost"] <= fx.GATE_DEVICE["pcost"]


# ------------------------------------------------------------------------------------------ 5. chaining
def test_three_sensors_chained_on_a_relinearised_prior(eng):
    """prior_relinearize -> position -> velocity -> orientation through base / pcost_base, against the reference of the sum."""
    S, dev = 9, eng.device
    cs = [fx.case(k, S) for k in (0, 1, 2)]
    states, anchor, prior0 = (a[:S].copy() for a in lc.prior_case(12))
    prior0[:, 135] = 0.0
    prior, pc = eng.prior_relinearize(_t(states, dev), _t(anchor, dev), _t(prior0, dev))
    torch.cuda.synchronize()
    rows, pcost = prior.cpu().numpy(), pc.cpu().numpy()
    ref_out, ref_pc = rows.astype(fx.LD), pcost.astype(fx.LD)
    u_out, u_pc = np.abs(ref_out), np.abs(ref_pc)
    for c in cs:
        k = c.head(S)
        k.states, k.base, k.pcost_base = states, np.zeros((S, 136)), np.zeros(S)
        if c.kind == 2:                                                       # keep the residual rotations of the case on the new states
            own = c.owner()
            k.z = np.stack([lc._quat_mul(lc._quat_mul(c.z[m, :4], c.states[own[m], :4] * [-1, -1, -1, 1]), states[own[m], :4]) for m in range(c.M)])
        r = fx.reference(k)
        ref_out, ref_pc, u_out, u_pc = ref_out + r["out"], ref_pc + r["pcost"], u_out + r["u_out"], u_pc + r["u_pcost"]
        rows, pcost, _ = dev_fix(eng, k, base_rows=rows, base_pcost=pcost)
    m = fx.metrics(rows, pcost, None, dict(out=ref_out, pcost=ref_pc, u_out=u_out, u_pcost=u_pc))
    print("prior + position + velocity + orientation: %s (gates %s)" % (m, fx.GATE_DEVICE))
    assert m["Lam"] <= fx.GATE_DEVICE["Lam"] and m["eta"] <= fx.GATE_DEVICE["eta"] and m["pcost"] <= fx.GATE_DEVICE["pcost"]


# ------------------------------------------------------------------------------------------ 6. failure stays local
def test_a_nan_measurement_stays_in_its_state_and_its_chain(eng):
    c = fx.case(3, 9)
    out, pcost, chi2 = dev_fix(eng, c)
    for bad_z in (np.nan, 0.0):                                               # NaN, and a zero-norm quaternion
        z = c.z.copy()
        m = int(c.mfirst[5]) + 3
        z[m, :4] = bad_z
        o, p, x2 = dev_fix(eng, c, z=z)
        keep = np.arange(c.S) != 5
        assert same_bits(o[keep], out[keep]) and same_bits(p[keep], pcost[keep]) and same_bits(np.delete(x2, m), np.delete(chi2, m))
        assert np.isnan(p[5]) and np.isnan(o[5]).any() and np.isnan(x2[m])
    dev = eng.device                                                          # three chains of three states: chain 1 holds state 5
    chi2f = torch.ones(6, dtype=torch.float64, device=dev)
    good = eng.chain_cost(chi2f, _t(pcost, dev), C=3, G=3)
    got = eng.chain_cost(chi2f, _t(p, dev), C=3, G=3)
    torch.cuda.synchronize()
    assert torch.isnan(got[1]) and torch.equal(got[[0, 2]], good[[0, 2]]) and not torch.isnan(good).any()


# ------------------------------------------------------------------------------------------ 7. end to end
ITER, LAM0 = 12, 1e-3


@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


@pytest.fixture(scope="module", params=["ragged", "dense"])
def problem(eng, pipe, request):
    """One end-to-end case as a dict.  "ragged" is the issue's: eight chains of 2, 3, 4, 5, 6, 6, 3, 2 states (fx.RAGGED_COUNTS), chain c
    the first states of its block of six, so first / count / ffirst are explicit and differ from chain to chain, the factor rows are
    compacted, and 17 of the 48 states belong to no chain and hold no fix.  "dense": the eight chains of six.  A Gaussian prior on every
    chain's first state, centred on the unperturbed state, and the fixes of fx.e2e_fixes at the device's unperturbed states."""
    C, G, dev = pipe.C, pipe.G, eng.device
    ragged = request.param == "ragged"
    L = fx.layout(ragged)
    P0 = np.zeros((C, 16, 16))
    P0[:, np.arange(15), np.arange(15)] = 0.1 * cc.SCALES ** 2
    first = _t(L["first"], dev)
    fixes = fx.e2e_fixes(pipe.pred.cpu().numpy(), L["member"])
    on_dev = [dict(kind=f["kind"], z=_t(f["z"], dev), R=_t(f["R"], dev), mfirst=_t(f["mfirst"], dev)) for f in fixes]
    own = np.repeat(np.arange(C * G), np.diff(fixes[1]["mfirst"]))           # fix_offsets from the state of every pose fix: the same mfirst
    assert torch.equal(eng.fix_offsets(_t(own, dev), C * G), on_dev[1]["mfirst"])
    keep = _t(L["keep"], dev)
    chain = dict(first=first, count=_t(L["count"], dev), ffirst=_t(L["ffirst"], dev)) if ragged else {}
    ii, jj = eng.chain_indices(C, G, chain.get("first"), chain.get("count"))
    assert np.array_equal(ii.cpu().numpy(), L["fi"]) and np.array_equal(jj.cpu().numpy(), L["fj"])
    return dict(layout=L, ragged=ragged, anchor=pipe.pred[first].contiguous(), prior0=_t(cc.pack_upper(P0), dev), idx=first.to(torch.int32),
                fixes=fixes, on_dev=on_dev, chain=chain, ii=ii.to(dev), jj=jj.to(dev), lin=pipe.lin[keep].contiguous(), Rt=pipe.Rt[keep].contiguous(),
                meas={n: v[keep].contiguous() for n, v in pipe.meas.items() if not n.startswith("_")})


def run_lm(eng, pipe, pb, fixes=True, iterations=ITER, buffers=None, states=None, init=True):
    st = pipe.states.clone() if states is None else states
    idx = {} if pb["ragged"] else dict(idx_i=pb["ii"], idx_j=pb["jj"])      # ragged: chain_lm forms the factor indices itself
    return eng.chain_lm(1, pb["meas"], pb["lin"], None, st, pb["Rt"], pipe.C, pipe.G, prior0=pb["prior0"], anchor=pb["anchor"], prior_idx=pb["idx"],
                        lam=LAM0, iterations=iterations, buffers=buffers, init=init, fixes=pb["on_dev"] if fixes else None, **idx, **pb["chain"])


@pytest.fixture(scope="module")
def eager(eng, pipe, problem):
    out = run_lm(eng, pipe, problem)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def test_chain_lm_with_fixes_converges_to_the_cpu_loops_states(eng, pipe, problem, eager):
    C, G, pb = pipe.C, pipe.G, problem
    member = pb["layout"]["member"]
    states, cost, lam, phase = (t.cpu().numpy() for t in eager)
    print("%s: cost %s\nlambda %s\nphase %s" % ("ragged" if pb["ragged"] else "dense", cost, lam, phase))
    assert (phase == lc.CONVERGED).all()
    assert np.array_equal(states[~member], pipe.states.cpu().numpy()[~member])                # a state of no chain is never moved
    loop = fx.FixLoop(pb["anchor"].cpu().numpy(), pb["prior0"].cpu().numpy(), pb["fixes"], pb["layout"])
    r_states, r_cost, r_lam, r_phase, r_hist = loop.run(pipe.states.cpu().numpy(), LAM0, ITER)
    print("the CPU loop: cost %s\nphase %s" % (r_cost, r_phase))
    assert (r_phase == lc.CONVERGED).all()
    # sigma at the final states: the undamped system there with the prior and the fixes, factorised and inverted block by block
    st = eager[0]
    rows, _ = eng.prior_relinearize(st, pb["anchor"], pb["prior0"], idx=pb["idx"])
    for f in pb["on_dev"]:
        rows, _ = eng.state_fix(st, f["kind"], f["z"], f["R"], f["mfirst"], base=rows, want_cost=False)
    ws = torch.empty((eng.chain_solve_workspace_doubles(C * G),), dtype=torch.float64, device=eng.device)
    status = torch.zeros((C,), dtype=torch.int32, device=eng.device)
    hess = eng.factor_hessian(1, pb["meas"], pb["lin"], None, st, pb["Rt"], pb["ii"], pb["jj"])
    eng.chain_solve(hess, C=C, G=G, prior=rows, status=status, workspace=ws, **pb["chain"])
    cov = torch.full((C * G, 120), float("nan"), dtype=torch.float64, device=eng.device)
    eng.chain_marginals(ws, C=C, G=G, status=status, out=cov, first=pb["chain"].get("first"), count=pb["chain"].get("count"))
    sigma = np.sqrt(cov.cpu().numpy()[member][:, [cc.tri(i) + i for i in range(15)]])
    worst = float(np.abs(lc.oracle_local(states[member], r_states[member]) / sigma).max())
    print("final states against the CPU loop: %.3g sigma (gate %.3g), cost difference %.3g" % (worst, fx.GATE_FINAL_DEVICE, np.abs(cost - r_cost).max()))
    assert status.cpu().tolist() == [0] * C and worst <= fx.GATE_FINAL_DEVICE
    # the fixes act: the same call without them ends elsewhere, by more than one standard deviation of the estimate with them
    plain = run_lm(eng, pipe, pb, fixes=False)[0]
    torch.cuda.synchronize()
    away = float(np.abs(lc.oracle_local(plain.cpu().numpy()[member], r_states[member]) / sigma).max())
    print("without the fixes: %.3g sigma away" % away)
    assert away > 1.0


def test_one_iteration_with_fixes_as_a_graph_replayed(eng, pipe, problem, eager):
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


def test_buffers_of_a_run_without_fixes_serve_a_run_with_them(eng, pipe, problem, eager):
    """A buffers dict filled by a call without fixes gets the two buffer pairs added when fixes arrive: the eager run's bits."""
    bufs = {}
    run_lm(eng, pipe, problem, fixes=False, iterations=0, buffers=bufs)
    assert "fix_rows" not in bufs
    bufs["lam"].fill_(LAM0)
    bufs["phase"].zero_()
    out = run_lm(eng, pipe, problem, buffers=bufs)
    torch.cuda.synchronize()
    assert len(bufs["fix_rows"]) == 2 and len(bufs["fix_pcost"]) == 2 and all(torch.equal(a, b) for a, b in zip(out, eager))


# ------------------------------------------------------------------------------------------ 8. C++
def test_fix_cpp_facade(eng):
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_fix")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_fix.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "test_fix ok 7 6", p.stdout
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[-8:-1]])
    S, dev = 7, eng.device                                                    # the states of the program, through the module-level entries
    states = np.zeros((S, 16))
    states[:, 3] = 1.0
    states[:, 4:] = np.arange(S)[:, None] + np.arange(4, 16)[None, :]
    counts = np.arange(S) % 3
    own = np.repeat(np.arange(S), counts)
    z = states[own, 13:16] + 0.25 * (np.arange(len(own))[:, None] + 1)
    R = np.tile([1.0, 0, 2.0, 0, 0, 3.0], (len(own), 1))
    rows, pcost = cpi_amd.state_fix(_t(states, dev), "position", _t(z, dev), _t(R, dev), cpi_amd.fix_offsets(_t(own, dev), S))
    rows, pcost = cpi_amd.state_fix(_t(states, dev), "velocity", _t(states[:, 7:10] - 0.5, dev), _t(np.tile([2.0, 0, 2.0, 0, 0, 2.0], (S, 1)), dev),
                                    _t(np.arange(S + 1, dtype=np.int64), dev), base=rows, pcost_base=pcost)
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    mine = np.concatenate([np.stack([r[:, fx.slot(6 + i, 6 + i)], r[:, fx.slot(6 + i, 15)], r[:, fx.slot(12 + i, 12 + i)], r[:, fx.slot(12 + i, 15)]], axis=1)
                           for i in range(3)] + [pcost.cpu().numpy()[:, None]], axis=1)
    assert same_bits(np.ascontiguousarray(mine), np.ascontiguousarray(got))
