"""GPU: the optimiser's trial step -- cpi_retract_batch, cpi_local_batch, cpi_factor_cost_[tri_]batch and their host forms.

Retract / local on the inputs of tests/trial_cases.py (|dtheta| from exact zero through both switches of sincos_fast to 2 pi, every
wavefront a mix; negated and float32-rounded quaternions; positions of 5e6) against oracle/cpi_oracle.c: quaternion entries within
tol.REG_FACTOR (local's rotation part: REG_FACTOR x max(1, |ref|)), the additive entries bit for bit the IEEE sums / differences.

Cost on factor_cases.mixed() with R = Engine.sqrt_information of the windows' covariance read back and used as given (the inputs and
the long-double reference of tests/test_gpu_factor_edges.py, computed once and shared): werr bit for bit the err of the whitened
sweep and within the whitened REG gates of profiles/factor_edges.md of the long-double reference; chi2 bit for bit the documented
summation of the device's own werr and within 32 g m^2 of the long-double sum; the total against math.fsum within the any-order
bound, the same bits on every run; states gathered through shuffled indices, and chained with idx = NULL at every size.  pytest -s prints the floors (profiles/trial_step.md records them)."""
import math

import numpy as np
import pytest
import torch

import cpi_amd
from tests import factor_cases as fc
from tests import test_gpu_factor_edges as fe
from tests import trial_cases as tc
from tests.tol import REG_FACTOR

pytestmark = pytest.mark.gpu

COST_SIZES = [1, 3, 4, 5, 15, 16, 17, 21, 22, 63, 64, 65, 257]
F_TWO_LEVEL = 32768 + 5                              # above it the total's reduction has a second level
WHITE_GATE = {1: 1.0e-12, 2: 2.1e-12}                # 100 x the whitened floors of profiles/factor_edges.md
assert WHITE_GATE == {m: fe.REG[m]["white"] for m in (1, 2)}


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _dev(a, eng):
    return torch.from_numpy(np.array(a, order="C")).to(eng.device)


# ------------------------------------------------------------------------------------------ retract / local
@pytest.mark.parametrize("S", tc.SIZES)
def test_retract_and_local_against_the_oracle(eng, S):
    states, delta, other, mag = (a[:S] for a in tc.states_and_steps())
    want_r, want_l, want_z = (a[:S] for a in tc.oracle_results())
    assert (tc.retract_margins(states, delta) >= tc.MARGIN_MIN).all() and (tc.local_margins(states, other) >= tc.MARGIN_MIN).all()
    x, d, o = _dev(states, eng), _dev(delta, eng), _dev(other, eng)
    pad = 2
    big = torch.full((S + pad, 16), -7.0, dtype=torch.float64, device=eng.device)
    bigl = torch.full((S + pad, 15), -7.0, dtype=torch.float64, device=eng.device)
    eng.retract(x, d, out=big[:S])
    eng.local_coordinates(x, o, out=bigl[:S])
    inplace = x.clone()
    assert eng.retract(inplace, d, out=inplace) is inplace
    zero = eng.retract(x, torch.zeros_like(d))
    torch.cuda.synchronize()
    got, gl = big[:S].cpu().numpy(), bigl[:S].cpu().numpy()
    e, el = tc.quat_dev(got, want_r), tc.local_rot_dev(gl, want_l)
    if S == tc.S_ALL:
        print("\nretract vs oracle, quaternion entries, per |dtheta|: %s" % ", ".join("%s: %.1e" % kv for kv in tc.per_mag(e, mag).items()))
    print("S %d: retract quaternion %.1e, local rotation part %.1e (gate %.0e)" % (S, e.max(), el.max(), REG_FACTOR))
    assert e.max() <= REG_FACTOR and el.max() <= REG_FACTOR
    assert np.array_equal(got[:, 4:], states[:, 4:] + delta[:, 3:])                 # bit for bit the IEEE sums
    assert np.array_equal(gl[:, 3:], other[:, 4:] - states[:, 4:])                  # ... and differences
    assert torch.equal(inplace, big[:S])                                            # in place == out of place
    assert torch.all(big[S:] == -7.0) and torch.all(bigl[S:] == -7.0)               # rows past S stay untouched
    z = zero.cpu().numpy()
    assert tc.quat_dev(z, want_z).max() <= REG_FACTOR and np.array_equal(z[:, 4:], states[:, 4:])
    if S >= 63:
        assert np.abs(z[:, :4] - states[:, :4]).max() > 1e-9                        # quat_multiply(identity, q), not a copy
    # the host forms give the device forms' bits
    hr = eng.retract_host(torch.from_numpy(states.copy()), torch.from_numpy(delta.copy()))
    hl = eng.local_coordinates_host(torch.from_numpy(states.copy()), torch.from_numpy(other.copy()))
    assert np.array_equal(hr.numpy(), got) and np.array_equal(hl.numpy(), gl)


def test_retract_refuses_a_partial_overlap_on_the_device(eng):
    buf = torch.zeros((10, 16), dtype=torch.float64, device=eng.device)
    d = torch.zeros((8, 15), dtype=torch.float64, device=eng.device)
    with pytest.raises(cpi_amd.CpiError, match="overlaps"):
        eng.retract(buf[:8], d, out=buf[1:9])
    with pytest.raises(AssertionError):
        eng.retract(buf[:8], d.float())


# ------------------------------------------------------------------------------------------ cost
def _cost_all(eng, x, pad=1, **kw):
    """Dense and packed R, with and without werr, each into buffers `pad` rows longer and pre-filled."""
    F = x.F
    a = (x.model, x.meas, x.lin, x.q, x.states)
    res = {}
    for name, R, want_err in (("dense", x.R, True), ("tri", x.Rt, True), ("tri_noerr", x.Rt, False)):
        ws = torch.full((eng.factor_cost_total_doubles(F) + pad,), -7.0, dtype=torch.float64, device=eng.device)
        out = {"chi2": torch.full((F + pad,), -7.0, dtype=torch.float64, device=eng.device), "workspace": ws}
        if want_err:
            out["werr"] = torch.full((F + pad, 15), -7.0, dtype=torch.float64, device=eng.device)
        head = {k: (v[:F] if k != "workspace" else v) for k, v in out.items()}
        eng.factor_cost(*a, R, x.ii, x.jj, want_err=want_err, out=head, **kw)
        res[name] = out
    return res


@pytest.mark.parametrize("F", COST_SIZES)
@pytest.mark.parametrize("model", [1, 2])
def test_cost_against_the_whitened_sweep_and_the_longdouble_reference(eng, model, F):
    x = fe.Inputs(eng, model, F)
    ref = fe._reference(eng, model)[1]["white"][0][x.rows]                          # R e, long double
    res = _cost_all(eng, x)
    white = eng.factor_eval(model, x.meas, x.lin, x.q, x.states, x.ii, x.jj, want_H=False, sqrt_info=x.Rt)["err"]
    contiguous = fe.Inputs(eng, model, F, gather=False)
    st = contiguous.states                                                          # xi rows, then xj rows
    flat = eng.factor_cost(model, contiguous.meas, contiguous.lin, contiguous.q, st, contiguous.Rt, contiguous.ii, contiguous.jj, want_err=True)
    torch.cuda.synchronize()
    werr, chi2 = res["tri"]["werr"][:F], res["tri"]["chi2"][:F]
    g = WHITE_GATE[model]
    # werr: the whitened sweep's err, bit for bit; the long-double reference within the REG gate
    assert torch.equal(werr, white)
    e = fc.rel_err(werr.cpu().numpy(), ref)
    # chi2: the documented summation of the device's own werr, bit for bit; the long-double sum within 32 g m^2
    w = werr.cpu().numpy()
    c = chi2.cpu().numpy()
    assert np.array_equal(c, tc.chi2_documented(w))
    refl = np.asarray(ref, dtype=np.longdouble)
    cref = np.asarray((refl * refl).sum(axis=1), dtype=np.float64)
    ec = np.abs(c - cref) / tc.chi2_gate(g, ref)
    print("model %d F %d: werr vs long double %.1e (gate %.1e), chi2 %.1e of its bound" % (model, F, e.max(), g, ec.max()))
    assert e.max() <= g and ec.max() <= 1.0
    # dense R == packed R; with and without werr; states gathered == contiguous; nothing written past F
    for k in ("werr", "chi2", "workspace"):
        assert torch.equal(res["dense"][k], res["tri"][k]), k
    for k in ("chi2", "workspace"):
        assert torch.equal(res["tri_noerr"][k], res["tri"][k]), k
    assert torch.equal(flat["chi2"], chi2) and torch.equal(flat["werr"], werr) and torch.equal(flat["total"], res["tri"]["workspace"][:1])
    for name, o in res.items():
        assert torch.all(o["chi2"][F:] == -7.0) and torch.all(o["workspace"][1:] == -7.0), name     # F <= 32768: one double of workspace
        assert "werr" not in o or torch.all(o["werr"][F:] == -7.0), name
    # the total
    total = float(res["tri"]["workspace"][0])
    exact = 0.5 * math.fsum(c.tolist())
    assert abs(total - exact) <= tc.total_bound(F, total), (total, exact)


@pytest.mark.parametrize("F", COST_SIZES)
@pytest.mark.parametrize("model", [1, 2])
def test_cost_with_chained_states_and_null_indices(eng, model, F):
    """idx_i = idx_j = NULL: factor f reads states f and f + 1 of an [F + 1, 16] array -- at every size (partial wavefronts, the
    f + 1 of a wavefront's last factor in the next wavefront's rows, the last f + 1 = S - 1), both layouts of R, bit for bit the
    call with ii = arange(F), jj = arange(F) + 1.  State 2 k is xi of factor 2 k and state 2 k + 1 its xj, so the even factors
    are the genuine pairs of mixed() (the odd ones pair unrelated states: large but finite residuals).  S = F is refused."""
    x = fe.Inputs(eng, model, F, gather=False)                                       # x.states: xi rows, then xj rows
    k = torch.arange(F + 1, device=eng.device)
    src = torch.where(k % 2 == 0, torch.clamp(k, max=F - 1), F + k - 1)               # even: xi_k (the last one: xi_{F-1}); odd: xj_{k-1}
    chain = x.states[src].contiguous()
    assert chain.shape == (F + 1, 16)
    ii = torch.arange(F, dtype=torch.int32, device=eng.device)
    a = (model, x.meas, x.lin, x.q, chain)
    for R in (x.Rt, x.R):
        null = eng.factor_cost(*a, R, want_err=True)
        explicit = eng.factor_cost(*a, R, ii, ii + 1, want_err=True)
        torch.cuda.synchronize()
        for key in ("chi2", "werr", "total"):
            assert torch.equal(null[key], explicit[key]), (key, R.shape[1])
        assert bool(torch.isfinite(null["chi2"]).all())
    genuine = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, x.Rt, x.ii, x.jj)
    torch.cuda.synchronize()
    even = torch.arange(0, F, 2, device=eng.device)
    assert torch.equal(null["chi2"][even], genuine["chi2"][even])
    with pytest.raises(cpi_amd.CpiError, match="F \\+ 1"):
        eng.factor_cost(model, x.meas, x.lin, x.q, chain[:F].contiguous(), x.Rt)


@pytest.mark.parametrize("model", [1, 2])
def test_a_permutation_of_the_factors_permutes_chi2(eng, model):
    F = 257
    a = _cost_all(eng, fe.Inputs(eng, model, F))
    perm = np.random.default_rng(78).permutation(F)
    b = _cost_all(eng, fe.Inputs(eng, model, F, gather=False, rows=perm))
    p = torch.from_numpy(perm).to(eng.device)
    for name in a:
        assert torch.equal(a[name]["chi2"][:F][p], b[name]["chi2"][:F]), name
    assert torch.equal(a["tri"]["werr"][:F][p], b["tri"]["werr"][:F])


@pytest.mark.parametrize("model", [1, 2])
def test_total_is_deterministic_and_has_a_second_level(eng, model):
    """F = 32768 + 5, mixed(257) tiled: every tile's chi2 is the first tile's, the total is within the any-order bound of fsum and two
    calls -- with and without werr -- give the same bits; nothing of the workspace past its size is written."""
    x = fe.Inputs(eng, model, 257)
    F = F_TWO_LEVEL
    t = torch.arange(F, device=eng.device) % 257
    meas = {k: v[t].contiguous() for k, v in x.meas.items()}
    lin, q = x.lin[t].contiguous(), (None if x.q is None else x.q[t].contiguous())
    ii, jj, Rt = x.ii[t].contiguous(), x.jj[t].contiguous(), x.Rt[t].contiguous()
    n = eng.factor_cost_total_doubles(F)
    assert n == 1 + (F + 4095) // 4096
    outs = []
    for want_err in (False, True, False):
        ws = torch.full((n + 3,), -7.0, dtype=torch.float64, device=eng.device)
        out = {"chi2": torch.full((F + 1,), -7.0, dtype=torch.float64, device=eng.device), "workspace": ws}
        if want_err:
            out["werr"] = torch.empty((F, 15), dtype=torch.float64, device=eng.device)
        eng.factor_cost(model, meas, lin, q, x.states, Rt, ii, jj, want_err=want_err, out={k: (v[:F] if k == "chi2" else v) for k, v in out.items()})
        outs.append(out)
    small = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, x.Rt, x.ii, x.jj)
    torch.cuda.synchronize()
    c = outs[0]["chi2"][:F]
    full = (F // 257) * 257
    assert bool((c[:full].view(-1, 257) == small["chi2"]).all()) and torch.equal(c[full:], small["chi2"][:F - full])
    for o in outs:
        assert torch.equal(o["chi2"], outs[0]["chi2"]) and torch.equal(o["workspace"], outs[0]["workspace"])
        assert torch.all(o["workspace"][n:] == -7.0) and float(o["chi2"][F]) == -7.0
    total = float(outs[0]["workspace"][0])
    exact = 0.5 * math.fsum(c.cpu().numpy().tolist())
    print("model %d F %d: total %.17g, |total - 0.5 fsum| = %.1e (bound %.1e)" % (model, F, total, abs(total - exact), tc.total_bound(F, total)))
    assert abs(total - exact) <= tc.total_bound(F, total)


@pytest.mark.parametrize("model", [1, 2])
def test_a_nan_factor_poisons_its_chi2_and_the_total_alone(eng, model):
    F = 65
    x = fe.Inputs(eng, model, F)
    clean = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, x.Rt, x.ii, x.jj)
    for tri in (True, False):
        R = (x.Rt if tri else x.R).clone()
        R[37] = float("nan")                                                        # what cpi_sqrt_information_* leaves of a non-positive pivot
        got = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, R, x.ii, x.jj, want_err=True)
        torch.cuda.synchronize()
        bad = torch.isnan(got["chi2"])
        assert bad.nonzero().flatten().tolist() == [37] and bool(torch.isnan(got["total"]).all())
        keep = ~bad
        assert torch.equal(got["chi2"][keep], clean["chi2"][keep]) and bool(torch.isfinite(got["werr"][keep]).all())


@pytest.mark.parametrize("model", [1, 2])
def test_the_call_captures_into_a_graph(eng, model):
    """retract -> factor_cost (with its total) captured once and replayed twice: the bits of the eager calls."""
    F = 257
    x = fe.Inputs(eng, model, F)
    delta = torch.zeros((2 * F, 15), dtype=torch.float64, device=eng.device)
    delta[:, 3:] = 1e-3
    delta[:, :3] = 1e-2
    eager_states = eng.retract(x.states, delta)
    eager = eng.factor_cost(model, x.meas, x.lin, x.q, eager_states, x.Rt, x.ii, x.jj, want_err=True)
    torch.cuda.synchronize()
    trial = torch.empty_like(x.states)
    out = {k: torch.zeros_like(v) for k, v in eager.items() if k != "total"}

    def call():
        eng.retract(x.states, delta, out=trial)
        eng.factor_cost(model, x.meas, x.lin, x.q, trial, x.Rt, x.ii, x.jj, want_err=True, out=out)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                  # warm-up on the side stream, as graph capture requires
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for v in out.values():
            v.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(trial, eager_states)
        for k in ("chi2", "werr", "total"):
            assert torch.equal(out[k], eager[k]), k


@pytest.mark.parametrize("model", [1, 2])
def test_host_cost_is_the_device_chain(eng, model):
    """cpi_factor_cost_batch_host = sqrt_information (packed) + factor_cost on the device, from P_sym and from the dense P."""
    F = 22
    b = fe._reference(eng, model)[0]
    bc = fc.base_cases(model)
    base = b["base"][:F]
    pre = eng.preintegrate(_dev(bc["knots"][base], eng), _dev(bc["lin"][base], eng), _dev(bc["q_k_lin"][base], eng), eng.make_params(model),
                           want=("cov", "cov_sym"))
    x = fe.Inputs(eng, model, F)
    Rt = eng.sqrt_information(pre["P_sym"])
    dev = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, Rt, x.ii, x.jj, want_err=True)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().contiguous()
    meas = {k: cpu(v) for k, v in x.meas.items()}
    for cov in ("P_sym", "P"):
        m = dict(meas)
        m[cov] = cpu(pre[cov])
        host = eng.factor_cost_host(model, m, cpu(x.lin), cpu(x.q), cpu(x.states), cpu(x.ii), cpu(x.jj), want_err=True)
        for k in ("chi2", "werr", "total"):
            assert torch.equal(host[k], dev[k].cpu()), (cov, k)
