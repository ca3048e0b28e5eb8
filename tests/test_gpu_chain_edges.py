"""GPU: cpi_chain_solve_batch and cpi_chain_marginals_batch at the edges of their contract (include/cpi_amd.h), on the cases of
tests/chain_cases.py whose expectations tests/test_chain_cpu.py and tests/test_marginals_cpu.py settle on the host twins first:
the refusal boundary of ffirst, ffirst NULL beside an explicit first, the clamps of first / count / G / S, status = s + 1 wherever
the failing pivot sits in the wavefront, NaN in the inputs, a block that is exactly zero, a wavefront of empty chains, a chain of
64 states beside chains of 1, 0 and 2, inputs scaled by 2^+-300, diagonal damping with and without a prior.
Every call is chain_solve followed by chain_marginals on the same workspace, the workspace, cov and cross pre-filled with NaN and
delta with the sentinel.  Contract cases assert exact status, NaN in exactly the rows stated, the bits of the clean or clamped call
elsewhere (tests/chain_edge_checks.py); reference cases print their metrics and assert the gates of tests/chain_cases.py and
tests/marginals_cases.py as they are.  The host forms give the device forms' status and bits where their validation accepts the
call, and name the chain where it does not."""
import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import chain_edge_checks as ck
from tests import marginals_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_run(eng, host=False):
    """run(call, status_in) of tests/chain_edge_checks.py: chain_solve, then chain_marginals on its workspace (host=True: the two host
    forms; chain_marginals_host inverts the undamped system, so a damped call gives the solve alone).  A call with S below the
    batch's passes the leading S rows of out, prior, cov and cross."""
    dev = "cpu" if host else eng.device

    def run(call, status_in=None):
        b, S = call.b, call.S
        kw = dict(C=call.C, G=call.G, first=_t(call.first, dev), count=_t(call.count, dev))
        ffirst = _t(call.ffirst, dev)
        hess, prior = _t(b.hess, dev), (_t(b.prior[:S], dev) if call.with_prior else None)
        delta = torch.full((b.S, 15), ck.SENTINEL, dtype=torch.float64, device=dev)
        cov = torch.full((b.S, 120), float("nan"), dtype=torch.float64, device=dev)
        cross = torch.full((b.S, 225), float("nan"), dtype=torch.float64, device=dev)
        status = torch.full((call.C,), 99, dtype=torch.int32, device=dev)
        damping = "diagonal" if call.diagonal else "identity"
        with_cov = True
        if host:
            assert status_in is None
            eng.chain_solve_host(hess, ffirst=ffirst, prior=prior, lam=_t(call.lam, dev), damping=damping, out=delta[:S], status=status, **kw)
            with_cov = call.lam is None
            if with_cov:
                again = torch.full((call.C,), 99, dtype=torch.int32)
                eng.chain_marginals_host(hess, ffirst=ffirst, prior=prior, cross=cross[:S], out=cov[:S], status=again, **kw)
                assert torch.equal(again, status)
        else:
            ws = torch.full((eng.chain_solve_workspace_doubles(S),), float("nan"), dtype=torch.float64, device=dev)
            eng.chain_solve(hess, ffirst=ffirst, prior=prior, lam=_t(call.lam, dev), damping=damping, out=delta[:S], status=status, workspace=ws, **kw)
            eng.chain_marginals(ws, status=status if status_in is None else _t(np.asarray(status_in, dtype=np.int32), dev), out=cov[:S], cross=cross[:S], **kw)
            torch.cuda.synchronize()
        if not with_cov:
            return ck.Result(delta.numpy(), status.numpy())
        return ck.Result(delta.cpu().numpy(), status.cpu().numpy(), cov.cpu().numpy(), cross.cpu().numpy(), fill=np.nan)
    return run


def solve_line(name, ref, r):
    a, bb = ref.metrics(r.delta)
    print("%s: cond max %.1e, (a) %.3e (gate %.2e), (b) %.3e (gate %.2e)" % (name, ref.cond.max(), a, cc.GATE_BACKWARD_DEVICE, bb, cc.GATE_FORWARD_DEVICE))
    return a, bb


# ------------------------------------------------------------------------------------------ 1. the contract
def test_status_names_the_state_of_the_first_failure(eng):
    """All four chains of wavefront 0 fail at different states (the ballot slice of each and "the first failure wins"), the chain in
    lanes 48 .. 63 among them; pivots 0, 7 and 14; state 0 and the last state."""
    r = ck.check_failure_plan(device_run(eng))
    ck.equal(ck.check_failure_plan(device_run(eng, host=True)), r)


def test_nan_in_the_inputs(eng):
    r = ck.check_nan_plan(device_run(eng))
    ck.equal(ck.check_nan_plan(device_run(eng, host=True)), r)


def test_refusal_boundary_of_ffirst(eng):
    ck.check_ffirst_boundaries(device_run(eng))
    base, cases = cc.ffirst_boundary_cases()
    call = [k for c, ff, k, _ in cases if (c, ff) == (0, 15)][0]
    with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain 0 leave"):      # the host form refuses the whole call instead
        device_run(eng, host=True)(call)


def test_ffirst_null_with_an_explicit_first(eng):
    ck.check_ffirst_null(device_run(eng))


def test_clamps_of_first_count_G_and_S(eng):
    ck.check_clamps(device_run(eng))
    raw = [r for name, r, _ in cc.clamp_cases() if name == "first beyond S"][0]
    with pytest.raises(cpi_amd.CpiError, match="the states of chain 9 leave"):           # the host form validates, it does not clamp
        device_run(eng, host=True)(raw)


def test_a_wavefront_of_empty_chains(eng):
    r = ck.check_empty_wave(device_run(eng), cc.GATE_BACKWARD_DEVICE, cc.GATE_FORWARD_DEVICE)
    ck.equal(ck.check_empty_wave(device_run(eng, host=True), cc.GATE_BACKWARD_DEVICE, cc.GATE_FORWARD_DEVICE), r)


def test_a_zero_block_is_a_failed_pivot(eng):
    dev = ck.check_zero_pivot(device_run(eng))
    host = ck.check_zero_pivot(device_run(eng, host=True))                    # damped calls: the host solve alone
    for d, h in zip(dev, host):
        assert np.array_equal(d.status, h.status) and np.array_equal(d.delta, h.delta, equal_nan=True)
    row = cc.zero_pivot_case(False)[0].rows(1).start
    # (0 + 2 I)^-1: the reciprocal square root (within 2 ulp), squared: below 8 x 2^-53
    assert np.abs(mc.unpack_cov(dev[0].cov[row]) - 0.5 * np.eye(15)).max() <= 8 * cc.EPS_HALF


def test_a_status_of_the_callers_poisons_exactly_its_chain(eng):
    ck.check_status_overlay(device_run(eng))


# ------------------------------------------------------------------------------------------ 2. against the references
def test_long_chain_beside_short_ones(eng):
    """64 states beside 1, 0 and 2: the back pass carries dn, and the marginals P, through 62 idle trips of the short chains."""
    b, ref = cc.long_case()
    _, mref = mc.long_case()
    call = cc.Call(b, count=b.count)
    run = device_run(eng)
    r = run(call)
    a, bb = solve_line("LONG %s" % cc.LONG, ref, r)
    m = mref.metric(r.cov, r.cross)
    print("LONG: marginals metric %.3e (gate %.2e)" % (m, mc.GATE_DEVICE))
    assert r.status.tolist() == [0] * 4
    assert a <= cc.GATE_BACKWARD_DEVICE and bb <= cc.GATE_FORWARD_DEVICE and m <= mc.GATE_DEVICE
    ck.unowned(r, call)
    own, _ = call.owned()
    assert np.isfinite(np.linalg.cholesky(mc.unpack_cov(r.cov[own]))).all()
    for c in range(b.C):                                                      # every chain alone: its bits in the batch
        one = cc.Call.explicit(b, chains=[c])
        alone = run(one)
        assert alone.status.tolist() == [0]
        ck.same(alone, one, 0, r, call, gc=c)
        ck.unowned(alone, one)
    ck.equal(device_run(eng, host=True)(call), r)


@pytest.mark.parametrize("e", cc.SCALED_EXPONENTS)
def test_scaled_by_a_power_of_two(eng, e):
    """pivot_rsqrt away from magnitudes near 1e8: hess and prior times 2^e.  delta is that of the unscaled system and the covariance
    2^-e times its own, exactly, so the unscaled references serve (2^301: an odd exponent under the square root; its covariances,
    which the twin was not run on, are not compared)."""
    _, ref = cc.scaled_reference()
    _, mref = mc.scaled_reference()
    b = cc.scaled_batch(e)
    r = device_run(eng)(cc.Call(b, count=b.count))
    a, bb = solve_line("hess, prior x 2^%d" % e, ref, r)
    assert (r.status == 0).all() and a <= cc.GATE_BACKWARD_DEVICE and bb <= cc.GATE_FORWARD_DEVICE
    if e in (300, -300):
        m = mref.metric(r.cov * 2.0 ** e, r.cross * 2.0 ** e)
        print("hess, prior x 2^%d: marginals metric %.3e (gate %.2e)" % (e, m, mc.GATE_DEVICE))
        assert m <= mc.GATE_DEVICE


def test_diagonal_damping_without_a_prior(eng):
    b, lam, ref = cc.no_prior_diagonal_case()
    call = cc.Call(b, count=b.count, lam=lam, diagonal=True, with_prior=False)
    r = device_run(eng)(call)
    a, bb = solve_line("no prior, diagonal damping 0.25", ref, r)
    assert (r.status == 0).all() and a <= cc.GATE_BACKWARD_DEVICE and bb <= cc.GATE_FORWARD_DEVICE
    ck.unowned(r, call)


def test_marginals_with_diagonal_damping_invert_the_damped_matrix(eng):
    b, lam, ref = mc.diagonal_case()
    call = cc.Call(b, count=b.count, lam=lam, diagonal=True)
    r = device_run(eng)(call)
    m = ref.metric(r.cov, r.cross)
    print("diagonal damping 0.25: cond max %.1e, marginals metric %.3e (gate %.2e)" % (ref.cond.max(), m, mc.GATE_DEVICE))
    assert (r.status == 0).all() and m <= mc.GATE_DEVICE
    ck.unowned(r, call)
