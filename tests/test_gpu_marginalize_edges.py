"""GPU: cpi_chain_marginalize_batch at the edges of its contract (include/cpi_amd.h), on the cases of tests/marginalize_cases.py whose
expectations tests/test_marginalize_cpu.py settles on the host twin first (tests/marginalize_edge_checks.py states them once):
chains that are frozen while a wavefront mate fails or while their own Pr_m would fail every pivot, NaN in what state m receives at
status 0, the status across marginalize and the reduced chain's solve, a block that is exactly zero, the refusal boundary of ffirst
for every m, ffirst / count NULL beside an explicit first, the clamps of first / count / G / S with m judged against the clamped
count, status == NULL, call sizes around a wavefront, inputs scaled by powers of two.
Contract cases assert exact status, NaN in exactly the entries stated and the bits of another call elsewhere; the reference-gated
cases (64 states beside 1, 0 and 2; the scaled chains) print their metrics and assert the gates of tests/marginalize_cases.py as
they are.  The host form gives the device form's status and bits where its validation accepts the call, and names the chain where
it does not.  The largest call has 64 states."""
import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import marginalize_cases as mz
from tests import marginalize_edge_checks as mk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_run(eng, host=False):
    """run(b, drop, **kw) of tests/marginalize_edge_checks.py: chain_marginalize (host=True: chain_marginalize_host on CPU tensors).
    out is the leading C rows of a tensor of C + 1 rows and status the leading C elements of one of C + 1, so that what follows them
    is the test's; S below the batch's passes the leading S rows of prior."""
    dev = "cpu" if host else eng.device
    fn = eng.chain_marginalize_host if host else eng.chain_marginalize

    def run(b, drop, with_prior=True, hess=None, prior=None, G=None, S=None, status_in=None, no_status=False, **kw):
        own = {"first": (b.first, np.int64), "count": (b.count, np.int32), "ffirst": (b.ffirst, np.int64)}
        assert set(kw) <= set(own), kw
        arr = {k: None if kw.get(k, v) is None else np.ascontiguousarray(kw.get(k, v), dtype=dt) for k, (v, dt) in own.items()}
        Cn = next((len(v) for v in arr.values() if v is not None), b.C)
        pr = None
        if with_prior:
            pr = _t((b.prior if prior is None else prior)[:b.S if S is None else S], dev)
        buf = torch.full((Cn + 1, 136), mk.SENTINEL, dtype=torch.float64, device=dev)
        sbuf = torch.full((Cn + 1,), 99, dtype=torch.int32, device=dev)
        if status_in is not None:
            sbuf[:Cn] = _t(np.asarray(status_in, dtype=np.int32), dev)
        before = sbuf.clone()
        d = int(drop) if np.isscalar(drop) else _t(np.asarray(drop, dtype=np.int32), dev)
        out = fn(_t(b.hess if hess is None else hess, dev), C=Cn, G=b.G if G is None else G, prior=pr, drop=d, out=buf[:Cn],
                 status=None if no_status else sbuf[:Cn], **{k: _t(v, dev) for k, v in arr.items()})
        if not host:
            torch.cuda.synchronize()
        assert out.data_ptr() == buf.data_ptr() and (buf[Cn] == mk.SENTINEL).all() and int(sbuf[Cn]) == 99
        if no_status:
            assert torch.equal(sbuf, before)
        return buf[:Cn].cpu().numpy(), (None if no_status else sbuf[:Cn].cpu().numpy())
    return run


def paired_run(eng):
    """The device form, with the host form run on every call beside it: same status, same bits."""
    dev, host = device_run(eng), device_run(eng, host=True)

    def run(b, drop, **kw):
        out, st = dev(b, drop, **kw)
        h, sh = host(b, drop, **kw)
        assert (st is None and sh is None) or np.array_equal(st, sh), (st, sh)
        assert mk.bits(out, h)
        return out, st
    return run


def solve_run(eng):
    """solve(b, first, count, ffirst, prior) of tests/marginalize_edge_checks.py: chain_solve with lambda = NULL."""
    dev = eng.device

    def solve(b, first, count, ffirst, prior):
        status = torch.full((len(first),), 99, dtype=torch.int32, device=dev)
        delta = eng.chain_solve(_t(b.hess, dev), C=len(first), G=b.G, first=_t(np.asarray(first, dtype=np.int64), dev),
                                count=_t(np.asarray(count, dtype=np.int32), dev), ffirst=_t(np.asarray(ffirst, dtype=np.int64), dev),
                                prior=_t(prior, dev), status=status, out=torch.full((b.S, 15), mk.SENTINEL, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return delta.cpu().numpy(), status.cpu().numpy()
    return solve


# ------------------------------------------------------------------------------------------ 1. the freeze
def test_frozen_chains_and_failures_with_an_m_per_chain(eng):
    """A chain whose m is below its wavefront mates' goes on executing on its carried block plus Pr_m: where Pr_m is the broken block
    its pivots fail in every idle trip, and status must not hear of it."""
    mk.check_frozen_failures(paired_run(eng))


def test_frozen_pivots_do_not_count(eng):
    mk.check_frozen_pivots_do_not_count(paired_run(eng))


def test_long_chain_freezes_its_mates(eng):
    """63 trips beside chains that stop after 0 and 1: the chain of two states re-reads a Pr_m with a NaN in it 62 times."""
    mk.check_long_freeze(paired_run(eng), mz.GATE_LAM_DEVICE, mz.GATE_ETA_DEVICE)


# ------------------------------------------------------------------------------------------ 2. NaN, status, zero
def test_nan_in_the_inputs(eng):
    mk.check_nan_inputs(paired_run(eng))


def test_status_law_across_marginalize_and_solve(eng):
    mk.check_status_law(device_run(eng), solve_run(eng))


def test_a_zero_block_is_a_failed_pivot(eng):
    mk.check_zero_block(paired_run(eng))


# ------------------------------------------------------------------------------------------ 3. ffirst, clamps, M
def test_refusal_boundary_of_ffirst(eng):
    mk.check_ffirst_boundaries(device_run(eng))
    base, cases = cc.ffirst_boundary_cases()
    host = device_run(eng, host=True)
    for c, ff, call, status in cases:                                         # the host form refuses the whole call instead
        for drop in mz.ffirst_drops(base.b.count):
            if status:
                with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain %d leave" % c):
                    host(call.b, drop, **mk.kw_of(call))
            else:
                assert host(call.b, drop, **mk.kw_of(call))[1].tolist() == [0] * 4


def test_ffirst_null_with_an_explicit_first(eng):
    mk.check_ffirst_null(paired_run(eng))


def test_clamps_of_first_count_G_and_S(eng):
    mk.check_clamps(device_run(eng))
    mk.check_clamps(paired_run(eng), only="G = 17")                           # the host form clamps count to G and validates the rest
    host = device_run(eng, host=True)
    for name, raw, clamped in cc.clamp_cases():
        drop = mz.plan_drop(clamped.b, "mixed2")
        if name == "first beyond S":
            with pytest.raises(cpi_amd.CpiError, match="the states of chain 9 leave"):
                host(raw.b, drop, **mk.kw_of(raw))
        if name == "S cuts the last chain":
            with pytest.raises(cpi_amd.CpiError, match="the states of chain 10 leave"):
                host(raw.b, drop, **mk.kw_of(raw))
            one = drop.copy()
            one[10] = 1                                                       # valid for the count given, not for the clamped one
            with pytest.raises(cpi_amd.CpiError, match="drop of chain 10 leaves"):
                host(clamped.b, one, **mk.kw_of(clamped))


def test_scalar_M_is_an_array_filled_with_M(eng):
    mk.check_scalar_against_array(device_run(eng))
    b = mz.scaled_case()[0]
    with pytest.raises(cpi_amd.CpiError, match="drop of chain 1 leaves"):     # chain 0 has no states; chain 1 has one
        device_run(eng, host=True)(b, 3, first=None, count=b.count, ffirst=None)


# ------------------------------------------------------------------------------------------ 4. status == NULL, call sizes
def test_status_null(eng):
    mk.check_status_null(paired_run(eng))


def test_call_sizes_around_a_wavefront(eng):
    mk.check_call_sizes(paired_run(eng))


# ------------------------------------------------------------------------------------------ 5. powers of two
def test_scaled_by_a_power_of_two(eng):
    """pivot_rsqrt away from magnitudes near 1e8.  4^k goes through it exactly (tests/test_gpu_sqrt_info_edges.py holds the
    square-root information to that with the same function), so even exponents are held to the unscaled bits."""
    mk.check_scaling(paired_run(eng), mz.GATE_LAM_DEVICE, mz.GATE_ETA_DEVICE)
