"""What the edge cases of tests/chain_cases.py must give, stated once for the host twins (tests/test_chain_cpu.py,
tests/test_marginals_cpu.py) and for the device (tests/test_gpu_chain_edges.py).  TEST INFRASTRUCTURE ONLY.

A check takes run(call, status_in=None) -> Result: the solve of a cc.Call and, where the runner has them, the marginals of the
same workspace.  delta is pre-filled with SENTINEL, cov and cross with Result.fill (NaN on the device, where the entry's own
allocation does the same; the sentinel on the twins, where it tells a row nobody wrote from a poisoned one).  Every expectation is a
sentence of include/cpi_amd.h: an exact status, NaN in exactly the rows of a failed or refused chain, the bits of another call in
every other row, and nothing written to rows of no chain."""
import numpy as np

from tests import chain_cases as cc

SENTINEL = -7.0


class Result:
    def __init__(self, delta, status, cov=None, cross=None, fill=np.nan):
        self.delta, self.status, self.cov, self.cross, self.fill = delta, status, cov, cross, fill


def kept(x, fill):
    return bool(np.isnan(x).all() if np.isnan(fill) else (x == fill).all())


def same(r, call, c, g, gcall, gc=None, delta=True):
    """Chain c of result r has the bits of chain gc of result g (cross: every row but the last state's, which nobody writes)."""
    rows, grows = call.rows(c), gcall.rows(c if gc is None else gc)
    assert rows.stop - rows.start == grows.stop - grows.start, c
    if delta:
        assert np.isfinite(g.delta[grows]).all() and np.array_equal(r.delta[rows], g.delta[grows]), ("delta", c)
    if r.cov is not None:
        assert np.isfinite(g.cov[grows]).all() and np.array_equal(r.cov[rows], g.cov[grows]), ("cov", c)
        assert np.isfinite(g.cross[grows][:-1]).all() and np.array_equal(r.cross[rows][:-1], g.cross[grows][:-1]), ("cross", c)


def is_nan(r, call, c, delta=True, cov=True):
    rows = call.rows(c)
    assert rows.stop > rows.start, c
    if delta:
        assert np.isnan(r.delta[rows]).all(), ("delta", c)
    if cov and r.cov is not None:
        assert np.isnan(r.cov[rows]).all() and np.isnan(r.cross[rows][:-1]).all(), ("cov", c)


def unowned(r, call):
    """Rows of no chain keep what was there, and so does the cross row of every chain's last state."""
    own, last = call.owned()
    assert (r.delta[~own] == SENTINEL).all(), np.nonzero(~own & (r.delta != SENTINEL).any(axis=1))[0]
    if r.cov is not None:
        assert kept(r.cov[~own], r.fill) and kept(r.cross[~own | last], r.fill)


def equal(r, g):
    """Two results agree in status and bit for bit, rows nobody wrote included."""
    assert np.array_equal(r.status, g.status), (r.status, g.status)
    assert np.array_equal(r.delta, g.delta, equal_nan=True)
    assert (r.cov is None) == (g.cov is None)
    if r.cov is not None:
        assert np.array_equal(r.cov, g.cov, equal_nan=True) and np.array_equal(r.cross, g.cross, equal_nan=True)


def check_failure_plan(run):
    """status = s + 1 wherever the pivot is: state 0 and the last state, pivots 0, 7 and 14, the chain in lanes 48 .. 63, the four
    chains of one wavefront at different states (the first failure of each wins).  Failed chains are NaN, chains 4 and 7 keep the bits
    of the clean call."""
    gcall, bcall, status = cc.failure_plan()
    g, r = run(gcall), run(bcall)
    assert g.status.tolist() == [0] * 8 and r.status.tolist() == status, r.status
    for c in range(8):
        if status[c]:
            is_nan(r, bcall, c)
        else:
            same(r, bcall, c, g, gcall)
    unowned(r, bcall)
    return r


def check_nan_plan(run):
    """A NaN in a D or a U block: status = state + 1 and a NaN chain.  A NaN in g alone: every pivot is fine, status 0, every delta row
    of the chain NaN -- and its covariances, which do not depend on g, those of the clean call."""
    gcall, bcall, status = cc.nan_plan()
    g, r = run(gcall), run(bcall)
    assert g.status.tolist() == [0] * 4 and r.status.tolist() == status == [2, 3, 3, 0], r.status
    for c in (0, 1, 2):
        is_nan(r, bcall, c)
    is_nan(r, bcall, 3, cov=False)
    same(r, bcall, 3, g, gcall, delta=False)
    unowned(r, bcall)
    return r


def check_ffirst_boundaries(run):
    """ff > F - (n - 1) refuses, ff == F - (n - 1) does not, and a chain of one state has no factor row to refuse."""
    base, cases = cc.ffirst_boundary_cases()
    g = run(base)
    assert g.status.tolist() == [0] * 4
    for c, ff, call, status in cases:
        r = run(call)
        assert r.status.tolist() == [status if k == c else 0 for k in range(4)], (c, ff, r.status)
        for k in range(4):
            if k == c and status:
                is_nan(r, call, k)
            else:
                same(r, call, k, g, base)
        unowned(r, call)


def check_ffirst_null(run):
    """ffirst NULL means first[c] - c with an explicit first too; count NULL beside an explicit first means G."""
    for counts, with_count in (((5, 3, 5, 1, 2), True), ((5,) * 5, False)):
        tile, null = cc.ffirst_null_case(counts)
        if not with_count:
            null = cc.Call(null.b, first=null.b.first)
        g, r = run(tile), run(null)
        assert g.status.tolist() == [0] * 5 and r.status.tolist() == [0] * 5, (counts, r.status)
        for c in range(5):
            same(r, null, c, g, tile)
        unowned(r, null)


def check_clamps(run, only=None):
    """A call whose first / count / G / S need clamping is the call given the clamped values."""
    for name, raw, clamped in cc.clamp_cases():
        if only is not None and name != only:
            continue
        r, g = run(raw), run(clamped)
        assert (g.status == 0).all() and np.array_equal(r.status, g.status), (name, r.status)
        own, last = clamped.owned()
        assert np.isfinite(g.delta[own]).all() and (g.cov is None or (np.isfinite(g.cov[own]).all() and np.isfinite(g.cross[own & ~last]).all())), name
        equal(r, g)
        unowned(r, clamped)
        assert all(raw.states(c)[1] == clamped.states(c)[1] for c in range(raw.C)), name


def check_empty_wave(run, gate_a, gate_b):
    """A wavefront whose four chains have no states writes status 0 and nothing else; the chains of the next wavefront solve."""
    b, ref = cc.empty_wave_case()
    call = cc.Call(b, count=b.count)
    r = run(call)
    a, bb = ref.metrics(r.delta)
    print("empty wavefront: (a) %.3e (gate %.2e), (b) %.3e (gate %.2e)" % (a, gate_a, bb, gate_b))
    assert r.status.tolist() == [0] * 7, r.status
    assert a <= gate_a and bb <= gate_b
    own, last = call.owned()
    assert own.sum() == 5 and (r.cov is None or (np.isfinite(r.cov[own]).all() and np.isfinite(r.cross[own & ~last]).all()))
    unowned(r, call)
    return r


def check_zero_pivot(run):
    """A block that is exactly zero is a failed pivot: no prior and one state, with lambda = 0 under identity damping and with any
    lambda under diagonal damping (lambda * 0).  Identity damping 2 of a zero block is 2 delta = 0."""
    out = []
    for diagonal in (False, True):
        call, status = cc.zero_pivot_case(diagonal)
        r = run(call)
        assert r.status.tolist() == status, (diagonal, r.status)
        is_nan(r, call, 0)
        if diagonal:
            is_nan(r, call, 1)
        else:
            assert (r.delta[call.rows(1)] == 0.0).all() and (r.cov is None or np.isfinite(r.cov[call.rows(1)]).all())
        rows = call.rows(2)
        assert np.isfinite(r.delta[rows]).all() and (r.cov is None or (np.isfinite(r.cov[rows]).all() and np.isfinite(r.cross[rows][:-1]).all()))
        unowned(r, call)
        out.append(r)
    return out


def check_status_overlay(run):
    """A non-zero status of the caller's for a chain that solved: exactly those chains are NaN in cov and cross, whatever the code."""
    b = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
    call = cc.Call.explicit(b)
    g = run(call)
    assert (g.status == 0).all() and g.cov is not None
    st = np.zeros(b.C, dtype=np.int32)
    st[1], st[3] = 7, -1
    r = run(call, status_in=st)
    assert np.array_equal(r.delta, g.delta) and (r.status == 0).all()
    for c in range(b.C):
        if b.count[c] == 0:
            continue
        if st[c]:
            is_nan(r, call, c, delta=False)
        else:
            same(r, call, c, g, call)
    unowned(r, call)
