"""What the edge cases of tests/marginalize_cases.py must give, stated once for the host twin (tests/test_marginalize_cpu.py) and for
the device (tests/test_gpu_marginalize_edges.py).  TEST INFRASTRUCTURE ONLY.

A check takes run(b, drop, **kw) -> (out [C, 136], status [C]): cpi_chain_marginalize_batch on the arrays of the cc.Batch b.  drop is
an int (M with drop = NULL) or an array [C].  kw may hold
    first, count, ffirst   an array [C], or None for NULL; a key that is absent means the batch's own array.  C is the length of the
                           first of them that is an array, else b.C
    G, S                   the batch's unless given; S < b.S passes the leading S rows of prior
    hess, prior            arrays in place of the batch's;  with_prior=False: prior = NULL
    status_in              what the status array holds before the call (99 by default)
    no_status=True         status = NULL: the runner returns None for it
The runner lets a row of SENTINEL follow out and one element of 99 follow status, and asserts itself that both are intact after the
call.  Some checks also take solve(b, first, count, ffirst, prior) -> (delta [S, 15], status [C]), cpi_chain_solve_batch with
lambda = NULL on the arrays of b with the given prior.

Every expectation is a sentence of include/cpi_amd.h: an exact status, NaN in exactly the entries stated, the bits of another call
in every other entry.  The reference-gated checks print their metrics before they assert."""
import numpy as np

from tests import chain_cases as cc
from tests import marginalize_cases as mz

SENTINEL = -7.0


def kw_of(call):
    """The keywords of run for a cc.Call: first / count / ffirst as the call has them (None: NULL), its G and S."""
    return dict(first=call.first, count=call.count, ffirst=call.ffirst, G=call.G, S=call.S)


def bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def nan_entries(row):
    return set(np.nonzero(np.isnan(row))[0].tolist())


# ------------------------------------------------------------------------------------------ frozen chains, per-chain m with failures
def check_frozen_failures(run):
    """(a) status = s + 1 of the chain's broken block if s < m_c, else 0, with an m of its own per chain: a frozen chain whose Pr_m is
    the broken block goes on failing its pivots in the trips it idles through, and that must not reach status.  Failed rows are all
    NaN.  A chain whose broken block lies beyond state m has the bits of the clean batch; one whose broken block IS Pr_m has, in every
    entry, (N + 0.0) + Pr_m with N the carried block the clean batch gives once its Pr_m is zeroed -- the bits of the clean batch
    everywhere but at the one entry that holds the -1e12."""
    results = []
    for k in range(len(mz.FREEZE_DROPS)):
        good, bad, drop, status = mz.freeze_failure_case(k)
        clean, st0 = run(good, drop)
        carried, st1 = run(good, drop, prior=mz.without_prior_m(good, drop))
        out, st = run(bad, drop)
        assert st0.tolist() == [0] * 8 and st1.tolist() == [0] * 8 and np.isfinite(clean).all() and np.isfinite(carried).all(), (st0, st1)
        assert st.tolist() == status, (k, st)
        at_m = 0
        for c in range(8):
            if status[c]:
                assert np.isnan(out[c]).all(), (k, c)
                continue
            assert np.isfinite(out[c]).all() and out[c, 135] == 0.0, (k, c)
            row = bad.prior[mz.prior_row_m(bad, drop, c)]
            assert np.array_equal(out[c, :135], (carried[c, :135] + 0.0) + row[:135]), (k, c)
            differs = np.nonzero(out[c] != clean[c])[0].tolist()
            if c in cc.FAILURES and cc.FAILURES[c][0] == drop[c]:
                p = cc.FAILURES[c][1]
                assert differs == [cc.tri(p) + p] and out[c, differs[0]] < -0.9e12, (k, c, differs)
                at_m += 1
            else:
                assert differs == [], (k, c, differs)
        assert at_m >= 1, k                                      # the case holds a frozen chain whose Pr_m is the broken block
        results.append((out, st))
    return results


def check_frozen_pivots_do_not_count(run):
    """(b) the good batch with Pr_m of chains 0, 2, 4 and 6 -- all frozen beside an m of 3 -- made -1e12 on its whole diagonal: status 0
    everywhere, every row finite, and row c the row of chain c called alone (C = 1 has no frozen trip), bit for bit.  Then a NaN at
    packed entry 7 of the same rows: exactly that entry is NaN, status is 0, every other entry has the bits of the unmodified call."""
    b, prior, drop = mz.poison_case("negative")
    out, st = run(b, drop, prior=prior)
    assert st.tolist() == [0] * 8 and np.isfinite(out).all(), st
    for c in range(8):
        one, s1 = run(b, drop[[c]], prior=prior, first=b.first[[c]], count=b.count[[c]], ffirst=b.ffirst[[c]])
        assert s1.tolist() == [0] and np.array_equal(one[0], out[c]), c
    for c in mz.POISON_CHAINS:
        assert (out[c, cc.tri(np.arange(15)) + np.arange(15)] < -0.9e12).all(), c
    base, st0 = run(b, drop)
    b, prior, drop = mz.poison_case("nan")
    out, st = run(b, drop, prior=prior)
    assert st0.tolist() == [0] * 8 and st.tolist() == [0] * 8 and np.isfinite(base).all(), st
    for c in range(8):
        assert nan_entries(out[c]) == ({mz.POISON_ENTRY} if c in mz.POISON_CHAINS else set()), (c, nan_entries(out[c]))
        keep = ~np.isnan(out[c])
        assert np.array_equal(out[c, keep], base[c, keep]), c
    return out, st


def check_long_freeze(run, gate_lam, gate_eta):
    """(c) 64 states beside 1, 0 and 2 under m = 63, 0, -, 1: the chain of two states idles through 62 trips on a Pr_m that holds a NaN.
    Its row carries exactly that NaN at status 0; the chain of 64 states keeps the bits of the unmodified call and meets the gates."""
    b, prior, drop = mz.long_freeze_case()
    ref = mz.Reference(b, drop)
    ref.check_inputs()
    base, st0 = run(b, drop, count=b.count, first=None, ffirst=None)
    out, st = run(b, drop, count=b.count, first=None, ffirst=None, prior=prior)
    m_c, m_d = ref.metrics(base)
    print("LONG %s under drop %s: cond(A_EE) max %.1e, (c) %.3e (gate %.2e), (d) %.3e (gate %.2e)"
          % (cc.LONG, mz.LONG_DROP, ref.cond.max(), m_c, gate_lam, m_d, gate_eta))
    assert st0.tolist() == [0, 0, -1, 0] and st.tolist() == [0, 0, -1, 0], (st0, st)
    assert m_c <= gate_lam and m_d <= gate_eta
    assert np.isfinite(base[[0, 1, 3]]).all() and np.isnan(base[2]).all() and np.isnan(out[2]).all()
    assert np.array_equal(out[0], base[0]) and np.array_equal(out[1], base[1])
    assert nan_entries(out[3]) == {mz.POISON_ENTRY}
    keep = ~np.isnan(out[3])
    assert np.array_equal(out[3, keep], base[3, keep]) and out[3, 135] == 0.0
    return out, st


# ------------------------------------------------------------------------------------------ NaN inputs
def check_nan_inputs(run):
    """cc.nan_plan() under M = 1, 2, 3: status 0 does not promise a finite row.  A NaN in what state m receives (the trailing block, U
    or g of factor m - 1) reaches exactly the entries it touches and leaves the status; a NaN in an eliminated block fails the chain."""
    gcall, bcall, _ = cc.nan_plan()
    results = []
    for M in (1, 2, 3):
        clean, st0 = run(gcall.b, M, **kw_of(gcall))
        out, st = run(bcall.b, M, **kw_of(bcall))
        sets = mz.nan_sets(M)
        print("nan_plan, M = %d: status %s, NaN entries %s" % (M, st.tolist(), {c: sorted(nan_entries(out[c])) for c in range(4) if st[c] == 0 and np.isnan(out[c]).any()}))
        assert st0.tolist() == [0] * 4 and np.isfinite(clean).all()
        assert st.tolist() == mz.NAN_STATUS[M], (M, st)
        for c in range(4):
            if st[c]:
                assert np.isnan(out[c]).all(), (M, c)
                continue
            assert nan_entries(out[c]) == set(sets.get(c, ())), (M, c, sorted(nan_entries(out[c])))
            keep = ~np.isnan(out[c])
            assert np.array_equal(out[c, keep], clean[c, keep]) and out[c, 135] == 0.0, (M, c)
        results.append((out, st))
    # a right-hand side further back: eta[3] of state 0 under M = 2 is NaN in y_0 from row 3 on, hence in every entry of W^T y that
    # state 1 receives and in all of what state 2 receives from it; no pivot sees it and Lam does not depend on it
    b, prior = mz.rhs_nan_case()
    clean, _ = run(gcall.b, 2, **kw_of(gcall))
    out, st = run(b, 2, prior=prior, **kw_of(gcall))
    print("eta[3] of state 0 NaN, M = 2: status %s, NaN entries of chain 0: %s" % (st.tolist(), sorted(nan_entries(out[0]))))
    assert st.tolist() == [0] * 4 and nan_entries(out[0]) == set(range(cc.tri(15), cc.tri(15) + 15))
    assert np.array_equal(out[0, :120], clean[0, :120]) and out[0, 135] == 0.0 and np.array_equal(out[1:], clean[1:])
    results.append((out, st))
    return results


def check_status_law(run, solve):
    """The status across the two entries, for cc.nan_plan() and cc.failure_plan() under M = 1, 2, 3: with `full` the status of the FULL
    chain's solve, marginalize reports full where 0 < full <= m and 0 elsewhere, and the solve of the reduced chain (mz.reduced)
    then reports max(full - m, 0).  A NaN that reached a row of status 0 is reported by that solve: a status, or a NaN delta."""
    for plan in (cc.nan_plan, cc.failure_plan):
        _, bcall, want = plan()
        b = bcall.b
        _, full = solve(b, b.first, b.count, b.ffirst, b.prior)
        assert full.tolist() == want, (plan.__name__, full)
        for M in (1, 2, 3):
            out, st = run(b, M)
            assert st.tolist() == [int(f) if 0 < f <= M else 0 for f in full], (plan.__name__, M, st)
            first, count, ffirst, prior = mz.reduced(b, np.full(b.C, M), out, st)
            delta, st2 = solve(b, first, count, ffirst, prior)
            for c in range(b.C):
                if st[c]:
                    continue
                assert st2[c] == max(int(full[c]) - M, 0), (plan.__name__, M, c, st2)
                rows = delta[first[c]:first[c] + count[c]]
                if np.isnan(out[c]).any():                           # a failed chain's delta is NaN, and so is one whose eta alone is
                    assert np.isnan(rows).all(), (plan.__name__, M, c)
                elif st2[c] == 0 and np.isfinite(b.chain(c)[0][M:]).all():
                    assert np.isfinite(rows).all(), (plan.__name__, M, c)


# ------------------------------------------------------------------------------------------ an exactly zero block
def check_zero_block(run):
    """No prior, and chain 0's one factor row exactly zero, of either sign: its first pivot is 0, which is not > 0.  Status [1, 0], a NaN
    row and a finite neighbour."""
    results = []
    for negative in (False, True):
        b, hess = mz.zero_block_case(negative)
        out, st = run(b, 1, hess=hess, with_prior=False)
        assert st.tolist() == [1, 0], (negative, st)
        assert np.isnan(out[0]).all() and np.isfinite(out[1]).all() and out[1, 135] == 0.0, negative
        results.append((out, st))
    return results


# ------------------------------------------------------------------------------------------ ffirst
def check_ffirst_boundaries(run):
    """The refusal is the solve's, over the WHOLE chain's factor rows: ff > F - (n - 1) refuses and ff == F - (n - 1) does not, whether
    m = n - 1 rows are read, none (m = 0), or one row that itself lies inside [0, F).  A chain of one state is never refused."""
    base, cases = cc.ffirst_boundary_cases()
    for drop in mz.ffirst_drops(base.b.count):
        g, st0 = run(base.b, drop, **kw_of(base))
        assert st0.tolist() == [0] * 4 and np.isfinite(g).all(), (drop, st0)
        for c, ff, call, status in cases:
            out, st = run(call.b, drop, **kw_of(call))
            assert st.tolist() == [status if k == c else 0 for k in range(4)], (drop.tolist(), c, ff, st)
            for k in range(4):
                if k == c and status:
                    assert np.isnan(out[k]).all(), (c, ff)
                else:
                    assert np.array_equal(out[k], g[k]), (drop.tolist(), c, ff, k)


def check_ffirst_null(run):
    """ffirst NULL means first[c] - c with an explicit first too; count NULL beside an explicit first means G."""
    for counts, drop in mz.FFIRST_NULL_DROPS:
        tile, null = cc.ffirst_null_case(counts)
        kw = kw_of(null)
        if np.isscalar(drop):
            kw["count"] = None
        else:
            drop = np.asarray(drop, dtype=np.int32)
        g, st0 = run(tile.b, drop, **kw_of(tile))
        out, st = run(null.b, drop, **kw)
        assert st0.tolist() == [0] * 5 and st.tolist() == [0] * 5 and np.isfinite(g).all(), (counts, st)
        assert np.array_equal(out, g), counts


# ------------------------------------------------------------------------------------------ clamps, scalar M
def check_clamps(run, only=None):
    """A call whose first / count / G / S need clamping is the call given the clamped values, and m is judged against the CLAMPED
    count: the drop plans are taken from the clamped counts, and an m that is valid for the count given and not for the clamped one
    is refused."""
    for name, raw, clamped in cc.clamp_cases():
        if only is not None and name != only:
            continue
        for plan in ("mixed0", "mixed2"):
            drop = mz.plan_drop(clamped.b, plan)
            want = mz.expected_status(clamped.b, drop)
            out, st = run(raw.b, drop, **kw_of(raw))
            g, sg = run(clamped.b, drop, **kw_of(clamped))
            assert np.array_equal(sg, want) and np.array_equal(st, want), (name, plan, st, sg)
            assert np.isfinite(g[want == 0]).all() and np.isnan(g[want != 0]).all() and bits(out, g), (name, plan)
        if name == "S cuts the last chain":
            assert raw.b.count[10] == 2 and drop[10] == 0
            assert np.array_equal(out[10, :135], raw.b.prior[raw.b.first[10], :135]) and out[10, 135] == 0.0      # m = 0: Pr_0 as it is
            one = drop.copy()
            one[10] = 1                                              # inside [0, 2), outside [0, 1)
            cut, sc = run(raw.b, one, **kw_of(raw))
            assert sc[10] == -1 and np.isnan(cut[10]).all(), sc
            assert np.array_equal(np.delete(sc, 10), np.delete(st, 10)) and bits(np.delete(cut, 10, 0), np.delete(out, 10, 0))


def check_scalar_against_array(run):
    """M with drop = NULL is an array filled with M, and every chain with n <= M is refused alone."""
    b = mz.scaled_case()[0]
    M = 3
    out, st = run(b, M, first=None, count=b.count, ffirst=None)
    arr, sa = run(b, np.full(b.C, M, dtype=np.int32), first=None, count=b.count, ffirst=None)
    assert st.tolist() == np.where(b.count > M, 0, -1).tolist() and (st == -1).sum() == 6 and (st == 0).sum() == 5, st
    assert np.array_equal(sa, st) and bits(arr, out)
    assert np.isnan(out[st != 0]).all() and np.isfinite(out[st == 0]).all()
    return out, st


# ------------------------------------------------------------------------------------------ status == NULL, call sizes
def check_status_null(run):
    """status == NULL gives the rows of the call with a status array, NaN rows included; a status array is overwritten in every
    element below C whatever it held."""
    _, bad, drop, status = mz.freeze_failure_case(0)
    out, st = run(bad, drop)
    none, sn = run(bad, drop, no_status=True)
    assert sn is None and st.tolist() == status and bits(none, out) and np.isnan(none[0]).all()
    for fill in (-1, 77):
        again, sf = run(bad, drop, status_in=np.full(8, fill, dtype=np.int32))
        assert sf.tolist() == status and bits(again, out), (fill, sf)


def check_call_sizes(run):
    """C = 1 .. 9 over the leading chains of (a), the 9th being chain 0 once more: the leading rows of the C = 8 call, bit for bit (the
    last wavefront of a call has 1, 2, 3 or 4 chains; the runner checks what follows out and status)."""
    for k in range(len(mz.FREEZE_DROPS)):
        _, bad, drop, status = mz.freeze_failure_case(k)
        idx = np.arange(9) % 8
        whole, sw = run(bad, drop)
        assert sw.tolist() == status
        for C in range(1, 10):
            i = idx[:C]
            out, st = run(bad, drop[i], first=bad.first[i], count=bad.count[i], ffirst=bad.ffirst[i])
            assert out.shape == (C, 136) and st.tolist() == [status[c] for c in i], (k, C, st)
            assert bits(out, whole[i]), (k, C)


# ------------------------------------------------------------------------------------------ scaling by a power of two
def check_scaling(run, gate_lam, gate_eta):
    """hess and prior times 2^e.  Every term of out is homogeneous of degree one in them, and a scaling by 4^k goes through
    pivot_rsqrt exactly: for even e out is 2^e times the unscaled out, bit for bit, and entry 135 stays 0.0.  e = 301 puts an odd
    exponent under the square root: out / 2^301 is held to the gates against the unscaled longdouble reference."""
    b, drop, ref = mz.scaled_case()
    kw = dict(first=None, count=b.count, ffirst=None)
    base, st0 = run(b, drop, **kw)
    m_c, m_d = ref.metrics(base)
    print("scaled, 2^0: cond(A_EE) max %.1e, (c) %.3e (gate %.2e), (d) %.3e (gate %.2e)" % (ref.cond.max(), m_c, gate_lam, m_d, gate_eta))
    assert np.array_equal(st0, ref.status) and m_c <= gate_lam and m_d <= gate_eta
    ok = st0 == 0
    assert ok.sum() == 10 and np.isfinite(base[ok]).all() and np.isnan(base[~ok]).all()
    for e in mz.SCALE_EXPONENTS:
        s = cc.scaled_batch(e)
        out, st = run(s, drop, **kw)
        assert np.array_equal(st, st0), (e, st)
        assert np.isfinite(out[ok]).all() and np.isnan(out[~ok]).all() and (out[ok, 135] == 0.0).all(), e
        back = out * 2.0 ** -e                                       # exact: no entry of these chains is near the subnormals
        m_c, m_d = ref.metrics(back)
        exact = bits(out, base * 2.0 ** e)
        print("scaled, 2^%d: (c) %.3e (d) %.3e, 2^e times the unscaled bits: %s" % (e, m_c, m_d, exact))
        assert m_c <= gate_lam and m_d <= gate_eta, e
        if e % 2 == 0:
            assert exact, e
