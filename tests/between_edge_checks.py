"""What cpi_state_between_batch must give at the edges of its contract, stated once for the host twin (tests/test_between_edges_cpu.py,
where each check is also shown to fail on a twin with the defect it is there for) and for the device (tests/test_gpu_between_edges.py).
TEST INFRASTRUCTURE ONLY.  Built on tests/between_cases.py, in the shape of tests/fix_edge_checks.py.

Every check takes a function that runs the entry -- run(case, **form) -> (hess [F, 496], chi2 [F], chi2_m [M]), weight and both bases
given unless the form says otherwise -- and asserts on what comes back; nothing here knows whether a GPU is behind it.  The forms are the
keyword arguments that tests/test_gpu_between.dev_between and tests/test_between_cpu.twin share: inplace, alias = (hess in place, chi2 in
place), base, bases = (hess_base given, chi2_base given), rows, cost, weight, padded.

  check_broken          a broken mfirst or state index is clamped where it is read: padded arrays tell a clamp from its absence without
                        a fault, and the clamp being specified, the bits are those of the call clamped in numpy
  check_mixed_aliasing  hess and chi2 in place or not, each by itself
  check_nan_locality    one NaN in z, R, weight, a state or a base reaches what the contract says and nothing else
  check_identity / check_pi / check_scaled    residuals of exactly 0, rotations of exactly pi, z quaternions far from unit norm
  check_weight_zero     weight 0 removes a measurement exactly
  check_long            a fold of 300 against the reference
  check_many            1027 factors: a factor's bits do not depend on F or on where the factor sits

WHAT A NaN REACHES, from the table of include/cpi_amd.h.  A touched entry (a, b) of factor f is P_ab = sum_r A_ra A_rb folded with
fma(w, P_ab, .), A = [R J | -R e]; column c of A holds A_0c = sum_k R[0][k] J[k][c], which takes in every row of column c of J, and the
b column holds wh_0, which takes in every e_k.  So an entry is NaN exactly when one of its two columns is "dirty", and the others are
the clean call's bits (the same arithmetic on the same numbers).  Dirty columns, by where the one NaN sits (theta_i = columns 0 1 2,
p_i = 12 13 14, theta_j = 15 16 17, p_j = 27 28 29, b = 30; "all" = every touched column):
    place                         position            orientation          pose                      chi2[f]   chi2_m
    z[m] (q or p part)            b                   b                    b                         NaN       NaN at m
    R[m][0], R[m][last]           all                 all                  all                       NaN       NaN at m
    weight[m]                     all                 all                  all                       NaN       clean
    q_i (w) of a state            all                 theta_i, b           theta_i, p_i, p_j, b      NaN       NaN, every m of f
    q_j (w) of a state            --  (not used)      theta_i, b           theta_i, b                NaN       NaN, every m of f
    p_i or p_j (x) of a state     theta_i, b          --  (not read)       theta_i, b                NaN       NaN, every m of f
    hess_base[f][slot]            that entry alone, touched or not; chi2 and chi2_m clean
    chi2_base[f]                  chi2[f] alone
    state doubles 4 .. 12         nothing: bg, v, ba are not read (orientation: 13 .. 15 neither)
(G are the entries with both columns < 30, g those of column 30 with a row < 30, f the entry (30, 30): "b dirty" is g and f NaN, G
clean.)  theta_j is never dirty through a state: its column of J is -I and zeros.  R_i = quat_2_Rot(q_i) has w in every entry, so a NaN
w makes all of R_i, y and R_ij NaN; -[y x] has a NaN in every column.  A NaN in a state reaches EVERY factor with measurements that uses
the state, and no other factor; a factor without measurements loads no state."""
import numpy as np

from tests import between_cases as bc
from tests.fix_edge_checks import GUARD, bits, same, with_nan

PAD = 4                                       # measurements of padding on either side of z, R, weight and chi2_m
PADS = 2                                      # states of padding on either side of states
TARGETS = (0, 3, 5)                           # 17 measurements in lane group 0; the last factor of its wavefront; 17 in lane group 1
UNTOUCHED = bc.hslot(4, 5)                    # an entry of the bg block of state i: no kind touches it
BLOCKS = dict(theta_i=(0, 1, 2), p_i=(12, 13, 14), theta_j=(15, 16, 17), p_j=(27, 28, 29), b=(30,))
ALL = tuple(BLOCKS)
# dirty blocks by (kind, part of the state, role of the state in the factor)
DIRTY = {(0, "q", "i"): ALL, (0, "q", "j"): (), (0, "p", "i"): ("theta_i", "b"), (0, "p", "j"): ("theta_i", "b"),
         (1, "q", "i"): ("theta_i", "b"), (1, "q", "j"): ("theta_i", "b"), (1, "p", "i"): (), (1, "p", "j"): (),
         (2, "q", "i"): ("theta_i", "p_i", "p_j", "b"), (2, "q", "j"): ("theta_i", "b"), (2, "p", "i"): ("theta_i", "b"), (2, "p", "j"): ("theta_i", "b")}
PART = {"q": 3, "p": 13}                      # the double of a state that gets the NaN: q.w, p.x


def variant(c, **arrays):
    """The case with some of its arrays replaced (the others shared)."""
    v = bc.Case.__new__(bc.Case)
    v.__dict__.update(c.__dict__)
    v.__dict__.update(arrays)
    return v


def _show(what, m):
    print("%s: %s" % (what, ", ".join("%s %.3g" % kv for kv in sorted(m.items()))))


# ---------------------------------------------------------------------------------------------- broken mfirst, broken indices
class Padded:
    """z, R, weight and chi2_m of a case as interior views of larger arrays, PAD measurements on either side, and the states with PADS
    states on either side: NaN in the input pads, GUARD in the chi2_m pad and fill.  A range that leaves [0, M] by less than PAD and an
    index that leaves [0, S) by at most PADS stay inside the allocations: a missing clamp reads a NaN or writes over a guard, and neither
    is a fault."""
    PAD, PADS = PAD, PADS

    def __init__(self, c):
        self.c, self.big = c, {}
        for name, a, n in (("z", c.z, PAD), ("R", c.R, PAD), ("weight", c.weight, PAD), ("states", c.states, PADS)):
            b = np.full((len(a) + 2 * n,) + a.shape[1:], np.nan)
            b[n:n + len(a)] = a
            self.big[name] = b
        self.big["chi2_m"] = np.full(c.M + 2 * PAD, GUARD)


def _refused(mf, M):
    return next(f for f in range(len(mf) - 1) if mf[f] < 0 or mf[f + 1] > M or mf[f + 1] < mf[f])


def broken_mfirsts(c):
    """[(what, the case with a broken mfirst, the factor the host form names)] -- every broken value within (-PAD, M + PAD)."""
    F, M, out = c.F, c.M, []
    for what, f, v in (("mfirst[0] = -3", 0, -3), ("mfirst[F] = M + 3", F, M + 3), ("mfirst[3] = mfirst[2] - 1", 3, int(c.mfirst[2]) - 1),
                       ("mfirst[5] = M + 2", 5, M + 2)):
        mf = c.mfirst.copy()
        mf[f] = v
        assert -PAD < v < M + PAD
        out.append((what, variant(c, mfirst=mf), _refused(mf, M)))
    return out


def broken_indices(c):
    """[(what, the case with one broken state index, the factor the host form names)] -- every broken value within [-PADS, S + PADS),
    each on a factor that has measurements (a factor without them loads no state)."""
    S, out = c.S, []
    for what, name, f, v in (("idx_i = -1", "idx_i", 0, -1), ("idx_j = S", "idx_j", 5, S), ("idx_i = S + 1", "idx_i", 3, S + 1), ("idx_j = -2", "idx_j", 6, -2)):
        idx = getattr(c, name).copy()
        idx[f] = v
        assert -PADS <= v < S + PADS and c.counts[f] > 0
        out.append((what, variant(c, **{name: idx}), f))
    return out


def clamped(c):
    """(m0 [F], m1 [F], si [F], sj [F]) as include/cpi_amd.h clamps them, in numpy."""
    m0 = np.clip(c.mfirst[:-1], 0, c.M)
    m1 = np.maximum(np.clip(c.mfirst[1:], 0, c.M), m0)
    fi, fj = c.pairs()
    return m0, m1, np.clip(fi, 0, c.S - 1), np.clip(fj, 0, c.S - 1)


def one_factor(c, f, m0, m1, si, sj):
    """Factor f of c by itself (F = 1) on the measurements m0 .. m1 - 1 between the states si and sj."""
    v = variant(c, F=1, M=int(m1 - m0), counts=np.array([m1 - m0], dtype=np.int64), mfirst=np.array([0, m1 - m0], dtype=np.int64),
                idx_i=np.array([si], dtype=np.int32), idx_j=np.array([sj], dtype=np.int32), base=np.ascontiguousarray(c.base[f:f + 1]),
                chi2_base=np.ascontiguousarray(c.chi2_base[f:f + 1]))
    v.z, v.R, v.weight = (np.ascontiguousarray(a[m0:m1]) for a in (c.z, c.R, c.weight))
    return v


def check_broken(run, sound_case, broken):
    """For each (what, case, factor) of `broken`, run with padded= the Padded of sound_case: every pad intact, every output finite, and
    hess and chi2 bit for bit those of the call the test clamped itself -- a factor whose clamped range and states are the sound call's
    has the sound call's bits, every other factor those of run() on that factor alone (F = 1) with its clamped range and states: the
    clamped ranges may overlap, and a factor's bits are its own data's only.  chi2_m is compared at the measurements that exactly one
    clamped range owns.  Returns the number of factors that were compared with a call of their own."""
    c, p = sound_case, Padded(sound_case)
    F, M = c.F, c.M
    sound = run(c, padded=p)
    s_m0, s_m1, s_i, s_j = clamped(c)
    alone = 0
    for what, bad, _ in [("sound", c, None)] + list(broken):
        hess, chi2, x2big = run(bad, padded=p)
        x2 = x2big[PAD:PAD + M]
        m0, m1, si, sj = clamped(bad)
        want_h, want_c, want_m = sound[0].copy(), sound[1].copy(), sound[2][PAD:PAD + M].copy()
        owners = np.zeros(M, dtype=np.int64)
        moved = []
        for f in range(F):
            owners[m0[f]:m1[f]] += 1
            if (m0[f], m1[f], si[f], sj[f]) != (s_m0[f], s_m1[f], s_i[f], s_j[f]):
                moved.append(f)
        for f in moved:
            if m1[f] > m0[f]:
                h1, c1, x1 = run(one_factor(c, f, m0[f], m1[f], si[f], sj[f]))
                want_h[f], want_c[f] = h1[0], c1[0]
                want_m[m0[f]:m1[f]] = np.where(owners[m0[f]:m1[f]] == 1, x1, want_m[m0[f]:m1[f]])
                alone += 1
            else:                                                             # nothing left of the range: the base
                want_h[f], want_c[f] = c.base[f], c.chi2_base[f]
        once = owners == 1
        print("%s, %s: factors clamped to another range or state %s, guards chi2_m %s, finite hess %d of %d, chi2 %d of %d, chi2_m owned once %d of %d, "
              "rows equal %d of %d, chi2 equal %d of %d" % (bc.KINDS[c.kind], what, moved, (x2big[:PAD] == GUARD).all() and (x2big[PAD + M:] == GUARD).all(),
              np.isfinite(hess).all(1).sum(), F, np.isfinite(chi2).sum(), F, once.sum(), M, (bits(hess) == bits(want_h)).all(1).sum(), F,
              (bits(chi2) == bits(want_c)).sum(), F))
        assert (x2big[:PAD] == GUARD).all() and (x2big[PAD + M:] == GUARD).all(), what
        assert np.isfinite(hess).all() and np.isfinite(chi2).all() and np.isfinite(x2).all(), what
        assert same(hess, want_h) and same(chi2, want_c), what
        assert same(x2[once], want_m[once]), what
    return alone


# ---------------------------------------------------------------------------------------------- mixed aliasing
MIXED = (("a: hess in place, chi2 out of place", dict(alias=(True, False)), True),
         ("b: hess out of place, chi2 in place", dict(alias=(False, True)), False),
         ("c: hess in place, chi2_base NULL", dict(alias=(True, False), bases=(True, False)), True),
         ("d: hess_base NULL, chi2 in place", dict(alias=(False, True), bases=(False, True)), False),
         ("e: hess in place, no chi2, chi2_m only", dict(alias=(True, False), cost=False), True))


def check_mixed_aliasing(run, kind):
    """include/cpi_amd.h states the in-place rule per array.  Each form of MIXED against the out-of-place call with the same bases, bit
    for bit; where hess is in place, a factor without measurements keeps every bit of its row."""
    c = bc.case(kind, 9)
    none = c.counts == 0
    assert none.any()
    for what, form, rows_in_place in MIXED:
        want = run(c, bases=form.get("bases", (True, True)))
        got = run(c, **form)
        print("%s, %s: hess %s, chi2 %s, chi2_m %s" % (bc.KINDS[kind], what, same(got[0], want[0]), got[1] is None or same(got[1], want[1]), same(got[2], want[2])))
        assert same(got[0], want[0]) and same(got[2], want[2]), what
        assert (got[1] is None) == ("cost" in form) and (got[1] is None or same(got[1], want[1])), what
        assert not np.isnan(got[0]).any() and (got[1] is None or not np.isnan(got[1]).any()), what
        if rows_in_place:
            assert same(got[0][none], c.base[none]), what


# ---------------------------------------------------------------------------------------------- NaN locality
def _entries(kind, blocks):
    """The touched slots of a row with a column in one of the blocks, and the other touched slots."""
    cols = bc.COLS[kind]
    dirty = set(k for b in blocks for k in BLOCKS[b]) & set(cols)
    pairs = [(cols[a], cols[b]) for b in range(len(cols)) for a in range(b + 1)]
    return ([bc.hslot(a, b) for a, b in pairs if a in dirty or b in dirty], [bc.hslot(a, b) for a, b in pairs if not (a in dirty or b in dirty)])


def _expect(clean, got, c, hit, nan_m, cost=True, what=""):
    """hit: {factor: dirty blocks}.  A hit factor has NaN exactly in the touched entries with a dirty column (and in chi2 when `cost`);
    chi2_m is NaN exactly at nan_m; everything else is the clean call's bits."""
    hess, chi2, x2 = got
    others = np.array([f not in hit for f in range(c.F)])
    assert same(hess[others], clean[0][others]) and same(chi2[others], clean[1][others]), what
    rest = np.setdiff1d(np.arange(496), bc.touched(c.kind))
    for f, blocks in hit.items():
        nan, keep = _entries(c.kind, blocks)
        assert np.isnan(hess[f, nan]).all() and same(hess[f, keep], clean[0][f, keep]) and same(hess[f, rest], clean[0][f, rest]), (what, f)
        assert np.isnan(chi2[f]) if cost else same(chi2[f], clean[1][f]), (what, f)
    bad = np.zeros(c.M, dtype=bool)
    bad[nan_m] = True
    assert np.isnan(x2[bad]).all() and same(x2[~bad], clean[2][~bad]), what


def check_nan_locality(run, kind):
    """One NaN, in turn, in every place of the module docstring, out of place and in place; returns the number of calls made."""
    calls = 0
    c, x = bc.case(kind, 9), bc.case(kind, 9, "explicit")
    last = bc.RN[kind] - 1
    zcols = ((0,) if bc.ROT[kind] else ()) + ((bc.ZN[kind] - 1,) if bc.POS[kind] else ())     # one column of the quaternion, one of the position
    for form in (dict(), dict(inplace=True)):
        clean = run(c, **form)
        assert all(np.isfinite(a).all() for a in clean)
        for t in TARGETS:
            ms = np.arange(c.mfirst[t], c.mfirst[t + 1])
            m = int(ms[min(3, len(ms) - 1)])
            for col in zcols:
                _expect(clean, run(variant(c, z=with_nan(c.z, m, col)), **form), c, {t: ("b",)}, [m], what=("z", t, col, form))
            for col in (0, last):
                _expect(clean, run(variant(c, R=with_nan(c.R, m, col)), **form), c, {t: ALL}, [m], what=("R", t, col, form))
            got = run(variant(c, weight=with_nan(c.weight, m)), **form)       # chi2_m is unweighted: it stays
            _expect(clean, got, c, {t: ALL}, [], what=("weight", t, form))
            assert same(got[2], clean[2])
            calls += len(zcols) + 3
            for slot in (bc.touched(kind)[3], UNTOUCHED):                     # the base: that entry alone, touched or not
                hess, chi2, x2 = run(variant(c, base=with_nan(c.base, t, slot)), **form)
                at = t * 496 + slot
                assert np.isnan(hess[t, slot]) and same(np.delete(hess.reshape(-1), at), np.delete(clean[0].reshape(-1), at)), ("base", t, slot, form)
                assert same(chi2, clean[1]) and same(x2, clean[2]), ("base", t, slot, form)
            hess, chi2, x2 = run(variant(c, chi2_base=with_nan(c.chi2_base, t)), **form)
            assert np.isnan(chi2[t]) and same(np.delete(chi2, t), np.delete(clean[1], t)) and same(hess, clean[0]) and same(x2, clean[2]), ("chi2_base", t, form)
            calls += 3
        # a state that several factors share, on the explicit variant: 7 is state i of three factors, 2 is state j of two of them
        xclean = run(x, **form)
        fi, fj = x.pairs()
        for s in (7, 2):
            uses = {f: ("i" if fi[f] == s else "j") for f in range(x.F) if s in (fi[f], fj[f]) and x.counts[f] > 0}
            assert len(uses) >= 2 and len(uses) < (x.counts > 0).sum()
            for part in ("q", "p"):
                hit = {f: DIRTY[(kind, part, role)] for f, role in uses.items() if DIRTY[(kind, part, role)]}
                ms = np.concatenate([np.arange(x.mfirst[f], x.mfirst[f + 1]) for f in hit]).astype(np.int64) if hit else []
                _expect(xclean, run(variant(x, states=with_nan(x.states, s, PART[part])), **form), x, hit, ms, what=("state", s, part, form))
                calls += 1
        unread = x.states.copy()                                              # bg, v, ba of EVERY state (orientation: p too): not read
        unread[:, 4:(16 if kind == 1 else 13)] = np.nan
        got = run(variant(x, states=unread), **form)
        assert all(same(a, b) for a, b in zip(got, xclean)), ("state, not read", form)
        calls += 1
    print("%s: %d calls with NaN in one place each, factors %s" % (bc.KINDS[kind], calls, TARGETS))
    return calls


def nan_calls(kind):
    """What check_nan_locality must return: per form 3 targets x (z classes + R 2 + weight 1 + base 2 + chi2_base 1) + states 4 + unread 1."""
    return 2 * (3 * ((2 if kind == 2 else 1) + 6) + 5)


# ---------------------------------------------------------------------------------------------- exact residuals
def check_identity(run, kind):
    """Every residual exactly +-0.0: chi2_m == 0.0 everywhere, chi2 the bits of chi2_base, column 30 and entry (30, 30) equal to the
    base as numbers (a -0.0 residual must not show).  Returns the metrics against the reference (the caller holds them to its gates)."""
    c = bc.edge_case("identity", kind)
    hess, chi2, x2 = run(c)
    m = bc.metrics(hess, chi2, x2, bc.edge_reference("identity", kind))
    _show("identity, %s, chi2_m max %.3g" % (bc.KINDS[kind], x2.max()), m)
    assert c.M == sum(bc.COUNTS) and (x2 == 0.0).all() and not np.signbit(x2).any()
    assert same(chi2, c.chi2_base)
    col30 = [bc.hslot(a, 30) for a in range(31)]
    assert (hess[:, col30] == c.base[:, col30]).all() and not np.isnan(hess).any()
    assert (hess[c.counts > 0][:, bc.touched(kind)[0]] != c.base[c.counts > 0][:, bc.touched(kind)[0]]).all()     # G did move
    return m


def _negated(c):
    z = c.z.copy()
    z[:, :4] = -z[:, :4]
    return variant(c, z=z)


def check_pi(run, kind):
    """Rotations of exactly pi, qd.w == 0: e_th = 2 vec(qd) as it is, +-2 on one axis -- the reference does not negate at qd.w == 0, so a
    kernel that does is 2 |g| away in g.  z and -z are one rotation but no longer one e: equal G, entry (30, 30), chi2 and chi2_m, and on
    a zero base exactly opposite g -- all of it for the orientation kind, the theta_j rows (15 .. 17) for the pose kind, whose other
    rotation rows of g also hold position terms (-[y x] in the theta_i columns) that do not change sign.  Returns the metrics."""
    c = bc.edge_case("pi", kind)
    hess, chi2, x2 = run(c)
    m = bc.metrics(hess, chi2, x2, bc.edge_reference("pi", kind))
    _show("pi, %s" % bc.KINDS[kind], m)
    assert np.isfinite(hess).all() and np.isfinite(chi2).all() and (x2 > 0).all()
    n_hess, n_chi2, n_x2 = run(_negated(c))
    G = [bc.hslot(a, b) for b in range(30) for a in range(b + 1)]
    assert np.array_equal(n_hess[:, G], hess[:, G]) and np.array_equal(n_hess[:, 495], hess[:, 495])
    assert np.array_equal(n_chi2, chi2) and np.array_equal(n_x2, x2)
    z_hess = run(c, base=False)[0]
    zn_hess = run(_negated(c), base=False)[0]
    flips = [bc.hslot(a, 30) for a in ((0, 1, 2, 15, 16, 17) if kind == 1 else (15, 16, 17))]
    has = c.counts > 0
    print("pi, %s: g on a zero base, z and -z: largest |g(z) + g(-z)| %.3g of |g| %.3g" % (bc.KINDS[kind], np.abs(z_hess[:, flips] + zn_hess[:, flips]).max(),
                                                                                       np.abs(z_hess[:, flips]).max()))
    assert np.array_equal(zn_hess[:, flips], -z_hess[:, flips]) and (z_hess[has][:, flips] != 0).any(1).all()
    return m


def check_scaled(run, kind):
    """z quaternions of norm 0.5, 3 and 1e-150: the product is normalised, so the reference's gates hold; finite everywhere."""
    c = bc.edge_case("scaled", kind)
    got = run(c)
    assert all(np.isfinite(a).all() for a in got)
    m = bc.metrics(*got, bc.edge_reference("scaled", kind))
    _show("scaled, %s" % bc.KINDS[kind], m)
    return m


# ---------------------------------------------------------------------------------------------- weight 0, long folds, position in the grid
def check_weight_zero(run, kind):
    """fma(0, P, acc) and fma(0, chi2_m, chi2) are exact: weight 0 on a measurement gives the hess and chi2 of the call without it (equal
    as numbers: a zero may change its sign), on every measurement of a factor the base; chi2_m does not know the weight."""
    c = bc.case(kind, 9)
    own = c.owner()
    some = np.zeros(c.M, dtype=bool)
    some[[int(c.mfirst[0]), int(c.mfirst[0]) + 9, int(c.mfirst[1]) - 1, int(c.mfirst[3]), int(c.mfirst[5]) + 16]] = True     # first, inner, last; one of two
    for what, drop in (("five measurements", some), ("every measurement of factor 5", own == 5)):
        gated = variant(c, weight=np.where(drop, 0.0, c.weight))
        less = bc.without(c, drop)
        for form in (dict(), dict(inplace=True)):
            full = run(c, **form)
            hess, chi2, x2 = run(gated, **form)
            w_hess, w_chi2, w_x2 = run(less, **form)
            print("%s, weight 0 on %s, %s: hess differs in %d entries, chi2 in %d" % (bc.KINDS[kind], what, form or "out of place", (hess != w_hess).sum(),
                                                                                    (chi2 != w_chi2).sum()))
            assert np.array_equal(hess, w_hess) and np.array_equal(chi2, w_chi2), (what, form)
            assert same(x2, full[2]) and (x2 > 0).all() and same(w_x2, full[2][~drop]), (what, form)
            gone = np.array([drop[own == f].all() for f in range(c.F)])      # (a factor without measurements counts)
            assert np.array_equal(hess[gone], c.base[gone]) and np.array_equal(chi2[gone], c.chi2_base[gone]), (what, form)
            assert not (hess[5] == full[0][5]).all()


def check_long(run, kind):
    """bc.LONG_COUNTS: a fold of 300 measurements on one factor, 33 on another.  Returns the metrics against the reference."""
    c = bc.edge_case("long", kind)
    worst = {}
    for weight, base in ((True, True), (False, False)):
        got = run(c, weight=weight, base=base)
        assert all(np.isfinite(a).all() for a in got)
        for k, v in bc.metrics(*got, bc.edge_reference("long", kind, weight, base)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _show("long, %s" % bc.KINDS[kind], worst)
    return worst


def check_many(run, kind):
    """bc.MANY factors, 257 workgroups: the first nine by themselves, and the factors in reverse order, reproduce the rows, chi2 and
    chi2_m bit for bit, out of place and in place."""
    c = bc.edge_case("many", kind)
    nine = c.head(9)
    mv, order, meas = bc.reversed_case(c)
    for form in (dict(), dict(inplace=True)):
        hess, chi2, x2 = run(c, **form)
        assert all(np.isfinite(a).all() for a in (hess, chi2, x2)) and hess.shape == (bc.MANY, 496)
        o, p, q = run(nine, **form)
        r_hess, r_chi2, r_x2 = run(mv, **form)
        print("many, %s, %s: head(9) equal %s, reversed: rows equal %d of %d, chi2 %d, chi2_m %d of %d"
              % (bc.KINDS[kind], form or "out of place", same(o, hess[:9]) and same(p, chi2[:9]) and same(q, x2[:len(q)]),
                 (bits(r_hess) == bits(hess[order])).all(1).sum(), c.F, (bits(r_chi2) == bits(chi2[order])).sum(), (bits(r_x2) == bits(x2[meas])).sum(), c.M))
        assert same(o, hess[:9]) and same(p, chi2[:9]) and same(q, x2[:len(q)]), form
        assert same(r_hess, hess[order]) and same(r_chi2, chi2[order]) and same(r_x2, x2[meas]), form
