"""What cpi_state_fix_batch must give at the edges of its contract, stated once for the host twin (tests/test_fix_cpu.py) and for the
device (tests/test_gpu_fix_edges.py).  TEST INFRASTRUCTURE ONLY.  Built on tests/fix_cases.py.

Every check takes a function that runs the entry -- run(case) -> (out [S, 136], pcost [S], chi2 [M]) with weight and base given -- and
asserts on what comes back; nothing here knows whether a GPU is behind it.

  check_exact_zero      the identity builder: a residual rotation of exactly +-0.0
  check_broken_mfirst   a broken mfirst is clamped where it is read: padded arrays tell a clamp from its absence without a fault
  check_nan_locality    one NaN in z, R, weight, the state or the base reaches what the contract says and nothing else

What include/cpi_amd.h promises of a NaN is "that state's row and pcost NaN": which entries of the row follows from the table of the
contract.  Lam does not depend on z or on the state (G = R^T R), so a NaN in z or in the state leaves the state's Lam entries as they
were and makes every eta entry of the kind NaN (u_a = sum_{i <= a} R[i][a] wh_i always holds wh_0, and wh_0 every e_k); a NaN in R[0][0]
reaches G_0b and every u_a; a NaN weight reaches every entry the kind touches through fma(w, ., .), and not chi2, which is unweighted."""
import numpy as np

from tests import fix_cases as fx

GUARD = -7.0
PAD = 4                                       # fixes of padding on either side of z, R, weight and chi2
TARGETS = (0, 3, 5)                           # 17 fixes in lane group 0; the last state of its wavefront; 17 fixes in lane group 1
UNTOUCHED = fx.slot(3, 4)                     # an entry of the bg block: no kind touches it
READ = {0: (13,), 1: (7,), 2: (0,), 3: (0, 13)}                     # a column of the state per part a kind reads: p, v, q
UNREAD = {0: (4, 10, 7, 0), 1: (4, 10, 13, 0), 2: (4, 10, 7, 13), 3: (4, 10, 7)}   # both biases, and the parts the kind must not read


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def variant(c, **arrays):
    """The case with some of its arrays replaced (the others shared)."""
    v = fx.Case.__new__(fx.Case)
    v.__dict__.update(c.__dict__)
    v.__dict__.update(arrays)
    return v


def with_nan(a, *index):
    a = np.array(a, dtype=np.float64)
    a[index] = np.nan
    return a


# ---------------------------------------------------------------------------------------------- exact zero
def check_exact_zero(run, kind):
    """The identity builder with a base.  Orientation: chi2 == 0.0 for every fix, pcost the bits of pcost_base, the eta entries 120 ..
    122 equal to the base's as numbers (a -0.0 residual must not show as anything but a zero).  Pose: the rotation rows of eta change
    through R's rotation-position entries alone.  Returns the metrics against the reference (the caller holds them to its gates)."""
    c = fx.edge_case("identity", kind)
    out, pcost, chi2 = run(c)
    m = fx.metrics(out, pcost, chi2, fx.reference(c))
    print("identity, %s: %s; chi2 max %.3g" % (fx.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(m.items())), chi2.max()))
    if kind == 2:
        assert (chi2 == 0.0).all() and c.M == sum(fx.COUNTS)
        assert same(pcost, c.pcost_base)
        assert (out[:, 120:123] == c.base[:, 120:123]).all() and not np.isnan(out).any()
    else:
        assert (chi2 > 0.0).all()
    return m


# ---------------------------------------------------------------------------------------------- broken mfirst
class Padded:
    """z, R, weight and chi2 of a case as interior views of larger arrays, PAD fixes on either side: NaN in the input pads, GUARD in
    the chi2 pad and fill.  A range that leaves [0, M) by up to PAD fixes stays inside the allocations: a missing clamp reads a NaN
    or writes over a guard, and neither is a fault."""

    def __init__(self, c):
        self.c, M = c, c.M
        self.big = {}
        for name, a in (("z", c.z), ("R", c.R), ("weight", c.weight)):
            b = np.full((M + 2 * PAD,) + a.shape[1:], np.nan)
            b[PAD:PAD + M] = a
            self.big[name] = b
        self.big["chi2"] = np.full(M + 2 * PAD, GUARD)


def broken_mfirsts(c):
    """[(what, mfirst, the states whose own two entries are unchanged)] -- every broken value within PAD of [0, M]."""
    S, M, out = c.S, c.M, []
    for what, s, v in (("mfirst[0] = -3", 0, -3), ("mfirst[S] = M + 3", S, M + 3), ("mfirst[3] = mfirst[2] - 1", 3, int(c.mfirst[2]) - 1),
                       ("mfirst[5] = M + 2", 5, M + 2)):
        mf = c.mfirst.copy()
        mf[s] = v
        assert -PAD < v <= M + PAD - 1
        out.append((what, mf, np.array([k for k in range(S) if k != s and k + 1 != s])))
    return out


def check_broken_mfirst(run_padded, kind):
    """run_padded(padded, mfirst) -> (out buffer [S + 2, 136], pcost buffer [S + 2], chi2 buffer [M + 2 PAD]): the WHOLE buffers, the
    entry having been given their interiors (out and pcost NaN-filled between two GUARD rows, chi2 all GUARD).  For each of the four
    breaks: every guard and pad intact; every row of out and every pcost written and finite (everything inside [0, M) is finite, so a
    NaN can only come from outside); every chi2 entry the fill or finite and >= 0; a state whose own two entries are unchanged has
    the bits of the sound call.  Nothing else about the broken states is asserted: their contents are unspecified."""
    c = fx.case(kind, 9)
    p = Padded(c)
    S, M = c.S, c.M
    sound = run_padded(p, c.mfirst)
    for what, mf, keep in [("sound", c.mfirst, np.arange(S))] + broken_mfirsts(c):
        out, pcost, chi2 = run_padded(p, mf)
        x2 = chi2[PAD:PAD + M]
        print("%s, %s: guards out %s pcost %s chi2 %s, finite rows %d of %d, pcost %d of %d, chi2 written %d of %d"
              % (fx.KINDS[kind], what, (out[[0, -1]] == GUARD).all(), (pcost[[0, -1]] == GUARD).all(),
                 (chi2[:PAD] == GUARD).all() and (chi2[PAD + M:] == GUARD).all(), np.isfinite(out[1:-1]).all(1).sum(), S,
                 np.isfinite(pcost[1:-1]).sum(), S, (x2 != GUARD).sum(), M))
        assert (out[[0, -1]] == GUARD).all() and (pcost[[0, -1]] == GUARD).all(), what
        assert (chi2[:PAD] == GUARD).all() and (chi2[PAD + M:] == GUARD).all(), what
        assert np.isfinite(out[1:-1]).all() and np.isfinite(pcost[1:-1]).all(), what
        assert ((x2 == GUARD) | (np.isfinite(x2) & (x2 >= 0))).all(), what
        assert same(out[1:-1][keep], sound[0][1:-1][keep]) and same(pcost[1:-1][keep], sound[1][1:-1][keep]), what
        for name in ("z", "R", "weight"):                                     # the inputs are inputs
            pad = np.concatenate([p.big[name][:PAD], p.big[name][PAD + M:]])
            assert np.isnan(pad).all() and same(p.big[name][PAD:PAD + M], getattr(c, name)), (what, name)


# ---------------------------------------------------------------------------------------------- NaN locality
def _expect(clean, got, c, t, nan_chi2, clean_chi2=None, eta_nan=True, lam="clean", what=""):
    """State t is hit: pcost NaN, every eta entry of the kind NaN; its Lam entries clean ("clean"), NaN ("nan") or either with the
    first one NaN ("some"); untouched entries the base's bits; chi2 NaN exactly at nan_chi2; everything else the clean call's bits."""
    out, pcost, chi2 = got
    lam_slots, eta_slots = fx.touched(c.kind)
    others = np.arange(c.S) != t
    assert same(out[others], clean[0][others]) and same(pcost[others], clean[1][others]), what
    assert np.isnan(pcost[t]) and np.isnan(out[t, eta_slots]).all(), what
    hit = np.isnan(out[t, lam_slots])
    if lam == "clean":
        assert same(out[t, lam_slots], clean[0][t, lam_slots]), what
    elif lam == "nan":
        assert hit.all(), what
    else:
        assert hit[0] and same(out[t, lam_slots][~hit], clean[0][t, lam_slots][~hit]), what
    rest = np.setdiff1d(np.arange(135), lam_slots + eta_slots)
    assert same(out[t, rest], c.base[t, rest]) and out[t, 135] == 0.0, what
    bad = np.zeros(c.M, dtype=bool)
    bad[nan_chi2] = True
    assert np.isnan(chi2[bad]).all() and same(chi2[~bad], clean[2][~bad]), what


def check_nan_locality(run, kind):
    """One NaN, in turn, in every place of the module docstring, for each state of TARGETS; returns the number of calls made."""
    c = fx.case(kind, 9)
    clean = run(c)
    assert all(np.isfinite(a).all() for a in clean)
    calls = 0
    for t in TARGETS:
        fixes = np.arange(c.mfirst[t], c.mfirst[t + 1])
        m = int(fixes[min(3, len(fixes) - 1)])
        for col in ((0, 5) if kind == 3 else (0,)):                           # a z entry of one fix (pose: of q, and of p)
            _expect(clean, run(variant(c, z=with_nan(c.z, m, col))), c, t, [m], what=("z", t, col))
            calls += 1
        _expect(clean, run(variant(c, R=with_nan(c.R, m, 0))), c, t, [m], lam="some", what=("R", t))
        got = run(variant(c, weight=with_nan(c.weight, m)))                   # chi2 is unweighted: it stays
        _expect(clean, got, c, t, [], lam="nan", what=("weight", t))
        assert same(got[2], clean[2])
        calls += 2
        for col in READ[kind]:                                                # a part of the state the kind reads: every fix of it
            _expect(clean, run(variant(c, states=with_nan(c.states, t, col))), c, t, fixes, what=("state", t, col))
            calls += 1
        for col in UNREAD[kind]:                                              # ... and one it must not read: nothing happens
            got = run(variant(c, states=with_nan(c.states, t, col)))
            assert all(same(a, b) for a, b in zip(got, clean)), ("state, not read", t, col)
            calls += 1
        out, pcost, chi2 = run(variant(c, base=with_nan(c.base, t, UNTOUCHED)))
        assert np.isnan(out[t, UNTOUCHED]) and same(np.delete(out.reshape(-1), t * 136 + UNTOUCHED), np.delete(clean[0].reshape(-1), t * 136 + UNTOUCHED))
        assert same(pcost, clean[1]) and same(chi2, clean[2]), ("base", t)
        calls += 1
    print("%s: %d calls with one NaN each, states %s" % (fx.KINDS[kind], calls, TARGETS))
    return calls
