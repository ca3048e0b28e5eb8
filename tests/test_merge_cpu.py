"""CPU: cpi_merge_batch without a GPU -- the mathematics, the kernel's arithmetic, the contract.

1. The NumPy restatement of the composition (tests/merge_cases.py) against ONE sequential integration by the oracle: segments of
   make_windows(64, 40) and (33, 23) preintegrated by the oracle one by one and folded -- 2 segments cut at 1, 14, 17 and N - 1, 8
   equal segments, N segments of one interval, imu_avg 0 and 1.  Gates: TOL_MEAN / TOL_JAC / TOL_COV, and the tighter observed
   facts: means and Jacobians <= 1e-12 (they compose exactly, to rounding), P <= 1e-6 relative at 200 Hz (measured <= 1.4e-8: the
   reference's own RK4 truncation, not an error of the merge).  q is compared after aligning its sign.
   The three mutations of merge_cases.MUTATIONS must each miss a gate: the test would see them.
2. The host simulation of cpi_merge_kernel (tests/hostsim/hostsim_merge.cpp: the kernel's CPI_HD arithmetic, its staging and its
   three exchanges, lanes as loops) against the restatement on the same cases and on ragged first / count (0, 1, > G), a group
   clipped by in_rows, P_sym input.  Bound: 1e-13 absolute on means and Jacobians, 1e-12 relative on P -- two 15 x 15 f64 triple
   products per fold step carry a few ulp each, 40 steps at most; the f64 and longdouble restatements differ by as much.
   The same on HARD operands (merge_cases.hard_rows from the oracle: rates of up to 20 rad/s, joined rotations past 3 rad and every
   branch of rot_2_quat, q negated, q unit only to float32, a zero-state row as operand), on a fold of 40 with uniform and mixed
   counts, on merged rows merged again; the coverage is asserted on the longdouble reference alone, the bounds are the same two.
3. The contract through ctypes: every refusal comes before the context is looked at, so a NULL context shows code and text.
4. Declarations: header, binding, unit table, resource report."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as op
from tests import merge_cases as mc
from tests.tol import TOL_COV, TOL_JAC, TOL_MEAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_merge.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_merge.so")
_HDRS = [os.path.join(ROOT, "cpi_amd", "csrc", f) for f in ("cpi_math.hpp", "cpi_merge_kernels.hpp")]
SHAPES = ((64, 40), (33, 23))
EXACT = 1e-12        # means and Jacobians compose exactly: rounding only
COV_200HZ = 1e-6     # P, relative, at the default rate (measured <= 1.4e-8)
HS_EXACT, HS_COV = 1e-13, 1e-12


def _cuts(N):
    return {"cut1": [1], "cut14": [14], "cut17": [17], "cutN-1": [N - 1],
            "eight": [round(i * N / 8) for i in range(1, 8)], "every": list(range(1, N))}


@pytest.fixture(scope="module")
def cases():
    """(W, N, avg) -> (reference of the whole window, {cut name: list of segment measurements}), computed once."""
    from cpi_amd import synth
    out = {}
    for W, N in SHAPES:
        kn, lin, q = (t.numpy() for t in synth.make_windows(W, N))
        for avg in (0, 1):
            prm = op.make_params(1, avg, 1)
            run = lambda k: {key: v.copy() for key, v in op.oracle().run(prm, np.ascontiguousarray(k), lin, q).items()}
            out[W, N, avg] = (run(kn), {name: [run(s) for s in mc.cut_segments(kn, cuts)] for name, cuts in _cuts(N).items()})
    return out


@pytest.fixture(scope="module")
def hs():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in [_SRC] + _HDRS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB, _SRC])
    lib = C.CDLL(_LIB)
    lib.hsm_merge.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def hs_merge(lib, meas, M, G, first=None, count=None, tri=False, jac=True, cov=True):
    rows = mc.hs_rows(meas)
    out = np.full((M, mc.HS_ROW), np.nan)
    f = None if first is None else np.ascontiguousarray(first, dtype=np.int64)
    c = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
    assert lib.hsm_merge(M, G, rows.shape[0], rows.ctypes.data, int(tri), None if f is None else f.ctypes.data,
                         None if c is None else c.ctypes.data, int(jac), int(cov), out.ctypes.data) == 0
    return mc.hs_meas(out)


def _gate(d, label, mean=TOL_MEAN, jac=TOL_JAC, cov=TOL_COV):
    bad = [(k, e) for k, e in d.items() if not e <= (mean if k in mc.MEAN else cov if k == "P" else jac)]
    assert not bad, (label, bad)


@pytest.mark.parametrize("W,N", SHAPES)
def test_restatement_matches_one_sequential_integration(cases, W, N):
    worst = {}
    for avg in (0, 1):
        ref, segs = cases[W, N, avg]
        for name, parts in segs.items():
            for dtype in (np.float64, np.longdouble):
                d = mc.deviations(mc.fold(parts, dtype), ref)
                _gate(d, (avg, name, dtype.__name__))
                _gate(d, (avg, name, dtype.__name__, "observed"), EXACT, EXACT, COV_200HZ)
                for k, e in d.items():
                    worst[k] = max(worst.get(k, 0.0), e)
    print("merge restatement vs one integration, W %d N %d: %s" % (W, N, ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("mutation,field,tol", (("drop_beta_x_Jq", "J_b", TOL_JAC), ("no_T_on_PB", "P", TOL_COV), ("wrong_sign_theta_bg", "P", TOL_COV)))
def test_a_broken_term_misses_the_gate(cases, mutation, field, tol):
    """The mutation checks of profiles/merge_bench.md: the comparison above would fail with any of the three terms broken."""
    for W, N in SHAPES:
        for avg in (0, 1):
            ref, segs = cases[W, N, avg]
            for name in ("cut14", "eight"):
                d = mc.deviations(mc.fold(segs[name], mutate=mutation), ref)
                assert d[field] > 10 * tol, (mutation, W, N, avg, name, d[field])
                assert all(e <= EXACT for k, e in d.items() if k in mc.MEAN), d


def _stack(parts):
    """segments [S] of batches [W] -> one measurement dict of W * S rows, window-major: row w * S + s."""
    S = len(parts)
    out = {}
    for k in mc.MEAN + mc.JAC + ("P",):
        a = np.stack([np.asarray(p[k]).reshape(np.asarray(p["DT"]).shape[0], -1) for p in parts], axis=1)
        out[k] = a.reshape(a.shape[0] * S, -1)
    out["DT"] = out["DT"].reshape(-1)
    return out


@pytest.mark.parametrize("W,N", SHAPES)
def test_hostsim_matches_the_restatement(cases, hs, W, N):
    worst = {}
    for avg in (0, 1):
        ref, segs = cases[W, N, avg]
        for name, parts in segs.items():
            S = len(parts)
            want = mc.fold(parts, np.longdouble)
            for tri in (False, True):
                got = hs_merge(hs, _stack(parts), W, S, tri=tri)
                d = mc.deviations(got, want)
                _gate(d, (avg, name, tri), HS_EXACT, HS_EXACT, HS_COV)
                _gate(mc.deviations(got, ref), (avg, name, tri, "vs one integration"))
                assert np.array_equal(got["P"].reshape(-1, 15, 15), got["P"].reshape(-1, 15, 15).transpose(0, 2, 1))
                rows, cols = mc.tri_index()
                assert np.array_equal(got["P_sym"], got["P"].reshape(-1, 15, 15)[:, cols, rows])
                for k, e in d.items():
                    worst[k] = max(worst.get(k, 0.0), e)
            assert np.array_equal(hs_merge(hs, _stack(parts), W, S)["P"], hs_merge(hs, _stack(parts), W, S, tri=True)["P"])
    print("hostsim merge vs longdouble restatement, W %d N %d: %s" % (W, N, ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))


def test_hostsim_ragged_groups_clipping_and_corners(cases, hs):
    """first / count with 0, 1, values past G and negative ones, a group clipped by in_rows, first at and past in_rows."""
    ref, segs = cases[33, 23, 1]
    meas = _stack(segs["eight"])                       # 33 windows x 8 segments = 264 rows
    in_rows, G = 264, 8
    first = np.array([0, 8, 8, 17, 256, 260, 263, 264, 300, -5, 40, 41], dtype=np.int64)
    count = np.array([8, 1, 0, 5, 8, 8, 3, 2, 4, 2, 11, -3], dtype=np.int32)
    M = len(first)
    got = hs_merge(hs, meas, M, G, first, count)
    want = mc.merge_ref(meas, M, G, first, count, np.longdouble)
    _gate(mc.deviations(got, want), "ragged", HS_EXACT, HS_EXACT, HS_COV)
    raw = mc.hs_rows(meas)
    out = mc.hs_rows(got)
    for j, row in ((1, 8), (6, 263)):                  # count 1, and clipped to one row: the row itself, bit for bit
        assert np.array_equal(out[j], raw[row]), j
    zero = np.zeros(mc.HS_ROW)
    zero[10] = 1.0
    for j in (2, 7, 8, 11):                            # count 0, first == in_rows, first past in_rows, count < 0: the zero state
        assert np.array_equal(out[j], zero), j
    assert np.array_equal(out[10], mc.hs_rows(hs_merge(hs, meas, M, G, first, np.minimum(count, G)))[10])   # count > G is G
    assert np.array_equal(out[0], mc.hs_rows(hs_merge(hs, meas, 1, G))[0])                                  # dense == ragged
    # the dense layout clipped by in_rows: 34 groups of 8 over 264 rows -> group 33 is empty; 38 groups of 7 -> group 37 has 5 rows
    d7 = hs_merge(hs, meas, 38, 7)
    w7 = mc.merge_ref(meas, 38, 7, dtype=np.longdouble)
    _gate(mc.deviations(d7, w7), "dense clipped", HS_EXACT, HS_EXACT, HS_COV)
    assert np.array_equal(mc.hs_rows(hs_merge(hs, meas, 34, 8))[33], zero)
    # requests: without the covariance / the Jacobians the other fields are bit for bit the same
    full = mc.hs_rows(got)
    nocov = mc.hs_rows({**hs_merge(hs, meas, M, G, first, count, cov=False), "P": got["P"]})
    assert np.array_equal(nocov[:, :56], full[:, :56])
    means = hs_merge(hs, meas, M, G, first, count, jac=False, cov=False)
    for k in mc.MEAN:
        assert np.array_equal(means[k], got[k]), k


# ---------------------------------------------------------------- hard operands: large rotations, odd quaternions, long folds
ULP = 2.0 ** -52
HARD_ROWS = mc.HARD_W * mc.HARD_S


class _Hard:
    """merge_cases.hard_rows from the oracle (model 1, imu_avg), and the longdouble references the tests below share: each is
    computed once and never written to."""
    def __init__(self):
        prm = op.make_params(1, 1, 1)
        self.rows, self.regime, self.long_rows = mc.hard_rows(
            lambda kn, lin: {k: v.copy() for k, v in op.oracle().run(prm, kn.numpy(), lin.numpy()).items()})
        self._refs = {}

    def ref(self, which, M, G, layout):
        """(reference, its folded state, first, count); layout: dense, ragged (hard rows), mixed (the long fold's counts)."""
        key = (which, M, G, layout)
        if key not in self._refs:
            meas = self.rows if which == "rows" else self.long_rows
            first, count = mc.ragged_groups(M, G, HARD_ROWS, 100 * M + G) if layout == "ragged" else (None, None)
            if layout == "mixed":
                count = mc.long_counts()
            self._refs[key] = mc.merge_ref(meas, M, G, first, count, np.longdouble, state=True) + (first, count)
        return self._refs[key]


@pytest.fixture(scope="module")
def hard():
    return _Hard()


def _dense_M(G):
    return -(-HARD_ROWS // G)


def test_hard_rows_reach_every_branch_of_rot_2_quat(hard):
    """What the hard rows are for, asserted on the longdouble reference alone, after the regimes are applied (measured: branches
    r00 / r11 / r22 / w taken 47 / 37 / 58 / 114 times, largest angle 3.12 rad, smallest |w| 1.2e-2; no row is left out below)."""
    want, S, _, _ = hard.ref("rows", mc.HARD_W, mc.HARD_S, "dense")
    taken = np.bincount(mc.branch_of(S["R"]), minlength=4)
    angle = mc.joined_angle(want["q"])
    print("hard rows, G 8: branches %s taken %s times, largest angle %.3f rad, smallest |w| %.2e" % (mc.BRANCHES, taken, angle.max(), np.abs(want["q"][:, 3]).min()))
    assert taken.min() >= 30, taken
    assert angle.max() > 3.0
    assert np.abs(want["q"][:, 3]).min() >= 1e-3
    for G in (2, 3):
        w2, S2, _, _ = hard.ref("rows", _dense_M(G), G, "dense")
        print("hard rows, G %d: branches taken %s times, largest angle %.3f rad" % (G, np.bincount(mc.branch_of(S2["R"]), minlength=4), mc.joined_angle(w2["q"]).max()))
    # the regimes are what they say
    q = hard.rows["q"].reshape(mc.HARD_W, mc.HARD_S, 4)
    off = np.abs((q * q).sum(-1) - 1)
    assert off[hard.regime == 0].max() <= 4 * ULP and (q[hard.regime == 0][:, :, 3] >= 0).all()
    assert (q[hard.regime == 1][:, 1::2, 3] <= 0).all() and (q[hard.regime == 1][:, 0::2, 3] >= 0).all()
    assert 1e-9 < off[hard.regime == 2].max() <= 2.0 ** -22         # four components rounded to 2^-24 relative each
    zero = (hard.rows["DT"].reshape(mc.HARD_W, mc.HARD_S) == 0)
    assert np.array_equal(zero.sum(1), (hard.regime == 3).astype(int)) and set(np.nonzero(zero)[1]) == set(mc.ZERO_AT)
    assert all(np.bincount(hard.regime[4 * i:4 * i + 4], minlength=4).min() == 1 for i in range(mc.HARD_W // 4))   # every wavefront: all four


def _hs_check(got, want, label, label_of=None, names=None):
    d = mc.deviations(got, want)
    print("%s: %s" % (label, ", ".join("%s %.1e" % kv for kv in d.items())))
    if label_of is not None:
        for name, dd in mc.deviations_by(got, want, label_of, names).items():
            print("    %-28s means %.1e  Jacobians %.1e  P %.1e" % ((name,) + mc.worst(dd)))
    _gate(d, label, HS_EXACT, HS_EXACT, HS_COV)
    return d


def _q_is_canonical(q, label):
    q = np.asarray(q, dtype=np.longdouble)
    assert (q[:, 3] >= 0).all(), label
    assert np.abs(np.sqrt((q * q).sum(-1)) - 1).max(initial=0) <= 4 * ULP, label


@pytest.mark.parametrize("G", (2, 3, 8))
def test_hostsim_matches_the_restatement_on_the_hard_rows(hard, hs, G):
    """Every row of every regime is compared; dense (all 2048 rows) and ragged, P read dense and packed."""
    for layout, M in (("dense", _dense_M(G)), ("ragged", 256)):
        want, S, first, count = hard.ref("rows", M, G, layout)
        got = hs_merge(hs, hard.rows, M, G, first, count)
        _hs_check(got, want, "hostsim, hard rows, %s M %d G %d, per regime" % (layout, M, G), mc.group_regime(M, G, first), mc.REGIMES)
        for name, dd in mc.deviations_by(got, want, mc.branch_of(S["R"]), mc.BRANCHES).items():
            print("    branch %-21s means %.1e  Jacobians %.1e  P %.1e" % ((name,) + mc.worst(dd)))
        assert np.array_equal(mc.hs_rows(hs_merge(hs, hard.rows, M, G, first, count, tri=True)), mc.hs_rows(got)), "P_sym input"
        if layout == "dense":
            n = np.minimum(G, HARD_ROWS - np.arange(M) * G)
            _q_is_canonical(got["q"][n > 1], (layout, G))


@pytest.mark.parametrize("layout", ("dense", "mixed"))
def test_hostsim_matches_the_restatement_on_a_fold_of_forty(hard, hs, layout):
    """64 groups of 40 one-interval rows, every count 40 and counts of 0 .. 40.  The bounds are the file's HS_EXACT / HS_COV
    (measured here: means 1.3e-15, Jacobians 2.8e-16, P 2.2e-15 relative)."""
    want, S, first, count = hard.ref("long", mc.LONG_W, mc.LONG_G, layout)
    got = hs_merge(hs, hard.long_rows, mc.LONG_W, mc.LONG_G, first, count)
    _hs_check(got, want, "hostsim, fold of 40, %s" % layout)
    n = np.full(mc.LONG_W, mc.LONG_G) if count is None else count
    _q_is_canonical(got["q"][n > 1], layout)
    assert set(n) >= {0, 1, mc.LONG_G} if layout == "mixed" else True


def _windows(rows, which):
    """the rows of the windows `which` (bool [256]) of the hard rows, window-major."""
    m = np.repeat(which, mc.HARD_S)
    return {k: v[m] for k, v in rows.items()}


def test_float32_quaternions_are_what_the_identity_blocks_are_for(hard, hs):
    """Operands whose q is unit only to float32: the kernel's arithmetic agrees with the restatement whose Phi~ has I, I and DT I in
    its (v,v), (p,p) and (p,v) blocks to the bounds of every other case, and is more than 1e-7 away from the dense triple product
    (R_A^T R_A in those blocks) in P and in P alone: the switch makes the reference valid, no gate was loosened."""
    sub = _windows(hard.rows, hard.regime == 2)
    for G in (2, 8):
        M = 64 * mc.HARD_S // G
        got = hs_merge(hs, sub, M, G)
        _hs_check(got, mc.merge_ref(sub, M, G, dtype=np.longdouble), "hostsim, float32 q, G %d, identity blocks" % G)
        d = mc.deviations(got, mc.merge_ref(sub, M, G, dtype=np.longdouble, identity_blocks=False))
        print("hostsim, float32 q, G %d, dense triple product: P %.1e" % (G, d["P"]))
        assert d.pop("P") > 1e-7
        assert max(d.values()) <= HS_EXACT, d


@pytest.mark.parametrize("W,N", SHAPES)
def test_the_two_forms_of_phi_agree_for_unit_quaternions(cases, W, N):
    """The operands of the existing cases have unit quaternions (to an ulp): R_A^T R_A = I to a few ulp, so the restatement with the
    three blocks set and the dense triple product agree to rounding -- HS_EXACT / HS_COV, as two f64 evaluations of one formula."""
    for avg in (0, 1):
        ref, segs = cases[W, N, avg]
        for name, parts in segs.items():
            d = mc.deviations(mc.fold(parts, identity_blocks=False), mc.fold(parts))
            _gate(d, (avg, name), HS_EXACT, HS_EXACT, HS_COV)
            assert all(d[k] == 0 for k in mc.MEAN + mc.JAC), d


def test_zero_state_operands_and_negated_quaternions(hard, hs):
    """A zero-state row (what count = 0 writes) before or after a row X gives X bit for bit in everything but q, and q within 4 ulp;
    -q is the same operand as q: every output field bit for bit."""
    X = mc.hs_rows(_windows(hard.rows, hard.regime == 0))
    zero = np.zeros_like(X)
    zero[:, 10] = 1.0
    notq = np.r_[0:7, 11:mc.HS_ROW]
    for name, pair in (("zero first", (zero, X)), ("zero second", (X, zero))):
        out = mc.hs_rows(hs_merge(hs, mc.hs_meas(np.stack(pair, 1).reshape(-1, mc.HS_ROW)), X.shape[0], 2))
        assert np.array_equal(out[:, notq], X[:, notq]), name
        assert np.abs(out[:, 7:11] - X[:, 7:11]).max() <= 4 * ULP, name
    flipped = dict(hard.rows)
    flipped["q"] = hard.rows["q"].copy()
    flipped["q"][1::2] *= -1
    for G in (2, 3, 8):
        M = HARD_ROWS // G
        assert np.array_equal(mc.hs_rows(hs_merge(hs, flipped, M, G)), mc.hs_rows(hs_merge(hs, hard.rows, M, G))), G


def test_merged_rows_merge_again(hard, hs):
    """8 -> 4 -> 2 -> 1 rows per window, outputs fed back in, against the flat longdouble fold of 8.  The windows whose operand
    quaternions are unit only to float32 differ from the flat fold by that defect (every pairwise step normalises the q it writes):
    8 x 2^-22 x the largest magnitude for means and Jacobians, four times that for P (tests/test_gpu_merge.py has the reasoning)."""
    level = hard.rows
    for _ in range(3):
        level = hs_merge(hs, level, np.asarray(level["DT"]).shape[0] // 2, 2)
    want = hard.ref("rows", mc.HARD_W, mc.HARD_S, "dense")[0]
    unit = hard.regime != 2
    cut = lambda d, m: {k: np.asarray(v)[m] for k, v in d.items()}
    _hs_check(cut(level, unit), cut(want, unit), "hostsim, three pairwise levels vs the flat longdouble fold, unit q")
    d = mc.deviations(cut(level, ~unit), cut(want, ~unit))
    print("hostsim, three pairwise levels, float32 q: %s" % ", ".join("%s %.1e" % kv for kv in d.items()))
    scale = max(1.0, max(np.abs(want[k][~unit]).max() for k in mc.MEAN + mc.JAC))
    eps = 8 * 2.0 ** -22
    assert all(e <= eps * scale for k, e in d.items() if k != "P") and d["P"] <= 4 * eps, (d, scale)
    assert max(d.values()) > 1e-9
    _q_is_canonical(level["q"], "hierarchy")


@pytest.mark.parametrize("mutation,field", (("drop_beta_x_Jq", "J_b"), ("no_T_on_PB", "P"), ("wrong_sign_theta_bg", "P")))
def test_a_broken_term_misses_the_gate_on_the_hard_rows(hard, hs, mutation, field):
    """The comparison of the hard rows would fail with any of the three terms broken, by a factor 1000 and more over its bound."""
    for G in (2, 8):
        d = mc.deviations(hs_merge(hs, hard.rows, mc.HARD_W, G), mc.merge_ref(hard.rows, mc.HARD_W, G, mutate=mutation))
        print("hostsim, hard rows G %d, %s: %s %.1e" % (G, mutation, field, d[field]))
        assert d[field] > 1e3 * (HS_COV if field == "P" else HS_EXACT), (mutation, G, d[field])
        assert all(e <= HS_EXACT for k, e in d.items() if k in mc.MEAN), d


# ---------------------------------------------------------------- contract, declarations
SYMBOLS = ("cpi_merge_batch", "cpi_merge_batch_host")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def _outputs(*names):
    from cpi_amd._lib import CpiOutputs
    o = CpiOutputs()
    buf = np.zeros(16 * 512)
    for i, n in enumerate(names):
        setattr(o, n, buf.ctypes.data + 8 * 512 * i)   # never dereferenced: the call is refused, or stops at the NULL context
    o._keep = buf
    return o


ALL_IN = ("DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a", "H_b", "P")


@pytest.mark.parametrize("entry", SYMBOLS)
def test_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)

    def call(model=1, M=1, G=2, in_rows=2, in_=ALL_IN, out=("DT", "alpha", "beta", "q"), o=None, i=None):
        i = _outputs(*in_) if i is None else i
        o = _outputs(*out) if o is None else o
        rc = f(None, model, M, G, in_rows, C.byref(i), None, None, C.byref(o))
        return rc, (lib.cpi_last_error(None) or b"").decode()

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    rc, msg = call()
    assert rc == 1 and msg == "ctx is NULL"            # a valid call gets as far as the context
    refused("model must be 1", model=2)
    refused("model must be 1", model=3)
    refused("q_k_lin", model=2)                        # the header's reason
    refused("G (the largest group) must be >= 1", G=0)
    refused("negative size", in_rows=-1)
    refused("negative size", M=-1)
    refused("in must hold DT, alpha, beta and q", in_=("DT", "alpha", "beta"))
    refused("all five Jacobians", in_=("DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a"), out=("J_q",))
    refused("all five Jacobians", in_=("DT", "alpha", "beta", "q", "P"), out=("P",))
    refused("in must hold P or P_sym", in_=ALL_IN[:-1], out=("P_sym",))
    refused("O_a / O_b", out=("DT", "O_a"))
    refused("O_a / O_b", out=("O_b",))
    assert call(in_=ALL_IN[:-1] + ("P_sym",), out=("P",))[1] == "ctx is NULL"          # the packed triangle serves a dense request
    assert call(in_=("DT", "alpha", "beta", "q"))[1] == "ctx is NULL"                  # the means need the means alone
    i = _outputs(*ALL_IN)
    o = _outputs("DT", "alpha", "beta", "q")
    o.alpha = i.alpha + 24                             # out.alpha = row 1 of in.alpha
    refused("overlaps", i=i, o=o)
    o.alpha = i.alpha + 48                             # behind the two input rows: fine
    assert call(i=i, o=o)[1] == "ctx is NULL"
    o.alpha = i.beta                                   # another field of in
    refused("overlaps", i=i, o=o)
    rc = f(None, 1, 1, 2, 2, None, None, None, C.byref(o))
    assert rc == 1 and "in/out is NULL" in (lib.cpi_last_error(None) or b"").decode()


def test_symbols_are_declared_bound_and_exported(lib):
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cpi_amd.h")).read())
    args = ("cpi_ctx *ctx, int32_t model, int64_t M, int32_t G, int64_t in_rows, const cpi_outputs *in, const int64_t *first /*[M] or NULL*/, "
            "const int32_t *count /*[M] or NULL*/, const cpi_outputs *out")
    for s in SYMBOLS:
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int and len(getattr(lib, s).argtypes) == 9
        assert flat.split("int %s(" % s, 1)[1].split(");", 1)[0] == args, s
    assert lib.cpi_abi_version() == 3
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    assert "cpi_merge_batch, cpi_merge_batch_host" in within3
    doc = flat.split("int cpi_merge_batch(")[0].rsplit("/*", 1)[1]
    for text in ("SAME linearisation point", "Model 2 is not composable", "BIT FOR BIT", "zero-state row", "no host synchronisation"):
        assert text in doc, text


def test_kernel_has_a_unit_and_a_report_of_its_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_merge"][-2:] == ["cpi_merge.hip", "cpi_merge_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_merge"]
    assert os.path.basename(own) == "resource_usage_merge.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(">", 1)[1].split()
        rows[ln.rsplit(">", 1)[0] + ">"] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == ["cpi_merge_kernel<%s, %s>" % (j, c) for j in ("false", "true") for c in ("false", "true")]
    for name, (regs, scratch, occ, lds) in rows.items():
        cov = name.endswith("true>")
        assert scratch == 0 and regs <= 512 and occ >= (1 if cov else 2), (name, regs, scratch, occ)
        assert lds == 4 * 8 * (506 if cov else 56), (name, lds)      # what cpi_merge_kernels.hpp says it stages
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_merge_kernel" in open(path).read()) == (unit == "cpi_merge"), path
    src = open(os.path.join(build.CSRC, "cpi_merge_kernels.hpp")).read()
    for helper in ("group_range(", "phi_apply(", "t_apply(", "jac_col_combine("):
        assert re.search(r"CPI_HD \w[\w<> ]* %s" % re.escape(helper), src), helper


def test_engine_and_facade_have_the_entry():
    import inspect
    import cpi_amd
    for fn, sym in ((cpi_amd.Engine.merge, "cpi_merge_batch"), (cpi_amd.Engine.merge_host, "cpi_merge_batch_host")):
        assert sym in inspect.getsource(fn)
        assert list(inspect.signature(fn).parameters)[1:8] == ["meas", "G", "first", "count", "want", "packed", "out"]
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_merge_batch_host(" in src and re.search(r"std::vector<CpiResult> merge\(const Context &ctx", src)
