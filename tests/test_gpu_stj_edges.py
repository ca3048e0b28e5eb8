"""GPU: model 2's bias Jacobians after every interval and at query times (cpi_running_stj_batch, cpi_query_stj_batch,
cpi_running_resume_stj_batch, cpi_query_open_batch, cpi_stream_running_stj_batch and the host forms) where the other tests of the
family never go: the tumbling windows of tests/running_cases.py (|w| dt up to ~1.16 rad per interval), so that every wavefront of
windows and of queries mixes lanes on the short polynomial of sincos_fast, on the long one and on the Cody-Waite reduction -- the
wave-uniform ballot of cpi_math.hpp, which no host emulation covers --, base rows on every branch of rot_2_quat / quat_2_Rot and
carried rotations past 90 degrees; window lengths and cuts on and beside cov_body<2>'s pass length.  tests/test_running_cases_cpu.py
keeps the inputs honest.

Reference: the oracle (oracle_py.oracle().trace of the whole window for rows and chains, .run on the cut window for queries), every
row and every query, none left out.  One gate per field and per kind of comparison: 100 x the floor measured on an MI355X (FLOOR
below, each beside the case that sets it; the per-case tables that pytest -s prints are in profiles/stj_edges.md), a floor never
below 2^-53 x max |ref| of the field, a gate never looser than TOL_MEAN / TOL_JAC / TOL_COV.  The row and output arrays are filled
with NaN before every call.  The bit rules are checked for exact equality."""
import numpy as np
import pytest
import torch

from cpi_amd import stream as st
from tests import running_cases as rc
from tests.test_gpu_open_query import CH1, JAC5, _cut_reference, _open_view_is_exact
from tests.test_gpu_open_resume_stj import CHAINS, NT, _rec
from tests.test_gpu_query import ALL_CASES, _case, _layout, _queries, _reference
from tests.test_gpu_running import _ragged_layout
from tests.test_gpu_stj import ALL, CH, JAC7, MEAN, _bits, _dev, _np, _stepped, _trace
from tests.test_gpu_stream_running import _Guarded, _dense, _twice
from tests.tol import FieldTable, field_gates

pytestmark = pytest.mark.gpu
FIELDS = MEAN + JAC7 + ("P",)
FIELDS1 = MEAN + JAC5 + ("P",)
CALL_SIZES = (1, 2, 5, 63, 64, 65, 130)
MORE_CHAINS = [(1,) * NT, (0, CH, 0, 2 * CH + 1, 0)]     # the record round-trips 69 times; no interval at the start, on a pass, at the end

# Largest error against the oracle measured on an MI355X (imu_avg 0 and 1), never below 2^-53 x max |ref| of the field (which sets DT's
# floor everywhere: its error is 0); P: cov_rel_err.  The case that sets each floor is named beside it; profiles/stj_edges.md holds the
# tables per case.
FLOOR = {
    # running rows: tumbling_windows(32, 47) dense ("47"), stj_edge_windows(46) ragged ("46"), tumbling_stream(46, 0.37) ("s46").  The
    # same gates hold row N - 1 against Engine.preintegrate (Jacobians and P: bit-equal in every case; means within 3.55e-15).
    "rows": {"DT": 2.61e-17,        # s46
             "alpha": 3.89e-16, "beta": 4.44e-15, "q": 3.55e-15, "H_a": 4.16e-17, "H_b": 3.33e-16, "O_b": 4.66e-15,        # 47
             "J_q": 2.50e-16, "J_a": 2.78e-17, "J_b": 2.50e-16, "O_a": 4.16e-16,        # 46
             "P": 2.86e-15},        # s46
    # queries: case reduced of tests/test_gpu_query.py, dense or ragged, but for H_a and H_b (case tumbling)
    "query": {"DT": 2.61e-17, "alpha": 2.78e-16, "beta": 3.55e-15, "q": 3.33e-15, "J_q": 2.22e-16, "J_a": 1.73e-17, "J_b": 2.91e-16,
              "H_a": 2.43e-17, "H_b": 2.64e-16, "O_a": 4.16e-16, "O_b": 4.44e-15, "P": 2.88e-15},
    # chains: stj_chain_windows() (8 x 70), with the launch policy's lanes per window (L0) and one lane (L1), dense = ragged; chain
    # (0, CH, 0, 2 CH + 1, 0) for alpha (L0), q, J_q, H_a, H_b and P (L1), (CH + 1, CH - 1, CH + 1) L0 for beta, J_b and O_b,
    # (2 CH + 1, 1, CH - 1) L0 for O_a, the one-shot call L1 for J_a -- all of them in the last third of the window
    "chain": {"DT": 3.89e-17, "alpha": 8.88e-16, "beta": 6.22e-15, "q": 3.18e-15, "J_q": 5.00e-16, "J_a": 6.94e-17, "J_b": 7.22e-16,
              "H_a": 6.94e-17, "H_b": 6.66e-16, "O_a": 1.22e-15, "O_b": 9.77e-15, "P": 2.76e-15},
    # open queries: stj_open_windows(model) (8 x 29 / 8 x 47); the last segment of the cuts (ch - 1, ch + 1) but for q (cut ch / ch - 1),
    # model 1's J_q and H_a (cut ch) and J_b and H_b (cut ch - 1)
    "open1": {"DT": 1.61e-17, "alpha": 4.16e-17, "beta": 8.88e-16, "q": 1.44e-15, "J_q": 8.33e-17, "J_a": 3.47e-18, "J_b": 4.86e-17,
              "H_a": 5.20e-18, "H_b": 6.94e-17, "P": 2.48e-15},
    "open2": {"DT": 2.61e-17, "alpha": 2.50e-16, "beta": 3.55e-15, "q": 3.43e-15, "J_q": 2.22e-16, "J_a": 1.73e-17, "J_b": 3.61e-16,
              "H_a": 2.43e-17, "H_b": 2.78e-16, "O_a": 5.00e-16, "O_b": 5.33e-15, "P": 2.88e-15},
}
GATE = {kind: field_gates(f) for kind, f in FLOOR.items()}


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _nan(eng, lead, want=ALL, model=2, fill=float("nan")):
    """Output arrays of leading shape `lead`, filled: what a call does not write fails every comparison."""
    flat = eng.alloc_outputs(int(np.prod(lead)), tuple(want), model)
    for v in flat.values():
        v.fill_(fill)
    return {k: v.view(tuple(lead) + tuple(v.shape[1:])) for k, v in flat.items()}


def _same(a, b, label):
    assert set(a) == set(b), (label, sorted(a), sorted(b))
    for k in a:
        assert _bits(a[k], b[k]), (label, k)


# ------------------------------------------------------------------------------------------------ 1. running rows
def _running(eng, avg, kn, lin, q, ref, label, ragged=None):
    """cpi_running_stj_batch on dense windows or on their ragged layout (flat, first, count, given): the table against ref, and the
    bit rules -- the twin's mean and P rows, the Jacobians asked for alone, the host form; row N - 1 against Engine.preintegrate."""
    W, N = kn.shape[0], kn.shape[1] - 1
    prm = eng.make_params(2, bool(avg))
    dl, dq = _dev(lin, eng), _dev(q, eng)
    if ragged is None:
        args, hcount = dict(knots=_dev(kn, eng)), None
    else:
        flat, first, count, given = ragged
        args, hcount = dict(knots=_dev(flat, eng), first=_dev(first, eng), count=_dev(given, eng), N=N), torch.from_numpy(count.copy())
    got = _np(eng.preintegrate_running_stj(lin=dl, q_k_lin=dq, params=prm, want=ALL, out=_nan(eng, (W, N)), **args))
    assert set(got) == set(FIELDS + ("P_sym",)) and all(v.shape[:2] == (W, N) for v in got.values())
    t = FieldTable(FIELDS)
    t.add(got, ref, label)
    fin = _np(eng.preintegrate(lin=dl, q_k_lin=dq, params=prm, want=("mean", "jac", "cov"), **args))
    last = FieldTable(FIELDS)
    last.add({k: got[k][:, N - 1] for k in FIELDS}, fin, label + " row N - 1 vs Engine.preintegrate")
    last_bits = all(_bits(got[k][:, N - 1], fin[k]) for k in JAC7)
    twin_want = ("mean", "cov", "cov_sym")
    twin = _np(eng.preintegrate_running(lin=dl, q_k_lin=dq, params=prm, want=twin_want, out=_nan(eng, (W, N), twin_want), **args))
    _same(twin, {k: got[k] for k in twin}, label + " twin")
    only = _np(eng.preintegrate_running_stj(lin=dl, q_k_lin=dq, params=prm, want=("jac",), out=_nan(eng, (W, N), ("jac",)), **args))
    _same(only, {k: got[k] for k in JAC7}, label + " Jacobians alone")
    host = eng.preintegrate_running_stj_host(torch.from_numpy(kn.copy()), torch.from_numpy(lin.copy()), q_k_lin=torch.from_numpy(q.copy()),
                                             params=prm, want=ALL, count=hcount)
    _same({k: v.numpy() for k, v in host.items()}, got, label + " host form")
    return t, last, last_bits


@pytest.mark.parametrize("avg", [0, 1])
def test_running_rows_tumbling_dense(eng, avg):
    kn, lin, q = rc.stj_edge_windows(47)
    ref = _trace(avg, kn, lin, q, key=("tumbling dense", 47))
    t, last, last_bits = _running(eng, avg, kn, lin, q, ref, "dense N47 avg%d" % avg)
    t.report("running stj, tumbling_windows(32, 47) dense, imu_avg %d, vs oracle.trace" % avg, GATE["rows"])
    last.report("row N - 1 vs Engine.preintegrate (Jacobians bit-equal: %s)" % last_bits, GATE["rows"])
    t.check(GATE["rows"], "running stj dense")
    last.check(GATE["rows"], "running stj dense, row N - 1")


@pytest.mark.parametrize("avg", [0, 1])
@pytest.mark.parametrize("N", rc.STJ_EDGE_N)
def test_running_rows_tumbling_edge_lengths_ragged(eng, N, avg):
    """The ragged layout with garbage counts (0, N, 1, N - 1, counts outside [0, N]): rows past the count repeat the final state."""
    kn, lin, q = rc.stj_edge_windows(N)
    flat, first, count, given = _ragged_layout(kn, rc.STJ_LAYOUT_SEED, garbage=True)
    ref = _trace(avg, kn, lin, q, count, key=("tumbling ragged", N))
    t, last, last_bits = _running(eng, avg, kn, lin, q, ref, "ragged N%d avg%d" % (N, avg), (flat, first, count, given))
    t.report("running stj, stj_edge_windows(%d) ragged, imu_avg %d, vs oracle.trace" % (N, avg), GATE["rows"])
    last.report("row N - 1 vs Engine.preintegrate (Jacobians bit-equal: %s)" % last_bits, GATE["rows"])
    t.check(GATE["rows"], "running stj ragged N%d" % N)
    last.check(GATE["rows"], "running stj ragged N%d, row N - 1" % N)


# ------------------------------------------------------------------------------------------------ 2. queries
def _case_rows(eng, name, layout, avg):
    kn, lin, q, _ = _case(name)
    knots, first, count = _layout(name, layout)[:3]
    W, N = ALL_CASES[name]
    prm = eng.make_params(2, bool(avg))
    args = dict(knots=_dev(knots, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng), params=prm, first=_dev(first, eng), count=_dev(count, eng),
                N=None if first is None else N)
    rows = eng.preintegrate_running_stj(args["knots"], args["lin"], args["q_k_lin"], prm, want=ALL, first=args["first"], count=args["count"],
                                        N=args["N"], out=_nan(eng, (W, N)))
    return args, rows


def _ask(eng, args, rows, qw, qt, want=ALL, entry="query_stj", fill=float("nan")):
    return _np(getattr(eng, entry)(args["knots"], args["lin"], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=args["q_k_lin"], params=args["params"],
                                   want=want, first=args["first"], count=args["count"], N=args["N"], out=_nan(eng, (len(qw),), want, fill=fill)))


@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("name", ["n2", "tumbling", "reduced"])
@pytest.mark.parametrize("avg", [0, 1])
def test_queries_n2_and_tumbling(eng, avg, name, layout):
    """Cases n2 and tumbling of tests/test_gpu_query.py and "reduced" (tumbling stays below |w| dt = 1: "reduced" puts queries on the
    Cody-Waite reduction beside gentle ones in every wavefront).  The complete shuffled query list of the case in calls of 1, 2, 5, 63, 64, 65 and 130 queries (the last filled up with
    repeats), everything asked for: every field of every query against the oracle on the cut window; then the bit rules."""
    qw, qt, idx, ref = _reference(name, layout, 2, avg)
    args, rows = _case_rows(eng, name, layout, avg)
    M = len(qw)
    got = {k: np.full(ref[k].shape, np.nan) for k in FIELDS}
    got["P_sym"] = np.full((M, 120), np.nan)
    seen_any = np.zeros(M, dtype=bool)
    rng = np.random.default_rng(3)
    at, c = 0, 0
    while at < M:
        size = CALL_SIZES[c % len(CALL_SIZES)]
        sel = np.arange(at, min(at + size, M))
        sel = np.concatenate([sel, rng.integers(0, M, size - len(sel))])
        out = _ask(eng, args, rows, qw[sel], qt[sel])
        assert set(out) == set(got) and all(v.shape[0] == size for v in out.values())
        seen = seen_any[sel]
        for k in got:
            assert _bits(got[k][sel][seen], out[k][seen]), ("a repeated query gives other bits", k)
            got[k][sel] = out[k]
        seen_any[sel] = True
        at += size
        c += 1
    assert seen_any.all()
    t = FieldTable(FIELDS)
    t.add(got, ref, "%s %s avg%d" % (name, layout, avg))
    stepped = _stepped(name, layout, qw, qt, idx)
    t.report("query stj, case %s %s, imu_avg %d (%d queries, %d with a step), vs the oracle on the cut window" % (name, layout, avg, M, stepped.sum()),
             GATE["query"])
    # no step: the base row bit for bit (zeros for i == 0)
    r = _np(rows)
    for k in JAC7:
        base = r[k][qw, np.maximum(idx - 1, 0)].copy()
        base[idx == 0] = 0.0
        assert np.array_equal(got[k][~stepped], base[~stepped]) and _bits(got[k][~stepped & (idx > 0)], base[~stepped & (idx > 0)]), k
    if stepped.any():
        assert (np.abs(got["J_q"][stepped] - r["J_q"][qw, np.maximum(idx - 1, 0)][stepped]).max(axis=1) > 0).all()
    # one call with the whole list gives the bits of the small calls; a permutation of the queries permutes the outputs
    full = _ask(eng, args, rows, qw, qt)
    _same(full, got, "one call")
    perm = np.random.default_rng(8).permutation(M)
    _same(_ask(eng, args, rows, qw[perm], qt[perm]), {k: v[perm] for k, v in got.items()}, "permutation")
    # the twin's means and P; the Jacobians asked for alone
    twin_want = ("mean", "cov", "cov_sym")
    twin = _ask(eng, args, {k: rows[k] for k in MEAN + ("P",)}, qw, qt, want=twin_want, entry="query")
    _same(twin, {k: got[k] for k in twin}, "Engine.query")
    _same(_ask(eng, args, {k: rows[k] for k in ("q",) + JAC7}, qw, qt, want=("jac",)), {k: got[k] for k in JAC7}, "Jacobians alone")
    # a NaN time: NaN in that query only
    qt_nan = qt.copy()
    holes = sorted({0, 63 % M, 64 % M, M // 2, M - 1})
    qt_nan[holes] = np.nan
    o_n = _ask(eng, args, rows, qw, qt_nan, fill=0.0)
    keep = np.ones(M, dtype=bool)
    keep[holes] = False
    for k in got:
        assert np.isnan(o_n[k][holes]).all() and _bits(o_n[k][keep], got[k][keep]), k
    t.check(GATE["query"], "query stj %s %s" % (name, layout))


# ------------------------------------------------------------------------------------------------ 3. chains
def _seg(eng, kn, lin, q, prm, a, n, carry, layout, want=ALL, entry="preintegrate_running_resume_stj"):
    """Rows [W, max(n, 1), ...] and carry_out of the intervals [a, a + n) continued from carry.  n == 0: one row with count 0 -- the
    read-out of the record (two copies of knot a in the dense layout, so that no other knot can be read)."""
    W, n1 = kn.shape[0], kn.shape[1]
    fn = getattr(eng, entry)
    out = _nan(eng, (W, max(n, 1)), want)
    dl, dq = _dev(lin, eng), _dev(q, eng)
    count = np.full(W, n, dtype=np.int32)
    if layout == "dense":
        knots = kn[:, a:a + n + 1] if n else np.repeat(kn[:, a:a + 1], 2, axis=1)
        return fn(_dev(knots, eng), dl, dq, prm, want=want, carry_in=carry, out=out, count=_dev(count, eng))
    flat = np.concatenate([kn.reshape(-1, 7), kn[-1, -1:]])
    first = np.arange(W, dtype=np.int64) * n1 + a
    return fn(_dev(flat, eng), dl, dq, prm, want=want, first=_dev(first, eng), count=_dev(count, eng), N=max(n, 1), carry_in=carry, out=out)


def _zero_state(ref):
    z = {k: np.zeros_like(v[:, :1]) for k, v in ref.items()}
    z["q"][..., 3] = 1.0
    return z


@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("avg", [0, 1])
def test_chains_under_large_rotations(eng, avg, layout):
    """8 tumbling windows of 3 CH + 1 intervals as the chains of tests/test_gpu_open_resume_stj.py, as 70 segments of one interval
    and with segments of no interval: every row of every segment against the whole-window trace (a segment of no interval against
    the row before it, the zero state at the start); the interchange rules for exact equality; whether the rows are the bits of the
    one-shot call."""
    kn, lin, q = rc.stj_chain_windows()
    W, N = kn.shape[0], kn.shape[1] - 1
    assert N == NT
    ref = _trace(avg, kn, lin, q, key=("tumbling chains", NT))
    dl, dq = _dev(lin, eng), _dev(q, eng)
    t = FieldTable(FIELDS)
    equal = []
    for L in (0, 1):                  # the launch policy's lanes per window, and one lane (whose mean rows do not depend on N)
        prm = eng.make_params(2, bool(avg), lanes_per_window=L)
        one = _np(eng.preintegrate_running_stj(_dev(kn, eng), dl, dq, prm, want=ALL, out=_nan(eng, (W, N))))
        t.add(one, ref, "one-shot L%d" % L)
        for lens in CHAINS + MORE_CHAINS:
            assert sum(lens) == NT
            name = "L%d %s" % (L, lens if len(lens) < 9 else "%d x 1" % len(lens))
            a, carry, parts = 0, None, []
            for si, n in enumerate(lens):
                rows_t, cout = _seg(eng, kn, lin, q, prm, a, n, carry, layout)
                rows = _np(rows_t)
                b = a + n
                label = "%s chain %s segment %d" % (layout, name, si)
                seg_ref = {k: v[:, a:b] for k, v in ref.items()} if n else ({k: v[:, a - 1:a] for k, v in ref.items()} if a else _zero_state(ref))
                t.add(rows, seg_ref, label)
                if n:
                    parts.append(rows)
                if si == 0 and n:
                    closed = _np(eng.preintegrate_running_stj(_dev(kn[:, :b + 1], eng), dl, dq, prm, want=ALL, out=_nan(eng, (W, n))))
                    _same(closed, rows, label + " vs running_stj")
                old_want = ("mean", "cov", "cov_sym")
                old, old_c = _seg(eng, kn, lin, q, prm, a, n, carry, layout, want=old_want, entry="preintegrate_running_resume")
                old = _np(old)
                _same(old, {k: rows[k] for k in old}, label + " vs running_resume")
                assert _bits(_rec(cout), _rec(old_c)), label + " carry vs running_resume"
                if b > 0:
                    fin, _ = eng.preintegrate_resume(_dev(kn[:, b:b + 1], eng), dl, dq, prm, want=("mean", "jac", "cov"), carry_in=cout)
                    fin = _np(fin)
                    _same(fin, {k: rows[k][:, -1] for k in fin}, label + " zero-interval preintegrate_resume")
                a, carry = b, cout
            cat = {k: np.concatenate([p[k] for p in parts], axis=1) for k in one}
            equal.append((name,) + tuple(all(_bits(cat[k], one[k]) for k in ks) for ks in (MEAN, JAC7, ("P", "P_sym"))))
    t.report("running resume stj chains, stj_chain_windows() %s, imu_avg %d, vs oracle.trace of the whole window" % (layout, avg), GATE["chain"])
    print("chain rows bit-equal to the one-shot call (means, Jacobians, P): %s" % "; ".join("%s: %s, %s, %s" % e for e in equal))
    # (not asserted: on the MI355X no chain gives the one-shot call's Jacobian bits -- they follow the covariance rows, which never did;
    # profiles/stj_edges.md -- so the gate is what holds)
    t.check(GATE["chain"], "resume stj chains %s" % layout)


# ------------------------------------------------------------------------------------------------ 4. open queries
@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("model,avg", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_open_view_of_a_closed_tumbling_window_is_exact(eng, model, avg, layout):
    _open_view_is_exact(eng, model, avg, layout, rc.stj_open_windows(model))


_open_cache = {}


def _open_reference(model, avg, b):
    """The query list of tests/test_gpu_query.py over the open windows cut at b intervals, and the oracle on the cut windows."""
    if (model, avg, b) not in _open_cache:
        kn, lin, q = rc.stj_open_windows(model)
        counts = np.full(kn.shape[0], b, dtype=np.int32)
        qw, qt = _queries(kn, counts)
        _open_cache[(model, avg, b)] = (qw, qt, _cut_reference(model, avg, kn, lin, q, qw, qt, counts)[1])
    return _open_cache[(model, avg, b)]


@pytest.mark.parametrize("model,avg", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_chain_then_open_query_under_large_rotations(eng, model, avg):
    """Chains cut at ch - 1, ch, ch + 1 and at (ch - 1, ch + 1): every segment after the first is queried while open, with the rows of
    the segment before it as base, at every time of the list from its first stamp on (times past its end give its last row); all
    fields, P included, against the oracle on the cut window."""
    ch = CH if model == 2 else CH1
    kn, lin, q = rc.stj_open_windows(model)
    W, N = kn.shape[0], kn.shape[1] - 1
    fields = FIELDS if model == 2 else FIELDS1
    prm = eng.make_params(model, bool(avg))
    dl, dq = _dev(lin, eng), (_dev(q, eng) if model == 2 else None)
    t = FieldTable(fields)
    asked = 0
    for cuts in ([0, ch - 1, N], [0, ch, N], [0, ch + 1, N], [0, ch - 1, ch + 1, N]):
        carry = prev = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            seg = _dev(kn[:, a:b + 1], eng)
            rows, cout = eng.preintegrate_running_resume_stj(seg, dl, dq, prm, want=ALL, carry_in=carry, out=_nan(eng, (W, b - a), ALL, model))
            if a:
                qw, qt, ref = _open_reference(model, avg, b)
                keep = qt >= kn[qw, a, 0]
                got = _np(eng.query_open(seg, dl, rows, _dev(qw[keep], eng), _dev(qt[keep], eng), prev, q_k_lin=dq, params=prm, want=ALL,
                                         out=_nan(eng, (int(keep.sum()),), ALL, model)))
                t.add(got, {k: ref[k][keep] for k in fields}, "cuts %s segment [%d, %d)" % (cuts[1:-1], a, b))
                asked += int(keep.sum())
            carry, prev = cout, rows
    kind = "open%d" % model
    t.report("query_open over chains, stj_open_windows(%d), imu_avg %d (%d queries), vs the oracle on the cut window" % (model, avg, asked), GATE[kind])
    t.check(GATE[kind], "query_open model %d" % model)


# ------------------------------------------------------------------------------------------------ 5. the stream route
@pytest.mark.parametrize("avg", [0, 1])
@pytest.mark.parametrize("n,phase", [(23, 0.37), (46, 0.37)])
def test_stream_route_rows(eng, n, phase, avg):
    """The tail interval of a stream window as slot 0 of a pass: cpi_stream_running_stj_batch gives the bits of the ragged route on
    the host-assembled windows (under both sentinels around the stream), and every row matches the oracle."""
    assert (n, phase) in rc.STREAM_CASES
    s, u, lin, q = rc.tumbling_stream(n, phase)
    knots, first, count = st.assemble_windows(s, u)
    U, N = len(u), int(count.max())
    assert N == n + 1 and np.all(count == N)
    ref = _trace(avg, _dense(knots, first, count, N), lin, q, count)
    prm = eng.make_params(2, bool(avg))
    dl, dq = _dev(lin, eng), _dev(q, eng)
    g = _Guarded(eng, s, u)
    label = "stream n%d phase %g avg%d" % (n, phase, avg)

    def call(sentinel):
        g.set(sentinel)
        out, cnt = eng.preintegrate_stream_running_stj(g.s, g.u, dl, q_k_lin=dq, params=prm, want=ALL, N=N, out=_nan(eng, (U, N)), return_counts=True)
        return _np(out), cnt.cpu().numpy()
    got, cnt = _twice(call, label)
    assert np.array_equal(cnt, count), label
    rag = _np(eng.preintegrate_running_stj(_dev(knots, eng), dl, dq, prm, want=ALL, first=_dev(first, eng), count=_dev(count, eng), N=N,
                                           out=_nan(eng, (U, N))))
    _same(got, rag, label + " vs the ragged route")
    t = FieldTable(FIELDS)
    t.add(got, ref, label)
    t.report("stream running stj, tumbling_stream(%d, %g), imu_avg %d, vs oracle.trace" % (n, phase, avg), GATE["rows"])
    t.check(GATE["rows"], label)
