"""GPU: model 2's seven bias Jacobians after every interval and at query times (cpi_running_stj_batch[_host], cpi_query_stj_batch[_host],
Engine.preintegrate_running_stj[_host], Engine.query_stj[_host], cpi_host::CpiBatch::running_stj / at_stj).

References: every running row against oracle_py.oracle().trace (state_transition_jacobians = 1: it returns O_a / O_b after every
feed_IMU) at TOL_JAC and against tests/golden/trace_v2.npz at REG_JAC; every query against the oracle on the cut window [knot 0 ..
knot i, {t_q, w_i, a_i}] (tests/test_gpu_query.py's _reference, as it is) at TOL_JAC.  The bit rules (repeat rows, stamp hits, the
twins' mean and P rows, host forms) are checked for exact equality.  Beside TOL_JAC every Jacobian field has a regression gate of its
own (FLOOR_ROWS / FLOOR_QUERY below).  The largest error of a test is printed (pytest -s).  The same entries under large rotations:
tests/test_gpu_stj_edges.py."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import synth
from oracle import oracle_py as op
from tests.test_gpu_query import CASES, _case, _layout, _queries, _reference
from tests.test_gpu_running import _ragged_layout
from tests.tol import REG_JAC, TOL_FACTOR, TOL_JAC, FieldTable, check_pre, field_gates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = ("DT", "alpha", "beta", "q")
JAC7 = ("J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b")
ALL = ("mean", "jac", "cov", "cov_sym")


def _pass_length():
    """CH of cov_body<2>: the intervals one phase-A pass stages (cpi_cov_kernels.hpp)."""
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_cov_kernels.hpp")).read()
    m = re.search(r"constexpr int CH = \(MODEL == 1\) \? (\d+) : (\d+);", src)
    assert m, "cov_body no longer states its pass length as it did"
    return int(m.group(2))


CH = _pass_length()
RUN_N = sorted({1, CH - 1, CH, CH + 1, 2 * CH + 1})

# Per-field regression gates beside TOL_JAC (tests/tol.py: field_gates): 100 x the largest error against the oracle measured on an
# MI355X over these tests, imu_avg 0 and 1, never below 2^-53 x max |ref| of the field (the tables: profiles/stj_edges.md).
#   rows:    test_running_rows_dense and test_running_rows_ragged, every N of RUN_N; every floor is set at N = 2 CH + 1
#   queries: test_query_parity_and_bit_rules, cases n1 and n13, dense and ragged; every floor is set by n13
FLOOR_ROWS = {"J_q": 2.50e-16, "J_a": 3.47e-17, "J_b": 4.44e-16, "H_a": 2.43e-17, "H_b": 2.50e-16, "O_a": 3.33e-16, "O_b": 3.55e-15}
FLOOR_QUERY = {"J_q": 4.16e-17, "J_a": 2.71e-19, "J_b": 1.73e-17, "H_a": 1.08e-18, "H_b": 4.16e-17, "O_a": 1.04e-17, "O_b": 4.44e-16}


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _dev(a, eng):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _flat(d, keys):
    return {k: d[k].reshape((-1,) + d[k].shape[2:]) for k in keys}


_trace_cache = {}


def _trace(avg, kn, lin, q, count=None, key=None):
    """[W, N, ...] rows of the oracle's model-2 trace, all fields; window w cut at count[w] clamped into [0, N], the rows from there
    on repeat its final state (count 0: the zero state)."""
    if key is not None and (key, avg) in _trace_cache:
        return _trace_cache[(key, avg)]
    W, N = kn.shape[0], kn.shape[1] - 1
    names = MEAN + JAC7 + ("P",)
    ref = {k: np.zeros((W, N) + ((n,) if n > 1 else ())) for k, n in op.OUT_FIELDS if k in names}
    ref["q"][:, :, 3] = 1.0
    prm = op.make_params(2, avg, 1)
    for w in range(W):
        n = N if count is None else min(max(int(count[w]), 0), N)
        if n == 0:
            continue
        tr = op.oracle().trace(prm, kn[w, :n + 1], lin[w], q[w])
        for k in names:
            ref[k][w, :n] = tr[k]
            ref[k][w, n:] = tr[k][n - 1]
    assert all(np.isfinite(v).all() for v in ref.values())
    if key is not None:
        _trace_cache[(key, avg)] = ref
    return ref


def _windows(N):
    """7 seeded windows of N intervals (the batches of 1, 2 and 3 windows are its leading ones)."""
    return tuple(t.numpy() for t in synth.make_windows(7, N, seed=9100 + N, edge_cases=False))


def _check_all(got, ref, label, worst):
    keys = MEAN + JAC7 + ("P",)
    check_pre(_flat(got, keys), _flat(ref, keys), what=("mean", "jac", "cov"), v2=True, label=label)
    for k in JAC7:
        worst[k] = max(worst.get(k, 0.0), float(np.abs(got[k] - ref[k]).max()))


# ------------------------------------------------------------------------------------------------ 1. running rows
@pytest.mark.parametrize("avg", [0, 1])
@pytest.mark.parametrize("N", RUN_N)
def test_running_rows_dense(eng, N, avg):
    """Dense batches of 1, 2 and 3 windows (two windows per wavefront: the last wavefront is half empty at odd W), every row of every
    field against the oracle's trace; the mean and P / P_sym rows are the bits of Engine.preintegrate_running; row N - 1 against
    Engine.preintegrate with state_transition_jacobians at REG_JAC."""
    kn, lin, q = _windows(N)
    ref = _trace(avg, kn, lin, q, key=("dense", N))
    prm = eng.make_params(2, bool(avg))
    worst, last_bits, t = {}, [], FieldTable(JAC7)
    for W in (1, 2, 3):
        a = [_dev(x[:W], eng) for x in (kn, lin, q)]
        got = _np(eng.preintegrate_running_stj(*a, params=prm, want=ALL))
        assert set(got) == set(MEAN + JAC7 + ("P", "P_sym")) and all(v.shape[:2] == (W, N) for v in got.values())
        _check_all(got, {k: v[:W] for k, v in ref.items()}, "stj dense N%d avg%d W%d" % (N, avg, W), worst)
        t.add(got, {k: v[:W] for k, v in ref.items()}, "W%d" % W)
        twin = _np(eng.preintegrate_running(*a, params=prm, want=("mean", "cov", "cov_sym")))
        for k in twin:
            assert _bits(got[k], twin[k]), (W, k)
        only = _np(eng.preintegrate_running_stj(*a, params=prm, want=("jac",)))        # the covariance columns still run
        for k in JAC7:
            assert _bits(only[k], got[k]), (W, k)
        fin = _np(eng.preintegrate(*a, params=prm, want=("mean", "jac", "cov")))
        for k in JAC7:
            e = float(np.abs(got[k][:, N - 1] - fin[k]).max())
            assert e <= REG_JAC, (W, k, e)
        last_bits.append(all(_bits(got[k][:, N - 1], fin[k]) for k in JAC7))
    print("running stj dense N %d avg %d: largest error per field vs oracle.trace: %s; last row bit-equal to Engine.preintegrate (W = 1, 2, 3): %s"
          % (N, avg, ", ".join("%s %.2e" % kv for kv in sorted(worst.items())), last_bits))
    t.report("running stj dense N %d avg %d, per field" % (N, avg), field_gates(FLOOR_ROWS))
    t.check(field_gates(FLOOR_ROWS), "running stj dense N %d avg %d" % (N, avg))


@pytest.mark.parametrize("avg", [0, 1])
@pytest.mark.parametrize("N", RUN_N)
def test_running_rows_ragged(eng, N, avg):
    """Ragged layout over one knot array (shuffled windows, NaN between them): counts 0, N, 1, N - 1 and counts outside [0, N], which
    are clamped; rows past the count repeat the final state bit for bit, a window that integrates nothing is all zeros."""
    kn, lin, q = _windows(N)
    flat, first, count, given = _ragged_layout(kn, 40 + N, garbage=True)
    given = given.copy()
    given[4:7] = [-3, N + 5, 2 ** 30]
    count = np.clip(given, 0, N)
    flat[first[5]:first[5] + N + 1] = kn[5]
    flat[first[6]:first[6] + N + 1] = kn[6]
    ref = _trace(avg, kn, lin, q, count)
    prm = eng.make_params(2, bool(avg))
    args = dict(knots=_dev(flat, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng), params=prm, first=_dev(first, eng), count=_dev(given, eng), N=N)
    got = _np(eng.preintegrate_running_stj(want=ALL, **args))
    worst = {}
    _check_all(got, ref, "stj ragged N%d avg%d" % (N, avg), worst)
    twin = _np(eng.preintegrate_running(want=("mean", "cov", "cov_sym"), **args))
    for k in twin:
        assert _bits(got[k], twin[k]), k
    for w in range(7):
        n = int(count[w])
        for k in JAC7:
            if n == 0:
                assert not got[k][w].any(), (w, k)
            for i in range(max(n, 1), N):
                assert _bits(got[k][w, i], got[k][w, i - 1]), (w, i, k)
    print("running stj ragged N %d avg %d (counts %s): %s" % (N, avg, list(given), ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    t = FieldTable(JAC7)
    t.add(got, ref, "ragged")
    t.report("running stj ragged N %d avg %d, per field" % (N, avg), field_gates(FLOOR_ROWS))
    t.check(field_gates(FLOOR_ROWS), "running stj ragged N %d avg %d" % (N, avg))


def test_running_rows_match_the_golden_trace(eng, golden_dir):
    d = np.load(os.path.join(golden_dir, "trace_v2.npz"))
    kn, lin, q = (_dev(d[k][None], eng) for k in ("knots", "lin", "q_k_lin"))
    got = _np(eng.preintegrate_running_stj(kn, lin, q, eng.make_params(2), want=("jac",)))
    held = [k for k in JAC7 if k in d.files]
    assert held == list(JAC7)
    for k in held:
        e = float(np.abs(got[k][0] - d[k]).max())
        print("running stj vs golden trace_v2 %s err %.2e" % (k, e))
        assert e <= REG_JAC, (k, e)


@pytest.mark.parametrize("avg", [0, 1])
def test_running_skipped_intervals_repeat_rows(eng, avg):
    """dt <= 0 at the first, a middle and the last interval, and at all of them: the Jacobian rows repeat bit for bit (row 0 of a
    window that has integrated nothing: zeros), and still match the oracle."""
    N = CH + 1
    kn = _windows(N)[0][:4].copy()
    lin, q = (x[:4] for x in _windows(N)[1:])
    skipped = [[0], [N // 2], [N - 1], list(range(N))]
    for w, s in enumerate(skipped):
        for i in s:
            kn[w, i + 1:, 0] -= kn[w, i + 1, 0] - kn[w, i, 0]
    ref = _trace(avg, kn, lin, q)
    got = _np(eng.preintegrate_running_stj(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), eng.make_params(2, bool(avg)), want=ALL))
    _check_all(got, ref, "stj skips avg%d" % avg, {})
    for w, s in enumerate(skipped):
        for i in s:
            for k in JAC7:
                if i == 0 or w == 3:
                    assert not got[k][w, i].any(), (w, i, k)
                if i > 0:
                    assert _bits(got[k][w, i], got[k][w, i - 1]), (w, i, k)


# ------------------------------------------------------------------------------------------------ 2. queries
_rows_cache = {}


def _rows(eng, name, layout, avg):
    key = (name, layout, avg)
    if key not in _rows_cache:
        kn, lin, q, _ = _case(name)
        knots, first, count = _layout(name, layout)[:3]
        prm = eng.make_params(2, bool(avg))
        args = dict(knots=_dev(knots, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng), params=prm, first=_dev(first, eng), count=_dev(count, eng),
                    N=None if first is None else CASES[name][1])
        rows = eng.preintegrate_running_stj(args["knots"], args["lin"], args["q_k_lin"], prm, want=ALL, first=args["first"], count=args["count"],
                                            N=args["N"])
        _rows_cache[key] = (args, rows)
    return _rows_cache[key]


def _query(eng, args, rows, qw, qt, want=("jac",), entry="query_stj"):
    return _np(getattr(eng, entry)(args["knots"], args["lin"], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=args["q_k_lin"], params=args["params"],
                                   want=want, first=args["first"], count=args["count"], N=args["N"]))


def _stepped(name, layout, qw, qt, idx):
    kn = _case(name)[0]
    counts = _layout(name, layout)[3]
    return np.array([i < counts[w] and t > kn[w, i, 0] for w, t, i in zip(qw, qt, idx)])


@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("name", ["n1", "n13"])
@pytest.mark.parametrize("avg", [0, 1])
def test_query_parity_and_bit_rules(eng, avg, name, layout):
    """The complete query list of the case (before t_0, on every stamp, 0.37 and 0.999 into every interval -- the first, the middle
    ones and the last --, at and past t_n; the ragged layout holds a window with count = 0; one interval has dt == 0), shuffled, in
    calls of 1, 2, 5 and 130 queries (filled up with repeats): every query against the oracle on the cut window; a query without a
    step is the base row bit for bit (zeros for i == 0); the means and P / P_sym beside the Jacobians are Engine.query's bits."""
    qw, qt, idx, ref = _reference(name, layout, 2, avg)
    args, rows = _rows(eng, name, layout, avg)
    M = len(qw)
    got = {k: np.full((M, 9), np.nan) for k in JAC7}
    rng = np.random.default_rng(3)
    at, c = 0, 0
    while at < M:
        size = (1, 2, 5, 130)[c % 4]
        sel = np.arange(at, min(at + size, M))
        sel = np.concatenate([sel, rng.integers(0, M, size - len(sel))])
        out = _query(eng, args, rows, qw[sel], qt[sel])
        assert set(out) == set(JAC7) and all(v.shape == (size, 9) for v in out.values())
        for k in JAC7:
            seen = ~np.isnan(got[k][sel][:, 0])
            assert _bits(got[k][sel][seen], out[k][seen]), "a repeated query gives other bits"
            got[k][sel] = out[k]
        at += size
        c += 1
    check_pre(got, ref, what=("jac",), v2=True, label="query stj %s %s avg%d" % (name, layout, avg))
    err = {k: float(np.abs(got[k] - ref[k]).max()) for k in JAC7}
    stepped = _stepped(name, layout, qw, qt, idx)
    r = _np(rows)
    for k in JAC7:
        base = r[k][qw, np.maximum(idx - 1, 0)].copy()
        base[idx == 0] = 0.0
        assert np.array_equal(got[k][~stepped], base[~stepped]) and _bits(got[k][~stepped & (idx > 0)], base[~stepped & (idx > 0)]), k
    if stepped.any():
        assert (np.abs(got["J_q"][stepped] - r["J_q"][qw, np.maximum(idx - 1, 0)][stepped]).max(axis=1) > 0).all()
    # everything in one call: the Jacobians do not depend on what else is asked for, the rest is Engine.query's
    full = _query(eng, args, rows, qw, qt, want=ALL)
    twin = _query(eng, args, {k: rows[k] for k in MEAN + ("P",)}, qw, qt, want=("mean", "cov", "cov_sym"), entry="query")
    for k in JAC7:
        assert _bits(full[k], got[k]), k
    for k in twin:
        assert _bits(full[k], twin[k]), k
    # a subset of out; a NaN time
    sub = _query(eng, args, {k: rows[k] for k in ("q",) + JAC7}, qw, qt, want=("jac",))
    assert all(_bits(sub[k], got[k]) for k in JAC7)
    qt_nan = qt.copy()
    holes = [0, M // 2, M - 1]
    qt_nan[holes] = np.nan
    o_n = _query(eng, args, rows, qw, qt_nan)
    keep = np.ones(M, dtype=bool)
    keep[holes] = False
    for k in JAC7:
        assert np.isnan(o_n[k][holes]).all() and _bits(o_n[k][keep], got[k][keep]), k
    print("query stj %s %s avg %d (%d queries, %d stepped): %s" % (name, layout, avg, M, stepped.sum(), ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    t = FieldTable(JAC7)
    t.add(got, ref, "%s %s" % (name, layout))
    t.report("query stj %s %s avg %d, per field" % (name, layout, avg), field_gates(FLOOR_QUERY))
    t.check(field_gates(FLOOR_QUERY), "query stj %s %s avg %d" % (name, layout, avg))


def _raw(eng, entry, prm, W, N, t, rows, out, Q=None, **ch):
    """cpi_query_stj_batch through ctypes; t: dict of device tensors; rows / out: dicts of tensors or None; ch: replaced arguments."""
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    a = dict(prm=C.byref(prm), W=W, N=N, knots=ptr(t["knots"]), first=None, count=None, lin=ptr(t["lin"]), q=ptr(t["q"]),
             rows=None if rows is None else C.byref(eng._outputs_struct(rows)), Q=len(t["qtime"]) if Q is None else Q, qwin=ptr(t["qwin"]),
             qtime=ptr(t["qtime"]), out=None if out is None else C.byref(eng._outputs_struct(out)))
    a.update(ch)
    rc = getattr(eng.lib, entry)(eng.ctx, a["prm"], a["W"], a["N"], a["knots"], a["first"], a["count"], a["lin"], a["q"], a["rows"], a["Q"],
                                 a["qwin"], a["qtime"], a["out"])
    torch.cuda.synchronize()
    return rc, (eng.lib.cpi_last_error(eng.ctx) or b"").decode()


class _Call:
    W, N, Q = 4, 3, 6

    def __init__(self, eng):
        kn, lin, q = (t.to(eng.device) for t in synth.make_windows(self.W, self.N, seed=77, edge_cases=False))
        self.eng, self.prm = eng, eng.make_params(2)
        self.t = dict(knots=kn, lin=lin, q=q, qwin=torch.tensor([0, 3, 1, 2, 2, 0], dtype=torch.int32, device=eng.device),
                      qtime=(kn[[0, 3, 1, 2, 2, 0], [1, 2, 0, 3, 1, 2], 0] + 0.002).contiguous())
        self.rows = {k: v for k, v in eng.preintegrate_running_stj(kn, lin, q, self.prm, want=ALL).items()}
        self.out = eng.alloc_outputs(self.Q, ALL, 2)
        for v in self.out.values():
            v.fill_(-7.0)

    def __call__(self, entry="cpi_query_stj_batch", rows="own", out="own", **ch):
        return _raw(self.eng, entry, ch.pop("prm", self.prm), ch.pop("W", self.W), ch.pop("N", self.N), dict(self.t, **ch.pop("t", {})),
                    self.rows if rows == "own" else rows, self.out if out == "own" else out, Q=ch.pop("Q", self.Q), **ch)


def test_query_refusals_and_empty_calls(eng):
    c = _Call(eng)
    assert c()[0] == 0
    torch.cuda.synchronize()
    assert not any((v == -7.0).any() for v in c.out.values())

    def refused(text, who="cpi_query_stj_batch: ", **ch):
        rc, msg = c(**ch)
        assert rc == 1 and msg.startswith(who) and text in msg, (rc, msg)

    refused("analytic O_a / O_b recursion has no running form", prm=eng.make_params(2, state_transition_jacobians=False))
    refused("model must be 1 or 2 (the Forster comparator", prm=eng.make_params(3))
    for f in ("q",) + JAC7:
        rc, msg = c(rows={k: v for k, v in c.rows.items() if k != f}, out={k: c.out[k] for k in ("J_a", "O_b")})
        assert rc == 1 and "missing: %s" % f in msg and msg.startswith("cpi_query_stj_batch: rows needs q and all seven Jacobian fields"), msg
    rc, msg = c(rows={k: c.rows[k] for k in MEAN}, out={k: c.out[k] for k in ("H_a",)})
    assert rc == 1 and msg.endswith("missing: J_q, J_a, J_b, H_a, H_b, O_a, O_b"), msg
    refused("model 2 needs q_k_lin", t=dict(q=None))
    refused("prm/rows/out is NULL", out=None)
    refused("prm/rows/out is NULL", rows=None)
    refused("qwin/qtime is NULL", t=dict(qwin=None))
    refused("qwin/qtime is NULL", t=dict(qtime=None))
    refused("W is 0", W=0)
    refused("negative size", Q=-1)
    # the Jacobian request needs nothing of the means; without a model-2 Jacobian in out the call is cpi_query_cov_batch
    assert c(rows={k: c.rows[k] for k in ("q",) + JAC7}, out={k: c.out[k] for k in JAC7})[0] == 0
    assert c(rows={k: c.rows[k] for k in MEAN + ("P_sym",)}, out={k: c.out[k] for k in MEAN + ("P", "P_sym")})[0] == 0
    # the old entries still refuse, with their own text; the running entry refuses the analytic recursion and Forster
    rc, msg = c(entry="cpi_query_cov_batch")
    assert rc == 1 and msg.startswith("cpi_query_cov_batch: the Jacobian fields (J_q ... O_b) are not available for model 2"), msg
    from cpi_amd import CpiError
    kn, lin, q = c.t["knots"], c.t["lin"], c.t["q"]
    with pytest.raises(CpiError, match="cpi_running_stj_batch: .*analytic O_a / O_b recursion has no running form"):
        eng.preintegrate_running_stj(kn, lin, q, eng.make_params(2, state_transition_jacobians=False), want=("jac",))
    with pytest.raises(CpiError, match="cpi_running_stj_batch: model must be 1 or 2 \\(the Forster comparator has no running form\\)"):
        eng.preintegrate_running_stj(kn, lin, q, eng.make_params(3), want=("mean",))
    with pytest.raises(CpiError, match="cpi_running_stj_batch: model 2 needs q_k_lin"):
        eng.preintegrate_running_stj(kn, lin, None, eng.make_params(2), want=("jac",))
    with pytest.raises(CpiError, match="cpi_preintegrate_running: the Jacobian fields"):
        eng.preintegrate_running(kn, lin, q, eng.make_params(2), want=("jac",))
    # state_transition_jacobians == 0 without a Jacobian field is the twin's call
    ok = _np(eng.preintegrate_running_stj(kn, lin, q, eng.make_params(2, state_transition_jacobians=False), want=("mean", "cov")))
    tw = _np(eng.preintegrate_running(kn, lin, q, eng.make_params(2, state_transition_jacobians=False), want=("mean", "cov")))
    assert all(_bits(ok[k], tw[k]) for k in tw)
    # model 1 is handled as by the twins
    p1 = eng.make_params(1)
    r1 = eng.preintegrate_running_stj(kn, lin, None, p1, want=("mean", "jac", "cov"))
    t1 = eng.preintegrate_running(kn, lin, None, p1, want=("mean", "jac", "cov"))
    assert all(_bits(a, b) for a, b in zip(_np(r1).values(), _np(t1).values()))
    q1 = _np(eng.query_stj(kn, lin, r1, c.t["qwin"], c.t["qtime"], params=p1, want=("mean", "jac", "cov")))
    u1 = _np(eng.query(kn, lin, t1, c.t["qwin"], c.t["qtime"], params=p1, want=("mean", "jac", "cov")))
    assert set(q1) == set(u1) and all(_bits(q1[k], u1[k]) for k in u1)

    # no-ops: Q == 0 and W == 0 write nothing; N == 0 gives zeros (a NaN time NaN) without reading rows
    c2 = _Call(eng)
    for ch in (dict(Q=0), dict(Q=0, W=0), dict(Q=0, t=dict(qwin=None, qtime=None, knots=None))):
        assert c2(**ch)[0] == 0
    torch.cuda.synchronize()
    assert all((v == -7.0).all() for v in c2.out.values())
    rows0 = eng.alloc_outputs(4, ALL, 2)
    for v in rows0.values():
        v.fill_(-7.0)
    o = eng._outputs_struct(rows0)
    for W, N in ((0, 3), (4, 0)):
        assert eng.lib.cpi_running_stj_batch(eng.ctx, C.byref(c.prm), W, N, C.c_void_p(kn.data_ptr()), None, None, C.c_void_p(lin.data_ptr()),
                                             C.c_void_p(q.data_ptr()), C.byref(o)) == 0
    torch.cuda.synchronize()
    assert all((v == -7.0).all() for v in rows0.values())
    qt = c.t["qtime"].clone()
    qt[4] = float("nan")
    rc, msg = c2(N=0, rows={}, t=dict(knots=kn[:, :1].contiguous(), qtime=qt))
    assert rc == 0, msg
    keep = np.arange(6) != 4
    for k in JAC7:
        v = c2.out[k].cpu().numpy()
        assert not v[keep].any() and np.isnan(v[4]).all(), k


def test_window_index_is_clamped_on_the_device_and_refused_on_the_host(eng):
    from cpi_amd import CpiError
    name = "n13"
    kn, lin, q, _ = _case(name)
    W = CASES[name][0]
    args, rows = _rows(eng, name, "dense", 0)
    qt = kn[[0, 0, W - 1, W - 1], [3, 3, 5, 5], 0] + 0.001
    wild = _query(eng, args, rows, np.array([-5, 0, 99, W - 1], dtype=np.int32), qt)
    for k in JAC7:
        assert _bits(wild[k][0], wild[k][1]) and _bits(wild[k][2], wild[k][3]) and np.abs(wild[k]).max() > 0, k
    for bad in (-1, W):
        with pytest.raises(CpiError, match=r"cpi_query_stj_batch_host: qwin\[1\] = %d is not a window" % bad):
            eng.query_stj_host(torch.from_numpy(kn), torch.from_numpy(lin), torch.tensor([0, bad], dtype=torch.int32), torch.from_numpy(qt[:2].copy()),
                               q_k_lin=torch.from_numpy(q), params=eng.make_params(2), want=("jac",))


# ------------------------------------------------------------------------------------------------ 3. host forms
@pytest.mark.parametrize("avg", [0, 1])
def test_host_forms(eng, avg):
    """cpi_running_stj_batch_host / cpi_query_stj_batch_host: the bits of the device forms (the query's rows hold P_sym, as staged)."""
    name = "n13"
    kn, lin, q, cnt = _case(name)
    qw, qt = _queries(kn, cnt)
    prm = eng.make_params(2, bool(avg))
    d = [_dev(x, eng) for x in (kn, lin, q)]
    rows = eng.preintegrate_running_stj(*d, params=prm, want=("mean", "jac", "cov_sym"), count=_dev(cnt, eng))
    cpu = [torch.from_numpy(x) for x in (kn, lin)]
    hrows = eng.preintegrate_running_stj_host(*cpu, q_k_lin=torch.from_numpy(q), params=prm, want=("mean", "jac", "cov_sym"), count=torch.from_numpy(cnt))
    r = _np(rows)
    assert set(hrows) == set(r) and set(JAC7) <= set(r)
    for k in r:
        assert _bits(hrows[k].numpy(), r[k]), k
    dev = _np(eng.query_stj(d[0], d[1], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=d[2], params=prm, want=ALL, count=_dev(cnt, eng)))
    host = eng.query_stj_host(*cpu, torch.from_numpy(qw), torch.from_numpy(qt), q_k_lin=torch.from_numpy(q), params=prm, want=ALL,
                              count=torch.from_numpy(cnt))
    assert set(host) == set(dev) and set(JAC7) <= set(dev)
    for k in dev:
        assert _bits(host[k].numpy(), dev[k]), k
    one = eng.query_stj_host(*cpu, torch.from_numpy(qw), torch.from_numpy(qt), q_k_lin=torch.from_numpy(q), params=prm, want=("jac",),
                             count=torch.from_numpy(cnt))
    assert all(_bits(one[k].numpy(), dev[k]) for k in JAC7)


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("avg", [0, 1])
def test_model2_factor_at_query_times(eng, avg):
    """8 windows, 3 queries each: query_stj -> sqrt_information on P_sym -> whitened factor_eval (model 2, idx_i = qwin), against the
    same chain fed by Engine.preintegrate on the cut windows: residual and H1 / H2 within TOL_FACTOR."""
    W, N = 8, 13
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=606, edge_cases=False))
    rng = np.random.default_rng(9)
    qw = np.repeat(np.arange(W, dtype=np.int32), 3)
    qi = np.tile(np.array([0, N // 2, N - 1]), W)
    frac = rng.uniform(0.1, 0.9, size=len(qw))
    qt = kn[qw, qi, 0] + frac * (kn[qw, qi + 1, 0] - kn[qw, qi, 0])
    prm = eng.make_params(2, bool(avg))
    d = [_dev(x, eng) for x in (kn, lin, q)]
    rows = eng.preintegrate_running_stj(*d, params=prm, want=("mean", "jac", "cov_sym"))
    meas = eng.query_stj(d[0], d[1], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=d[2], params=prm, want=("mean", "jac", "cov_sym"))
    cut = np.zeros((len(qw), N + 2, 7))
    for k, (w, t, i) in enumerate(zip(qw, qt, qi)):
        cut[k, :i + 1] = kn[w, :i + 1]
        cut[k, i + 1:] = kn[w, i]
        cut[k, i + 1:, 0] = t
    ref = eng.preintegrate(_dev(cut, eng), _dev(lin[qw], eng), _dev(q[qw], eng), params=prm, want=("mean", "jac", "cov_sym"))
    # one state per window (idx_i = qwin) and one predicted-and-perturbed successor per query: make_states draws the states_i
    # first, so the three calls (one per query slot) with one seed share them
    rc = {k: v.cpu() for k, v in ref.items()}
    xi, xjs = None, []
    for s_ in range(3):
        pick = torch.arange(s_, len(qw), 3)
        a, b = synth.make_states(rc["alpha"][pick], rc["beta"][pick], rc["q"][pick], rc["DT"][pick], torch.from_numpy(lin), 2, seed=321)
        assert xi is None or torch.equal(a, xi)
        xi = a
        xjs.append(b)
    states = torch.cat([xi] + xjs).contiguous().to(eng.device)
    idx_i = _dev(qw, eng)
    idx_j = _dev((W + (np.arange(len(qw)) % 3) * W + qw).astype(np.int32), eng)
    lin_f, qk_f = _dev(lin[qw], eng), _dev(q[qw], eng)
    out = {}
    for label, m in (("query", meas), ("cut", ref)):
        R = eng.sqrt_information(m["P_sym"])
        m = {k: v for k, v in m.items() if k != "P_sym"}
        out[label] = _np(eng.factor_eval(2, m, lin_f, qk_f, states, idx_i, idx_j, sqrt_info=R))
        out[label + " plain"] = _np(eng.factor_eval(2, m, lin_f, qk_f, states, idx_i, idx_j))
    assert all(np.isfinite(v).all() for o in out.values() for v in o.values())
    worst = {}
    for kind in ("", " plain"):
        for k in ("err", "H1", "H2"):
            e = float(np.abs(out["query" + kind][k] - out["cut" + kind][k]).max())
            worst[k + kind] = e
            print("model-2 factor at query times avg %d: %s%s max-abs difference %.3e (largest entry %.3g)"
                  % (avg, k, kind or " whitened", e, float(np.abs(out["cut" + kind][k]).max())))
    bad = {k: e for k, e in worst.items() if not e <= TOL_FACTOR}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. C++ facade
def test_query_stj_cpp_facade(eng):
    """tests/cpp/test_query_stj.cpp: cpi_host::CpiBatch::running_stj / at_stj against libcpi_amd.so; the program checks itself."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    W, N = 6, 9
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=31, edge_cases=False))
    count = [9, 1, 4, 9, 6, 2]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_query_stj")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_query_stj.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        with open(os.path.join(tmp, "win.txt"), "w") as f:
            f.write("%d\n" % W)
            for w in range(W):
                f.write("%d\n" % count[w])
                f.write(" ".join("%.17g" % v for v in [*lin[w], *q[w]]) + "\n")
                for s in range(count[w] + 1):
                    f.write(" ".join("%.17g" % v for v in kn[w, s]) + "\n")
        for avg in (0, 1):
            p = subprocess.run([exe, os.path.join(tmp, "win.txt"), str(avg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            print(p.stdout.strip())
            assert p.stdout.splitlines()[-1] == "test_query_stj ok"


# ------------------------------------------------------------------------------------------------ 6. graph
def test_running_stj_then_query_stj_replays_from_a_graph(eng):
    """One capture of cpi_running_stj_batch followed by cpi_query_stj_batch -- a chain on one stream -- replays to the bits of the eager
    calls."""
    kn, lin, q, cnt = (_dev(x, eng) for x in _case("n13"))
    qw_h, qt_h = _queries(_case("n13")[0], _case("n13")[3])
    qw, qt = _dev(qw_h, eng), _dev(qt_h, eng)
    prm = eng.make_params(2, True)
    want_r, want_q = ("mean", "jac", "cov_sym"), ALL
    rows = eng.preintegrate_running_stj(kn, lin, q, prm, want=want_r, count=cnt)
    out = eng.query_stj(kn, lin, rows, qw, qt, q_k_lin=q, params=prm, want=want_q, count=cnt)

    def call():
        eng.preintegrate_running_stj(kn, lin, q, prm, want=want_r, count=cnt, out=rows)
        eng.query_stj(kn, lin, rows, qw, qt, q_k_lin=q, params=prm, want=want_q, count=cnt, out=out)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                          # warm-up on the side stream, as graph capture requires
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for v in list(out.values()) + list(rows.values()):
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], eager[k]), k
