"""GPU: the measurement at arbitrary times inside a window (cpi_query_batch[_host], Engine.query[_host], cpi_host::CpiBatch::at).

Reference for a query (w, t_q): with n the window's count, t_0 .. t_n its stamps and i the largest index in [0, n] with
t_i <= t_q (0 when t_q < t_0), oracle_py.oracle().run on the dense window [knot 0 .. knot i, {t, w_i, a_i}], t = t_q clipped into
[t_0, t_n] (the entry neither integrates backwards nor extrapolates), padded by repeating that last knot -- dt = 0 intervals are
no-ops.  Every query of every case is compared, none is left out: means and model-1 Jacobians at the contractual gates of
tests/tol.py (TOL_MEAN 1e-9, TOL_JAC 1e-8) and at the regression gates below (100 x the floor measured on an MI355X,
profiles/query_bench.md: 2.66e-13 for the means, 1.94e-14 for the Jacobians).  The largest error per field of a test is printed (pytest -s)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import synth
from oracle import oracle_py as op
from tests import running_cases
from tests.tol import TOL_FACTOR, TOL_JAC, TOL_MEAN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]
MEAN = ("DT", "alpha", "beta", "q")
JAC = ("J_q", "J_a", "J_b", "H_a", "H_b")
CALL_SIZES = (1, 63, 64, 65, 200)     # queries per call: one lane, a wavefront less one, exactly one, one more, several blocks
# name -> (W, N): the bisection runs 1, 2 and 4 trips on the seeded windows, 6 on the tumbling ones (large rotations)
CASES = {"n1": (5, 1), "n2": (5, 2), "n13": (5, 13), "tumbling": (8, 47)}
# + a case for tests/test_gpu_stj_edges.py, not part of the tests below: "tumbling" stays on the polynomials of sincos_fast (largest
# |w| dt 0.96), the windows of "reduced" hold intervals on the Cody-Waite reduction as well, in the ragged layout too
ALL_CASES = dict(CASES, reduced=(8, 47))
TUMBLING_SEED = {"tumbling": 901, "reduced": 947}

# Largest error against the oracle over test_parity (all modes, cases and layouts) measured on an MI355X, per group of fields as
# in tests/tol.py (per field and mode: profiles/query_bench.md): beta of the tumbling windows under model 2 for the means, J_q /
# J_b for the Jacobians.  The regression gate is 100 x the floor, never looser than the contractual gate.
FLOOR = {"mean": 2.66e-15, "jac": 1.94e-16}


def _gate(field):
    contract, group = (TOL_MEAN, "mean") if field in MEAN else (TOL_JAC, "jac")
    return min(contract, 100.0 * FLOOR[group])


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


def _want(model):
    return ("mean", "jac") if model == 1 else ("mean",)


def _fields(model):
    return MEAN + (JAC if model == 1 else ())


_case_cache = {}


def _case(name):
    """Dense windows [W, N + 1, 7] with one dt == 0 interval in window 2, and the counts of the ragged layout (0, 1 and N among
    them)."""
    if name not in _case_cache:
        W, N = ALL_CASES[name]
        if name in TUMBLING_SEED:
            kn, lin, q = running_cases.tumbling_windows(W=W, N=N, seed=TUMBLING_SEED[name])
        else:
            kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=4711 + N, edge_cases=False))
        kn = kn.copy()
        z = min(1, N - 1)
        kn[2, z + 1, 0] = kn[2, z, 0]
        count = np.array([N, 0, N, (N + 1) // 2, 1, N - 1, 13, N][:W], dtype=np.int32).clip(0, N)
        assert np.isfinite(kn).all() and (np.diff(kn[:, :, 0], axis=1) >= 0).all() and 0 in count and N in count
        _case_cache[name] = (kn, lin, q, count)
    return _case_cache[name]


def _layout(name, layout):
    """(knots, first, count, N, counts as the kernel sees them) of a case: "dense" = knots [W, N + 1, 7] and no count; "ragged" =
    one knot array the windows lie in in shuffled order, with gaps of unused knots between them."""
    kn, lin, q, count = _case(name)
    W, N = ALL_CASES[name]
    if layout == "dense":
        return kn, None, None, np.full(W, N, dtype=np.int32)
    rng = np.random.default_rng(17)
    parts, first, at = [], np.zeros(W, dtype=np.int64), 0
    for w in rng.permutation(W):
        gap = rng.normal(size=(int(rng.integers(0, 4)), 7))
        parts += [gap, kn[w, :count[w] + 1]]
        first[w] = at + len(gap)
        at += len(gap) + count[w] + 1
    return np.concatenate(parts), first, count, count


def _queries(kn, counts):
    """Every (window, time) the issue lists: before t_0, t_0, every knot stamp, 0.37 and 0.999 of every interval, t_n, past t_n."""
    qw, qt = [], []
    for w, n in enumerate(counts):
        t = kn[w, :n + 1, 0]
        ts = [t[0] - 0.01, t[0], t[n], t[n] + 0.01] + list(t)
        for f in (0.37, 0.999):
            ts += list(t[:-1] + f * np.diff(t))
        qw += [w] * len(ts)
        qt += ts
    return np.array(qw, dtype=np.int32), np.array(qt)


def _index(kn, counts, qw, qt):
    """i of every query: the largest index in [0, n] with t_i <= t_q, 0 when t_q < t_0."""
    return np.array([max(int(np.searchsorted(kn[w, :counts[w] + 1, 0], t, side="right")) - 1, 0) for w, t in zip(qw, qt)])


_ref_cache = {}


def _reference(name, layout, model, avg):
    """(qwin, qtime, i, reference rows) of the complete query list of a case, in shuffled order."""
    key = (name, layout, model, avg)
    if key not in _ref_cache:
        kn, lin, q, _ = _case(name)
        W, N = ALL_CASES[name]
        counts = _layout(name, layout)[3]
        qw, qt = _queries(kn, counts)
        perm = np.random.default_rng(5).permutation(len(qw))
        qw, qt = qw[perm], qt[perm]
        idx = _index(kn, counts, qw, qt)
        win = np.zeros((len(qw), N + 2, 7))
        for k, (w, t, i) in enumerate(zip(qw, qt, idx)):
            win[k, :i + 1] = kn[w, :i + 1]
            win[k, i + 1:] = kn[w, i]
            win[k, i + 1:, 0] = min(max(t, kn[w, 0, 0]), kn[w, counts[w], 0])
        ref = op.oracle().run(op.make_params(model, avg, 1), win, lin[qw], q[qw])
        assert all(np.isfinite(ref[f]).all() for f in _fields(model))
        _ref_cache[key] = (qw, qt, idx, ref)
    return _ref_cache[key]


def _rows(eng, name, layout, model, avg):
    """The device arguments of a case and its running rows: what cpi_query_batch reads."""
    kn, lin, q, _ = _case(name)
    knots, first, count, N = _layout(name, layout)[:3] + (CASES[name][1],)
    prm = eng.make_params(model, bool(avg))
    args = dict(knots=_dev(knots, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng), params=prm, first=_dev(first, eng), count=_dev(count, eng),
                N=None if first is None else N)
    rows = eng.preintegrate_running(args["knots"], args["lin"], args["q_k_lin"], prm, want=_want(model), first=args["first"],
                                    count=args["count"], N=args["N"])
    return args, rows


def _query(eng, args, rows, qw, qt, model, want=None):
    return _np(eng.query(args["knots"], args["lin"], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=args["q_k_lin"], params=args["params"],
                         want=want or _want(model), first=args["first"], count=args["count"], N=args["N"]))


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _zero_row(field, model):
    n = dict(op.OUT_FIELDS)[field]
    z = np.zeros(n) if n > 1 else np.zeros(())
    if field == "q":
        z[3] = 1.0
    return z


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("model,avg", MODES)
def test_parity(eng, model, avg, name, layout):
    """The complete query list of the case, unsorted, issued in calls of 1, 63, 64, 65 and 200 queries (the last call is filled up
    with repeats of earlier queries): every query against the oracle."""
    qw, qt, idx, ref = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    M = len(qw)
    got = {f: np.full(ref[f].shape, np.nan) for f in _fields(model)}
    rng = np.random.default_rng(3)
    at, c = 0, 0
    while at < M:
        size = CALL_SIZES[c % len(CALL_SIZES)]
        sel = np.arange(at, min(at + size, M))
        sel = np.concatenate([sel, rng.integers(0, M, size - len(sel))])
        out = _query(eng, args, rows, qw[sel], qt[sel], model)
        for f in got:
            assert out[f].shape[0] == size
            prev = got[f][sel]
            seen = ~np.isnan(prev.reshape(size, -1)[:, 0])
            assert _bits(prev[seen], out[f][seen]), "a repeated query gives other bits"
            got[f][sel] = out[f]
        at += size
        c += 1
    err = {f: float(np.abs(got[f] - ref[f]).max()) for f in got}
    print("query parity model %d avg %d %s %s (%d queries): largest error per field: %s"
          % (model, avg, name, layout, M, ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    bad = ["%s %.3e > %.1e" % (f, e, _gate(f)) for f, e in err.items() if not e <= _gate(f)]
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ 2. bit rules
@pytest.mark.parametrize("model,avg", MODES)
def test_bit_rules(eng, model, avg):
    name, layout = "n13", "ragged"
    kn, lin, q, _ = _case(name)
    W, N = CASES[name]
    counts = _layout(name, layout)[3]
    qw, qt, idx, _ = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    out = _query(eng, args, rows, qw, qt, model)
    r = _np(rows)
    copies = zeros = 0
    for k, (w, t, i) in enumerate(zip(qw, qt, idx)):
        n = counts[w]
        if i < n and t > kn[w, i, 0]:
            continue                                           # a partial interval was integrated
        for f in _fields(model):
            want = _zero_row(f, model) if i == 0 else r[f][w, i - 1]     # t_q == t_i (i >= 1), t_q >= t_n; t_q <= t_0, count 0
            assert _bits(out[f][k], want), (f, w, i)
        copies += i > 0
        zeros += i == 0
    assert copies >= 40 and zeros >= 3 * W
    # a permutation of the queries permutes the outputs
    perm = np.random.default_rng(8).permutation(len(qw))
    out_p = _query(eng, args, rows, qw[perm], qt[perm], model)
    for f in _fields(model):
        assert _bits(out_p[f], out[f][perm]), f
    # a NaN time: NaN in every requested field of that query, its neighbours untouched
    qt_nan = qt.copy()
    holes = [0, 63, 64, len(qt) - 1]
    qt_nan[holes] = np.nan
    out_n = _query(eng, args, rows, qw, qt_nan, model)
    keep = np.ones(len(qt), dtype=bool)
    keep[holes] = False
    for f in _fields(model):
        assert np.isnan(out_n[f][holes]).all(), f
        assert _bits(out_n[f][keep], out[f][keep]), f
    # the host form: the same bits (dense knots with counts, as Engine.query_host takes them)
    cnt = _case(name)[3]
    qw_d, qt_d = _queries(kn, cnt)
    prm = eng.make_params(model, bool(avg))
    rows_d = eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=_want(model), count=_dev(cnt, eng))
    dev = _np(eng.query(_dev(kn, eng), _dev(lin, eng), rows_d, _dev(qw_d, eng), _dev(qt_d, eng), q_k_lin=_dev(q, eng), params=prm,
                        want=_want(model), count=_dev(cnt, eng)))
    host = eng.query_host(torch.from_numpy(kn), torch.from_numpy(lin), torch.from_numpy(qw_d), torch.from_numpy(qt_d),
                          q_k_lin=torch.from_numpy(q), params=prm, want=_want(model), count=torch.from_numpy(cnt))
    for f in _fields(model):
        assert _bits(host[f].numpy(), dev[f]), f


# ------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("model,avg", MODES)
def test_predict_at_query_times(eng, model, avg):
    """Engine.predict on the query rows with idx_i = qwin: the states AT the query times, against the oracle's prediction from the
    reference rows."""
    name, layout = "tumbling", "dense"
    _, lin, q, _ = _case(name)
    W = CASES[name][0]
    qw, qt, idx, ref = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    meas = eng.query(args["knots"], args["lin"], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=args["q_k_lin"], params=args["params"])
    rng = np.random.default_rng(12)
    states = rng.normal(size=(W, 16))
    states[:, :4] /= np.linalg.norm(states[:, :4], axis=1, keepdims=True)
    states[:, :4] *= np.sign(states[:, 3:4])
    xj = eng.predict(model, meas, _dev(states, eng), idx_i=_dev(qw, eng))
    torch.cuda.synchronize()
    want = op.oracle().predict(model, op.factor_records(ref, lin[qw], q[qw]), states[qw])
    e = float(np.abs(xj.cpu().numpy() - want).max())
    print("predict at query times model %d avg %d: %.2e" % (model, avg, e))
    assert e <= TOL_FACTOR


# ------------------------------------------------------------------------------------------------ 4. contract
class _Call:
    """Valid arguments of cpi_query_batch on 4 windows of 3 intervals; call(**changes) returns (code, message)."""
    W, N, Q = 4, 3, 6

    def __init__(self, eng, model=1):
        import ctypes as C
        from cpi_amd._lib import CpiOutputs
        self.C, self.eng = C, eng
        kn, lin, q = (t.to(eng.device) for t in synth.make_windows(self.W, self.N, seed=77, edge_cases=False))
        self.prm = eng.make_params(model)
        self.t = dict(knots=kn, lin=lin, q=q, qwin=torch.tensor([0, 3, 1, 2, 2, 0], dtype=torch.int32, device=eng.device),
                      qtime=(kn[[0, 3, 1, 2, 2, 0], [1, 2, 0, 3, 1, 2], 0] + 0.002).contiguous())
        self.rows = eng.preintegrate_running(kn, lin, q, self.prm, want=("mean", "jac") if model == 1 else ("mean",))
        self.out = eng.alloc_outputs(self.Q, ("mean",), model)
        for v in self.out.values():
            v.fill_(-7.0)
        self.ro, self.oo = eng._outputs_struct(self.rows), eng._outputs_struct(self.out)
        self.CpiOutputs = CpiOutputs

    def __call__(self, **ch):
        C = self.C
        a = dict(prm=C.byref(self.prm), W=self.W, N=self.N, knots=self.t["knots"].data_ptr(), first=None, count=None,
                 lin=self.t["lin"].data_ptr(), q=self.t["q"].data_ptr(), rows=C.byref(self.ro), Q=self.Q, qwin=self.t["qwin"].data_ptr(),
                 qtime=self.t["qtime"].data_ptr(), out=C.byref(self.oo))
        a.update(ch)
        rc = self.eng.lib.cpi_query_batch(self.eng.ctx, a["prm"], a["W"], a["N"], a["knots"], a["first"], a["count"], a["lin"], a["q"],
                                          a["rows"], a["Q"], a["qwin"], a["qtime"], a["out"])
        return rc, (self.eng.lib.cpi_last_error(self.eng.ctx) or b"").decode()


def test_refusals(eng):
    import ctypes as C
    c = _Call(eng)
    assert c()[0] == 0
    torch.cuda.synchronize()
    assert not (c.out["DT"] == -7.0).any()

    def refused(text, who="cpi_query_batch: ", **ch):
        rc, msg = c(**ch)
        assert rc == 1 and msg.startswith(who) and text in msg, (rc, msg)

    P = torch.zeros((c.Q, 225), dtype=torch.float64, device=eng.device)
    for f in ("P", "P_sym"):
        o = eng._outputs_struct(dict(c.out, **{f: P}))
        refused("P / P_sym are not available at query times", out=C.byref(o))
    J = torch.zeros((c.Q, 9), dtype=torch.float64, device=eng.device)
    for f in JAC + ("O_a", "O_b"):
        refused("not available for model 2", prm=C.byref(eng.make_params(2)), out=C.byref(eng._outputs_struct(dict(c.out, **{f: J}))))
    refused("model must be 1 or 2 (the Forster comparator", prm=C.byref(eng.make_params(3)))
    refused("model must be 1 or 2", prm=C.byref(eng.make_params(4)))
    refused("model 2 needs q_k_lin", prm=C.byref(eng.make_params(2)), q=None)
    for name in ("prm", "rows", "out"):
        refused("prm/rows/out is NULL", **{name: None})
    for name in ("qwin", "qtime"):
        refused("qwin/qtime is NULL", **{name: None})
    for name in ("knots", "lin"):
        refused("knots/lin is NULL", **{name: None})
    for name in ("W", "N", "Q"):
        refused("negative size", **{name: -1})
    refused("W is 0", W=0)
    refused("N (intervals per window) must be <= 65535", N=65536)
    refused("lanes_per_window must be 0 or one of", who="", prm=C.byref(eng.make_params(1, lanes_per_window=7)))   # the shared check's text
    refused("Q exceeds 2^31 - 1", Q=2 ** 31)
    refused("rows needs DT, alpha, beta and q", rows=C.byref(eng._outputs_struct({k: v for k, v in c.rows.items() if k != "q"})))
    refused("a Jacobian field of out needs the same field of rows", out=C.byref(eng._outputs_struct(dict(c.out, J_a=J))),
            rows=C.byref(eng._outputs_struct({k: v for k, v in c.rows.items() if k != "J_a"})))
    assert c(prm=C.byref(eng.make_params(1, lanes_per_window=12)))[0] == 0        # a supported value is accepted (and ignored)
    assert eng.lib.cpi_query_batch(None, C.byref(c.prm), 1, 1, None, None, None, None, None, C.byref(c.ro), 1, None, None, C.byref(c.oo)) == 1


def test_empty_calls(eng):
    """Q == 0 writes nothing, whatever else is passed; N == 0 gives every query the zero state without reading rows."""
    import ctypes as C
    c = _Call(eng)
    for ch in (dict(Q=0), dict(Q=0, W=0), dict(Q=0, qwin=None, qtime=None, knots=None)):
        assert c(**ch)[0] == 0
    torch.cuda.synchronize()
    assert all((v == -7.0).all() for v in c.out.values())
    for model in (1, 2):
        c = _Call(eng, model)
        out = eng.alloc_outputs(c.Q, ("mean", "jac") if model == 1 else ("mean",), 1)
        for v in out.values():
            v.fill_(-7.0)
        knots0 = c.t["knots"][:, :1].contiguous()                              # dense windows of 0 intervals: [W, 1, 7]
        qtime = c.t["qtime"].clone()
        qtime[4] = float("nan")
        rc, msg = c(N=0, knots=knots0.data_ptr(), rows=C.byref(c.CpiOutputs()), qtime=qtime.data_ptr(), out=C.byref(eng._outputs_struct(out)))
        assert rc == 0, msg
        got = _np(out)
        keep = np.arange(c.Q) != 4
        for f, v in got.items():
            assert _bits(v[keep], np.broadcast_to(_zero_row(f, model), v[keep].shape)), f
            assert np.isnan(v[4]).all(), f


def test_window_index_is_clamped_on_the_device_and_refused_on_the_host(eng):
    name, model, avg = "n13", 1, 0
    kn, lin, q, cnt = _case(name)
    W = CASES[name][0]
    args, rows = _rows(eng, name, "dense", model, avg)
    qt = kn[[0, 0, W - 1, W - 1], [3, 3, 5, 5], 0] + 0.001
    wild = _query(eng, args, rows, np.array([-5, 0, 99, W - 1], dtype=np.int32), qt, model)
    for f in _fields(model):
        assert _bits(wild[f][0], wild[f][1]) and _bits(wild[f][2], wild[f][3]), f
    from cpi_amd import CpiError
    cpu = [torch.from_numpy(x) for x in (kn, lin)]
    for bad in (-1, W):
        with pytest.raises(CpiError, match=r"cpi_query_batch_host: qwin\[1\] = %d is not a window" % bad) as e:
            eng.query_host(*cpu, torch.tensor([0, bad], dtype=torch.int32), torch.from_numpy(qt[:2].copy()), q_k_lin=torch.from_numpy(q))
        assert e.value.code == 1


def test_host_form_checks_the_stamps_of_queried_windows(eng):
    from cpi_amd import CpiError
    kn, lin, q, _ = _case("n13")
    lin_t, q_t = torch.from_numpy(lin), torch.from_numpy(q)
    qtime = torch.from_numpy(kn[[0, 3], [2, 2], 0].copy())
    for value, what in ((kn[3, 4, 0] - 1.0, "decreasing"), (float("nan"), "NaN")):
        bad = kn.copy()
        bad[3, 5, 0] = value
        with pytest.raises(CpiError, match="cpi_query_batch_host: window 3 has a NaN, infinite or decreasing stamp at knot 5") as e:
            eng.query_host(torch.from_numpy(bad), lin_t, torch.tensor([0, 3], dtype=torch.int32), qtime, q_k_lin=q_t)
        assert e.value.code == 1, what
        # a window nobody queries may hold what it likes (a NaN-stamp separator, for instance)
        ok = eng.query_host(torch.from_numpy(bad), lin_t, torch.tensor([0, 1], dtype=torch.int32), qtime, q_k_lin=q_t)
        assert np.isfinite(ok["alpha"].numpy()).all()


def test_running_then_query_replays_from_a_graph(eng):
    """One capture of cpi_preintegrate_running followed by cpi_query_batch -- a chain without parallel branches -- replays to the
    bits of the eager calls, also on new measurements in the same buffers."""
    for model in (1, 2):
        kn, lin, q, cnt = (_dev(x, eng) for x in _case("tumbling"))
        qw_h, qt_h = _queries(_case("tumbling")[0], _case("tumbling")[3])
        qw, qt = _dev(qw_h, eng), _dev(qt_h, eng)
        prm = eng.make_params(model, True)
        rows = eng.preintegrate_running(kn, lin, q, prm, want=_want(model), count=cnt)
        out = eng.query(kn, lin, rows, qw, qt, q_k_lin=q, params=prm, want=_want(model), count=cnt)

        def call():
            eng.preintegrate_running(kn, lin, q, prm, want=_want(model), count=cnt, out=rows)
            eng.query(kn, lin, rows, qw, qt, q_k_lin=q, params=prm, want=_want(model), count=cnt, out=out)
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
        kn[:, :, 1:4] *= 1.01                               # new measurements in the same buffers
        g.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        call()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], replayed[k]), k
        assert not torch.equal(out["alpha"], eager["alpha"])


# ------------------------------------------------------------------------------------------------ 5. C++ facade
@pytest.mark.parametrize("model", [1, 2])
def test_query_cpp_facade(eng, model):
    """tests/cpp/test_query.cpp: cpi_host::CpiBatch::at against libcpi_amd.so; the program checks itself (bit rules against
    CpiBatch::running, parity of the partial intervals against windows of their own, the separator refusal)."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    W, N = 6, 9
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=31, edge_cases=False))
    count = [9, 1, 4, 9, 6, 2]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_query")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_query.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        with open(os.path.join(tmp, "win.txt"), "w") as f:
            f.write("%d\n" % W)
            for w in range(W):
                f.write("%d\n" % count[w])
                f.write(" ".join("%.17g" % v for v in [*lin[w], *q[w]]) + "\n")
                for s in range(count[w] + 1):
                    f.write(" ".join("%.17g" % v for v in kn[w, s]) + "\n")
        for avg in (0, 1):
            p = subprocess.run([exe, os.path.join(tmp, "win.txt"), str(model), str(avg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            print(p.stdout.strip())
            assert p.stdout.splitlines()[-1] == "test_query ok"
