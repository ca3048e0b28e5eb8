"""GPU: the query family by absolute time over IMU stream(s) read in place, and model 2's Jacobian rows from streams
(cpi_query_stream_batch[_host], cpi_stream_running_stj_batch[_host], Engine.query_stream[_host],
Engine.preintegrate_stream[s]_running_stj[_host]).

References.  (a) The window index: numpy's searchsorted(side="left") over the run's update times, clamped to the run's last window.
(b) Bit for bit: Engine.query_stj on the windows the host assembler (cpi_amd/stream.py) cuts from the same stream(s), count clamped
to N, with qwin = the index the call returned and rows from Engine.preintegrate_running_stj on those windows -- the route a caller
had before.  (c) Every query that takes a step against the oracle's cpi_preintegrate_batch equivalent on the cut window
[knot 0 .. knot i, {t_q, w_i, a_i}] at the gates of tests/tol.py.  (d) The rows of the stream entry against
preintegrate_running_stj on the assembled windows, bit for bit.

One stream: 401 readings at 200 Hz, 12 update times -- one before the first reading (a window of 0 intervals), two equal, one exactly
on a stamp, one past the last reading -- at the tight N and at N - 2 (the two longest windows truncated).  The query list holds every
update time, the doubles next above and below each, every stamp of one window, a stream stamp of every window, the midpoint of EVERY
interval of every window, a time before the stream, one past the last update and a NaN; it is longer than 197, so it is asked in
calls of Q = 197 (a partial last wavefront of the mean kernel, a partial last group of the lane-group kernels), the last call filled
up with repeats.  The conditions on the list are asserted on the input."""
import ctypes as C

import numpy as np
import pytest
import torch

from cpi_amd import stream as st
from cpi_amd import synth
from oracle import oracle_py as op
from tests.test_gpu_streams import _lin_q, _pack, _ragged
from tests.tol import check_pre

pytestmark = pytest.mark.gpu
MEAN = ("DT", "alpha", "beta", "q")
JAC5 = ("J_q", "J_a", "J_b", "H_a", "H_b")
JAC7 = JAC5 + ("O_a", "O_b")
ALL = ("mean", "jac", "cov", "cov_sym")
WANTS = [("mean",), ("mean", "jac"), ("mean", "jac", "cov"), ("cov_sym",), ALL]
MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]
Q = 197


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


def lookup(ut, uo, qrun, qt):
    """The window of every query by numpy: searchsorted(side="left") over the run's update times, clamped to its last window; the
    run clamped into [0, R); -1 for a run without update times; a NaN time gives the run's first window."""
    R = len(uo) - 1
    out = np.empty(len(qt), dtype=np.int32)
    for k, t in enumerate(qt):
        r = min(max(int(qrun[k]), 0), R - 1)
        u0, u1 = int(uo[r]), int(uo[r + 1])
        if u1 <= u0:
            out[k] = -1
        elif t != t:
            out[k] = u0
        else:
            out[k] = u0 + min(int(np.searchsorted(ut[u0:u1], t, side="left")), u1 - u0 - 1)
    return out


def classify(knots, first, clamped, qwin, qt):
    """(i, step, on_stamp) of every query on the assembled windows: i = the largest knot index in [0, n] with t_i <= t_q."""
    i = np.zeros(len(qt), dtype=np.int64)
    step = np.zeros(len(qt), dtype=bool)
    on = np.zeros(len(qt), dtype=bool)
    for k, (u, t) in enumerate(zip(qwin, qt)):
        if u < 0 or t != t:
            continue
        n = int(clamped[u])
        ts = knots[first[u]:first[u] + n + 1, 0]
        i[k] = max(int(np.searchsorted(ts, t, side="right")) - 1, 0)
        step[k] = i[k] < n and t > ts[i[k]]
        on[k] = bool((ts == t).any())
    return i, step, on


def oracle_on_cut_windows(model, avg, knots, first, lin, q, qwin, qt, i, sel, N):
    """The oracle's cpi_preintegrate_batch on [knot 0 .. knot i, {t_q, w_i, a_i}] for the queries sel."""
    win = np.zeros((len(sel), N + 2, 7))
    for m, k in enumerate(sel):
        kn = knots[first[qwin[k]]:]
        win[m, :i[k] + 1] = kn[:i[k] + 1]
        win[m, i[k] + 1:] = kn[i[k]]
        win[m, i[k] + 1:, 0] = qt[k]
    return op.oracle().run(op.make_params(model, avg, 1), win, lin[qwin[sel]], q[qwin[sel]])


_single_cache = {}


def _single():
    """stream, update times, assembled windows, lin / q, and the query list of the single-stream tests."""
    if _single_cache:
        return _single_cache
    s = synth.make_stream(10, 40, seed=4242)[0].numpy().copy()
    t = s[:, 0].copy()
    assert len(s) == 401
    ut = np.array([t[0] - 0.5, t[37] + 0.002, t[80] + 0.0013, t[80] + 0.0013, t[120], t[150] + 0.0021, t[190] + 0.004, t[199] + 0.001,
                   t[235] + 0.0015, t[270] + 0.003, t[335] + 0.002, t[400] + 0.7])
    knots, first, count = st.assemble_windows(s, ut)
    assert count[0] == 0 and count[3] == 0 and count[4] == 40 and knots[first[4] + 40, 0] == t[120] and count[7] == 10
    assert sorted(count)[-2:] == [66, 66]
    # rotation well outside the small-angle branch of the closed forms (|w| dt above the reference's 0.008726646 rad/s threshold)
    assert np.median(np.linalg.norm(s[:, 1:4], axis=1)) > 0.1
    qt = list(ut) + list(np.nextafter(ut, np.inf)) + list(np.nextafter(ut, -np.inf))
    qt += list(knots[first[7]:first[7] + count[7] + 1, 0])                         # every stamp of one window
    for u in range(len(ut)):
        if count[u] > 0:
            ts = knots[first[u]:first[u] + count[u] + 1, 0]
            qt += [ts[1]] + list(0.5 * (ts[:-1] + ts[1:]))                             # a stream stamp and every interval's midpoint
    qt += [t[0] - 1.0, ut[-1] + 1.0, float("nan")]
    qt = np.array(qt)
    qt = qt[np.random.default_rng(11).permutation(len(qt))]
    lin, q = _lin_q(len(ut), 5)
    _single_cache.update(stream=s, ut=ut, knots=knots, first=first, count=count, lin=lin, q=q, qt=qt)
    return _single_cache


def _chunks(M):
    """Index sets of Q = 197 queries covering [0, M), the last one filled up with repeats."""
    pad = (-M) % Q
    idx = np.concatenate([np.arange(M), np.arange(pad) % M])
    return idx.reshape(-1, Q)


def _assembled_route(eng, d, prm, N, want_rows):
    """Device arguments of the host-assembled windows and their running rows (preintegrate_running_stj)."""
    clamped = np.minimum(d["count"], N).astype(np.int32)
    a = dict(knots=_dev(d["knots"], eng), lin=_dev(d["lin"], eng), q=_dev(d["q"], eng), first=_dev(d["first"], eng), count=_dev(clamped, eng))
    rows = eng.preintegrate_running_stj(a["knots"], a["lin"], a["q"], prm, want=want_rows, first=a["first"], count=a["count"], N=N)
    return a, rows, clamped


@pytest.mark.parametrize("trunc", [0, 2], ids=["tight", "truncated"])
@pytest.mark.parametrize("mode", MODES, ids=["m%d-avg%d" % m for m in MODES])
def test_single_stream(eng, mode, trunc):
    """(a), (b), (c), (d) on one stream, every want, at the tight N and at N - 2."""
    model, avg = mode
    d = _single()
    ut, qt, knots, first, count = d["ut"], d["qt"], d["knots"], d["first"], d["count"]
    U, M = len(ut), len(qt)
    N = int(count.max()) - trunc
    prm = eng.make_params(model, bool(avg))
    want_rows = ("mean", "jac", "cov")
    a, rows_ref, clamped = _assembled_route(eng, d, prm, N, want_rows)
    ds, du = _dev(d["stream"], eng), _dev(ut, eng)

    # ---- (d) the rows of the stream entry
    rows, cnt = eng.preintegrate_stream_running_stj(ds, du, a["lin"], q_k_lin=a["q"], params=prm, want=want_rows, N=N,
                                                    return_counts=True, check_counts=False)
    assert np.array_equal(cnt.cpu().numpy(), count)
    rr, rs = _np(rows_ref), _np(rows)
    assert sorted(rr) == sorted(rs) and set(rs) >= set(MEAN + (JAC7 if model == 2 else JAC5) + ("P",))
    for k in rr:
        assert _bits(rs[k], rr[k]), ("stream_running_stj rows", k)

    # ---- the conditions on the query list, on the input
    qwin_np = lookup(ut, [0, U], np.zeros(M, dtype=np.int32), qt)
    i, step, on = classify(knots, first, clamped, qwin_np, qt)
    assert M > Q and step.sum() * 4 >= M
    for u in range(U):
        if count[u] > 0:
            assert (step & (qwin_np == u)).any() and (on & (qwin_np == u)).any(), u
    if trunc:
        tN = {u: knots[first[u] + N, 0] for u in range(U) if count[u] > N}
        assert len(tN) >= 2 and any(qwin_np[k] in tN and qt[k] > tN[qwin_np[k]] for k in range(M))

    # ---- (a), (b) for every want, in calls of Q = 197
    dq = _dev(qt, eng)
    full = None
    for want in WANTS:
        got = None
        for sel in _chunks(M):
            sel_t = torch.from_numpy(sel).to(eng.device)
            out, qwin = eng.query_stream(ds, du, a["lin"], rows, dq[sel_t].contiguous(), q_k_lin=a["q"], params=prm, want=want, N=N)
            assert np.array_equal(qwin.cpu().numpy(), qwin_np[sel]), want
            ref = eng.query_stj(a["knots"], a["lin"], rows_ref, qwin, dq[sel_t].contiguous(), q_k_lin=a["q"], params=prm, want=want,
                                first=a["first"], count=a["count"], N=N)
            out, ref = _np(out), _np(ref)
            assert sorted(out) == sorted(ref) and len(out) > 0
            for k in out:
                assert out[k].shape[0] == Q and _bits(out[k], ref[k]), (want, k)
            if got is None:
                got = {k: np.full((M,) + v.shape[1:], np.nan) for k, v in out.items()}
            for k in out:
                got[k][sel] = out[k]
        if want == ALL:
            full = got
    nan_q = np.flatnonzero(qt != qt)
    for k in full:
        assert np.isnan(full[k][nan_q]).all() and np.isfinite(np.delete(full[k], nan_q, axis=0)).all(), k

    # ---- (c) every stepped query against the oracle on its cut window
    sel = np.flatnonzero(step)
    ref = oracle_on_cut_windows(model, avg, knots, first, d["lin"], d["q"], qwin_np, qt, i, sel, N)
    check_pre({k: v[sel] for k, v in full.items()}, ref, what=("mean", "jac", "cov"), v2=model == 2,
              label="query_stream m%d avg%d N%d" % (model, avg, N))
    err = {k: float(np.abs(full[k][sel] - ref[k]).max()) for k in full if k != "P_sym"}
    print("query_stream model %d avg %d N %d: %d queries, %d stepped; max-abs vs the oracle: %s"
          % (model, avg, N, M, len(sel), ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))


_RUNS = None


def _runs():
    """Four runs, every clock starting at 0: a normal one, one of 2 readings, one without readings, one without update times."""
    global _RUNS
    if _RUNS is None:
        def run(W, n, seed, phase):
            s, u, _, _ = synth.make_stream(W, n, seed=seed, phase=phase)
            s, u = s.numpy().copy(), u.numpy().copy()
            u -= s[0, 0]
            s[:, 0] -= s[0, 0]
            return s, u
        a = run(5, 9, 71, 0.37)
        b = run(1, 1, 72, 0.0)
        b = (b[0], np.array([0.5 * b[0][1, 0], b[0][1, 0] + 0.002]))
        c = (np.zeros((0, 7)), np.array([0.01, 0.02]))
        e = (run(3, 7, 73, 0.5)[0], np.zeros(0))
        _RUNS = [a, b, c, e]
    return _RUNS


def _multi():
    runs = _runs()
    stream, so, ut, uo = _pack(runs)
    knots, first, count = _ragged(runs)
    qrun, qt = [], []
    for r, (s, u) in enumerate(runs):
        ts = list(u) + list(np.nextafter(u, np.inf)) + [-1.0, 1e3, float("nan")]
        if len(s) > 1:
            ts += list(0.5 * (s[:-1, 0] + s[1:, 0])) + list(s[:, 0])
        qrun += [r] * len(ts)
        qt += ts
    # out of range on either side: clamped to run 0 and to run R - 1 (which has no update times)
    qrun += [-3, len(runs) + 5, -3]
    qt += [runs[0][1][1], 0.1, runs[0][0][7, 0] + 0.001]
    return stream, so, ut, uo, knots, first, count, np.array(qrun, dtype=np.int32), np.array(qt)


@pytest.mark.parametrize("mode", [(1, 0), (2, 1)], ids=["m1-avg0", "m2-avg1"])
def test_many_streams(eng, mode):
    """R = 4 with every run's clock at 0: rows (d), window index (a), bits (b) and the oracle (c); -1 and NaN for the run without
    update times; qrun out of range is clamped."""
    model, avg = mode
    stream, so, ut, uo, knots, first, count, qrun, qt = _multi()
    U, M, N = len(ut), len(qt), int(count.max())
    lin, q = _lin_q(U, 8)
    prm = eng.make_params(model, bool(avg))
    d = dict(knots=knots, first=first, count=count, lin=lin, q=q)
    a, rows_ref, clamped = _assembled_route(eng, d, prm, N, ("mean", "jac", "cov"))
    ds, du, dso, duo = _dev(stream, eng), _dev(ut, eng), _dev(so, eng), _dev(uo, eng)
    rows = eng.preintegrate_streams_running_stj(ds, dso, du, duo, a["lin"], q_k_lin=a["q"], params=prm, want=("mean", "jac", "cov"), N=N)
    rr, rs = _np(rows_ref), _np(rows)
    for k in rr:
        assert _bits(rs[k], rr[k]), ("stream_running_stj rows, 4 runs", k)
    qwin_np = lookup(ut, uo, qrun, qt)
    none = qwin_np < 0
    assert none.sum() >= 5 and (qwin_np[-3] == 1) and none[-2] and (qrun[none] >= 3).all()
    out, qwin = eng.query_stream(ds, du, a["lin"], rows, _dev(qt, eng), q_k_lin=a["q"], params=prm, want=ALL, N=N,
                                 stream_offsets=dso, update_offsets=duo, qrun=_dev(qrun, eng))
    assert np.array_equal(qwin.cpu().numpy(), qwin_np)
    ref = eng.query_stj(a["knots"], a["lin"], rows_ref, qwin, _dev(qt, eng), q_k_lin=a["q"], params=prm, want=ALL, first=a["first"],
                        count=a["count"], N=N)
    out, ref = _np(out), _np(ref)
    for k in out:
        assert np.isnan(out[k][none]).all(), k
        assert _bits(out[k][~none], ref[k][~none]), k
    i, step, _ = classify(knots, first, clamped, qwin_np, qt)
    sel = np.flatnonzero(step)
    assert len(sel) * 4 >= M and {0, 1} <= set(qrun[sel])
    oref = oracle_on_cut_windows(model, avg, knots, first, lin, q, qwin_np, qt, i, sel, N)
    check_pre({k: v[sel] for k, v in out.items()}, oref, what=("mean", "jac", "cov"), v2=model == 2, label="query_stream 4 runs m%d" % model)


def _raw_args(eng, prm, t, rows, out, **ch):
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    a = dict(prm=C.byref(prm), R=1, K=t["stream"].shape[0], stream=ptr(t["stream"]), soff=None, U=t["ut"].shape[0], ut=ptr(t["ut"]), uoff=None,
             N=t["N"], lin=ptr(t["lin"]), q=ptr(t["q"]), ws=ptr(t["ws"]), rows=None if rows is None else C.byref(eng._outputs_struct(rows)),
             Q=t["qt"].shape[0], qrun=None, qt=ptr(t["qt"]), qwin=ptr(t["qwin"]), out=None if out is None else C.byref(eng._outputs_struct(out)))
    a.update(ch)
    return a


def test_refusals(eng):
    """(e) every refusal with its text; nothing is written by a refused call."""
    d = _single()
    N = int(d["count"].max())
    U = len(d["ut"])
    p1, p2, p3 = eng.make_params(1), eng.make_params(2), eng.make_params(3)
    p2a = eng.make_params(2, state_transition_jacobians=False)
    t = dict(stream=_dev(d["stream"], eng), ut=_dev(d["ut"], eng), lin=_dev(d["lin"], eng), q=_dev(d["q"], eng), N=N,
             ws=eng.streams_workspace(1, U), qt=_dev(d["qt"][:5], eng), qwin=torch.full((5,), 77, dtype=torch.int32, device=eng.device))
    rows = {k: v.reshape((U * N,) + v.shape[2:]) for k, v in
            eng.preintegrate_stream_running_stj(t["stream"], t["ut"], t["lin"], q_k_lin=t["q"], params=p2, want=ALL, N=N).items()}
    out = eng.alloc_outputs(5, ALL, 2)
    for v in out.values():
        v.fill_(7.0)
    lib = eng.lib
    order = ("prm", "R", "K", "stream", "soff", "U", "ut", "uoff", "N", "lin", "q", "ws", "rows", "Q", "qrun", "qt", "qwin", "out")
    who = "cpi_query_stream_batch: "

    def refused(text, prm=p2, rows=rows, out=out, **ch):
        a = _raw_args(eng, prm, t, rows, out, **ch)
        assert lib.cpi_query_stream_batch(eng.ctx, *[a[k] for k in order]) == 1, text
        msg = lib.cpi_last_error(eng.ctx).decode()
        assert msg == text or msg.startswith(text), (msg, text)

    def ok(prm=p2, rows=rows, out=out, **ch):
        a = _raw_args(eng, prm, t, rows, out, **ch)
        assert lib.cpi_query_stream_batch(eng.ctx, *[a[k] for k in order]) == 0, lib.cpi_last_error(eng.ctx).decode()

    means = {k: out[k] for k in MEAN}
    refused(who + "model must be 1 or 2 (the Forster comparator has no running form)", prm=p3)
    refused(who + "N (intervals per window) must be <= 65535", N=65536)
    refused(who + "Q exceeds 2^31 - 1 queries per call (32-bit grid)", Q=2 ** 31)
    refused(who + "the stream is empty", K=0)
    refused(who + "the streams hold no reading", K=0, R=2, soff=C.c_void_p(t["ws"].data_ptr()), uoff=C.c_void_p(t["ws"].data_ptr()))
    refused(who + "U > 0 windows and no run", R=0)
    refused(who + "U is 0: there is no window to query", U=0)
    refused(who + "negative size", Q=-1)
    refused(who + "NULL argument", qt=None)
    refused(who + "NULL argument", ws=None)
    refused(who + "the workspace must be 16-byte aligned", ws=C.c_void_p(t["ws"].data_ptr() + 8))
    refused(who + "model 2 needs q_k_lin", q=None)
    refused(who + "prm/rows/out is NULL", rows=None)
    refused(who + "the Jacobian fields (J_q ... O_b) of model 2 need state_transition_jacobians != 0 here", prm=p2a)
    refused(who + "rows needs q and all seven Jacobian fields for the model-2 Jacobians; missing: O_a", rows={k: v for k, v in rows.items() if k != "O_a"})
    refused(who + "rows needs DT, alpha, beta and q", rows={k: v for k, v in rows.items() if k != "DT"}, out=means)
    refused(who + "rows needs P or P_sym when out asks for P / P_sym", rows={k: rows[k] for k in MEAN}, out={"P": out["P"]})
    refused(who + "a Jacobian field of out needs the same field of rows", prm=p1, rows={k: rows[k] for k in MEAN}, out={"J_a": out["J_a"], **means})
    a = _raw_args(eng, p2, t, rows, out)
    assert lib.cpi_query_stream_batch(None, *[a[k] for k in order]) == 1
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in out.values()) and bool((t["qwin"] == 77).all()), "a refused call wrote something"
    ok(Q=0)
    ok(Q=0, U=0)
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in out.values()) and bool((t["qwin"] == 77).all()), "a no-op call wrote something"
    ok(out={})                                             # qwin_out alone
    torch.cuda.synchronize()
    assert np.array_equal(t["qwin"].cpu().numpy(), lookup(d["ut"], [0, U], np.zeros(5, dtype=np.int32), d["qt"][:5]))
    # cpi_stream_running_stj_batch: cpi_running_stj_batch's text, under its own name
    with pytest.raises(Exception, match=r"cpi_stream_running_stj_batch: the Jacobian fields \(J_q ... O_b\) of model 2 need state_transition_jacobians != 0 here"):
        eng.preintegrate_stream_running_stj(t["stream"], t["ut"], t["lin"], q_k_lin=t["q"], params=p2a, want=("mean", "jac"), N=N)
    with pytest.raises(Exception, match="cpi_stream_running_stj_batch: model must be 1 or 2"):
        eng.preintegrate_stream_running_stj(t["stream"], t["ut"], t["lin"], q_k_lin=t["q"], params=p3, want=("mean",), N=N)
    with pytest.raises(Exception, match=r"qrun\[1\] = 4 is not a run of \[0, R\)"):
        eng.query_stream_host(torch.from_numpy(d["stream"]), torch.from_numpy(d["ut"]), torch.from_numpy(d["lin"]), torch.from_numpy(d["qt"][:2].copy()),
                              q_k_lin=torch.from_numpy(d["q"]), params=p2, N=N, qrun=torch.tensor([0, 4], dtype=torch.int32))


@pytest.mark.parametrize("many", [False, True], ids=["one", "four"])
def test_host_forms_equal_the_device_forms(eng, many):
    """(f) query_stream_host and preintegrate_stream[s]_running_stj_host against the device forms (rows holding P_sym), bit for bit."""
    cpu = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    if many:
        stream, so, ut, uo, _, _, count, qrun, qt = _multi()
        keep = (qrun >= 0) & (qrun < 4)                    # the host form refuses a run out of range
        qrun, qt = qrun[keep], qt[keep]
        lin, q = _lin_q(len(ut), 8)
    else:
        d = _single()
        stream, ut, count, qt, lin, q = d["stream"], d["ut"], d["count"], d["qt"], d["lin"], d["q"]
        so = uo = qrun = None
    N = int(count.max())
    for model, avg in ((1, 0), (2, 1)):
        prm = eng.make_params(model, bool(avg))
        want_rows = ("mean", "jac", "cov_sym")
        dv = [_dev(x, eng) for x in (stream, ut, lin, q, qt, so, uo, qrun)]
        if many:
            rows = eng.preintegrate_streams_running_stj(dv[0], dv[5], dv[1], dv[6], dv[2], q_k_lin=dv[3], params=prm, want=want_rows, N=N)
            hrows, hcnt = eng.preintegrate_streams_running_stj_host(cpu(stream), so, cpu(ut), uo, cpu(lin), q_k_lin=cpu(q), params=prm,
                                                                   want=want_rows, N=N, return_counts=True)
        else:
            rows = eng.preintegrate_stream_running_stj(dv[0], dv[1], dv[2], q_k_lin=dv[3], params=prm, want=want_rows, N=N)
            hrows, hcnt = eng.preintegrate_stream_running_stj_host(cpu(stream), cpu(ut), cpu(lin), q_k_lin=cpu(q), params=prm, want=want_rows,
                                                                  N=N, return_counts=True)
        assert np.array_equal(hcnt.numpy(), count)
        rd = _np(rows)
        assert sorted(rd) == sorted(hrows)
        for k in rd:
            assert _bits(rd[k], hrows[k].numpy()), ("rows", model, k)
        out, qwin = eng.query_stream(dv[0], dv[1], dv[2], rows, dv[4], q_k_lin=dv[3], params=prm, want=ALL, N=N, stream_offsets=dv[5],
                                     update_offsets=dv[6], qrun=dv[7])
        hout, hqwin = eng.query_stream_host(cpu(stream), cpu(ut), cpu(lin), cpu(qt), q_k_lin=cpu(q), params=prm, want=ALL, N=N,
                                            stream_offsets=so, update_offsets=uo, qrun=cpu(qrun))
        assert np.array_equal(qwin.cpu().numpy(), hqwin.numpy())
        out = _np(out)
        assert sorted(out) == sorted(hout)
        for k in out:
            assert _bits(out[k], hout[k].numpy()), ("query", model, k)


def test_running_then_query_replays_from_a_graph(eng):
    """(g) one capture of cpi_stream_running_stj_batch followed by cpi_query_stream_batch -- a chain on one stream -- replays to the
    bits of the eager calls."""
    d = _single()
    N = int(d["count"].max())
    U = len(d["ut"])
    ds, du, dl, dq, dt = (_dev(d[k], eng) for k in ("stream", "ut", "lin", "q", "qt"))
    prm = eng.make_params(2, True)
    ws = eng.streams_workspace(1, U)
    rows = eng.preintegrate_stream_running_stj(ds, du, dl, q_k_lin=dq, params=prm, want=ALL, N=N, workspace=ws)
    out, qwin = eng.query_stream(ds, du, dl, rows, dt, q_k_lin=dq, params=prm, want=ALL, N=N, workspace=ws)
    lib, ro, oo = eng.lib, eng._outputs_struct(rows), eng._outputs_struct(out)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def call():
        eng._sync_stream()
        eng._check(lib.cpi_stream_running_stj_batch(eng.ctx, C.byref(prm), 1, len(d["stream"]), ptr(ds), None, U, ptr(du), None, N, ptr(dl),
                                                    ptr(dq), ptr(ws), C.byref(ro)))
        eng._check(lib.cpi_query_stream_batch(eng.ctx, C.byref(prm), 1, len(d["stream"]), ptr(ds), None, U, ptr(du), None, N, ptr(dl), ptr(dq),
                                              ptr(ws), C.byref(ro), len(d["qt"]), None, ptr(dt), ptr(qwin), C.byref(oo)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                          # warm-up on the side stream, as graph capture requires
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    eager_qwin = qwin.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for v in list(out.values()) + list(rows.values()) + [qwin, ws]:
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(qwin, eager_qwin)
    for k in out:
        assert _bits(out[k].cpu().numpy(), eager[k].cpu().numpy()), k


def test_composition_with_the_factor_sweeps(eng):
    """(h) query_stream -> sqrt_information (packed) -> factor_hessian with idx_i = qwin runs and equals the same chain fed from
    query_stj on the assembled windows."""
    d = _single()
    N = int(d["count"].max())
    U = len(d["ut"])
    prm = eng.make_params(2, True)
    want = ("mean", "jac", "cov_sym")
    a, rows_ref, _ = _assembled_route(eng, d, prm, N, want)
    ds, du = _dev(d["stream"], eng), _dev(d["ut"], eng)
    w_all = lookup(d["ut"], [0, U], np.zeros(len(d["qt"]), dtype=np.int32), d["qt"])
    i_all, step_all, _ = classify(d["knots"], d["first"], d["count"], w_all, d["qt"])
    qt = d["qt"][step_all & (i_all >= 1)][:64]              # stepped queries behind at least one whole interval: P is well conditioned
    dt = _dev(qt, eng)
    rows = eng.preintegrate_stream_running_stj(ds, du, a["lin"], q_k_lin=a["q"], params=prm, want=want, N=N)
    meas, qwin = eng.query_stream(ds, du, a["lin"], rows, dt, q_k_lin=a["q"], params=prm, want=want, N=N)
    twin = eng.query_stj(a["knots"], a["lin"], rows_ref, qwin, dt, q_k_lin=a["q"], params=prm, want=want, first=a["first"], count=a["count"], N=N)
    F = len(qt)
    qw = qwin.cpu().numpy()
    assert (qw >= 0).all() and len(set(qw)) > 3
    mc = {k: v.cpu() for k, v in meas.items()}
    lin_f, qk_f = torch.from_numpy(d["lin"][qw]), _dev(d["q"][qw], eng)
    xi, xj = synth.make_states(mc["alpha"], mc["beta"], mc["q"], mc["DT"], lin_f, 2, seed=99)
    # state i of factor f sits at index qwin[f] (one state per window: the first factor of a window supplies it), state j at U + f
    si = torch.zeros((U, 16), dtype=torch.float64)
    si[:, 3] = 1.0
    first_of = {}
    for f, u in enumerate(qw):
        first_of.setdefault(int(u), f)
    for u, f in first_of.items():
        si[u] = xi[f]
    states = torch.cat([si, xj]).contiguous().to(eng.device)
    idx_j = _dev((U + np.arange(F)).astype(np.int32), eng)
    res = {}
    for label, m in (("stream", meas), ("assembled", twin)):
        R = eng.sqrt_information(m["P_sym"])
        mm = {k: v for k, v in m.items() if k != "P_sym"}
        res[label] = eng.factor_hessian(2, mm, lin_f.to(eng.device), qk_f, states, R, idx_i=qwin, idx_j=idx_j)
    torch.cuda.synchronize()
    h1, h2 = res["stream"].cpu().numpy(), res["assembled"].cpu().numpy()
    assert np.isfinite(h1).all() and np.abs(h1).max() > 0 and _bits(h1, h2)
