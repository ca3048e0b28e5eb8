"""GPU: the query family for windows that continue from a carried state (cpi_query_open_batch[_host], Engine.query_open[_host]).

The exact test: on a VIEW of a closed window -- first + m, count - m, rows m ..., base = row m - 1 -- the open entry must return the
bits of the closed entry (cpi_query_cov_batch for model 1, cpi_query_stj_batch for model 2) on the whole window for every query time
>= t_m, and the base row's bits before t_m.  The end-to-end test runs a real chain of cpi_running_resume_stj_batch, queries its second
segment with the first call's rows as base and compares with the oracle on the cut window (tests/tol.py: TOL_*), then takes the
result through the whitened factor sweep.  Cuts lie on and beside the pass lengths of cov_body (14 for model 1, CH for model 2)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cpi_amd import synth
from oracle import oracle_py as op
from tests.test_gpu_query import _index, _queries
from tests.test_gpu_stj import ALL, CH, JAC7, MEAN, _bits, _dev, _np
from tests.tol import TOL_FACTOR, check_pre

pytestmark = pytest.mark.gpu
JAC5 = JAC7[:5]
CH1 = 14                      # cov_body<1>'s pass length (cpi_cov_kernels.hpp: CH)
QS = (1, 5, 65, 130)          # 1 / 4 / 64 queries per wavefront, and a partly filled last wavefront


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _windows(N):
    return tuple(t.numpy() for t in synth.make_windows(7, N, seed=9300 + N, edge_cases=False))


def _closed_rows(eng, model, kn, lin, q, prm):
    fn = eng.preintegrate_running_stj if model == 2 else eng.preintegrate_running
    return fn(_dev(kn, eng), _dev(lin, eng), _dev(q, eng) if model == 2 else None, prm, want=ALL)


def _times(kn, m):
    """Per window: before t_m (twice), on t_m, inside interval m, on a later stamp, inside the last interval, on t_n, past t_n, NaN."""
    W, N = kn.shape[0], kn.shape[1] - 1
    qw, qt = [], []
    for w in range(W):
        t = kn[w, :, 0]
        later = min(m + 2, N)
        ts = [t[m] - 1e-3, t[m - 1], t[m], t[m] + 0.37 * (t[m + 1] - t[m]), t[later], t[N - 1] + 0.6 * (t[N] - t[N - 1]), t[N], t[N] + 0.01, np.nan]
        qw += [w] * len(ts)
        qt += ts
    return np.array(qw, dtype=np.int32), np.array(qt)


@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("model,avg", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_open_view_of_a_closed_window_is_exact(eng, model, avg, layout):
    ch = CH if model == 2 else CH1
    _open_view_is_exact(eng, model, avg, layout, tuple(x[:3] for x in _windows(2 * ch + 1)))


def _open_view_is_exact(eng, model, avg, layout, windows):
    """The exact test on dense windows (kn, lin, q) of 2 ch + 1 intervals (tests/test_gpu_stj_edges.py repeats it on tumbling ones)."""
    ch = CH if model == 2 else CH1
    kn, lin, q = windows
    W, N = kn.shape[0], kn.shape[1] - 1
    assert N == 2 * ch + 1
    prm = eng.make_params(model, bool(avg))
    rows = _closed_rows(eng, model, kn, lin, q, prm)
    fields = MEAN + (JAC7 if model == 2 else JAC5) + ("P", "P_sym")
    d_kn, d_lin, d_q = _dev(kn, eng), _dev(lin, eng), (_dev(q, eng) if model == 2 else None)
    closed_fn = eng.query_stj if model == 2 else eng.query
    r_np = _np(rows)
    rng = np.random.default_rng(11)
    for m in (1, ch - 1, ch, ch + 1, N - 1):
        qw_all, qt_all = _times(kn, m)
        view_rows = {k: v[:, m:].contiguous() for k, v in rows.items()}
        bases = {"one row": {k: v[:, m - 1].contiguous() for k, v in rows.items()}, "in place": {k: v[:, :m].contiguous() for k, v in rows.items()}}
        if layout == "dense":
            view = dict(knots=_dev(kn[:, m:], eng))
        else:
            view = dict(knots=_dev(kn.reshape(-1, 7), eng), first=_dev(np.arange(W, dtype=np.int64) * (N + 1) + m, eng),
                        count=_dev(np.full(W, N - m, dtype=np.int32), eng), N=N - m)
        for Q in QS:
            sel = np.resize(rng.permutation(len(qw_all)), Q)
            qw, qt = qw_all[sel], qt_all[sel]
            dqw, dqt = _dev(qw, eng), _dev(qt, eng)
            closed = _np(closed_fn(d_kn, d_lin, rows, dqw, dqt, q_k_lin=d_q, params=prm, want=ALL))
            assert set(closed) == set(fields)
            after = ~(qt < kn[qw, m, 0])                      # t_q >= t_m, and the NaN times
            for label, base in bases.items():
                got = _np(eng.query_open(view["knots"], d_lin, view_rows, dqw, dqt, base, q_k_lin=d_q, params=prm, want=ALL,
                                         **{k: v for k, v in view.items() if k != "knots"}))
                for k in fields:
                    assert _bits(got[k][after], closed[k][after]), (m, Q, label, k)
                    assert _bits(got[k][~after], r_np[k][qw[~after], m - 1]), (m, Q, label, k)
                    assert np.isnan(got[k][np.isnan(qt)]).all(), (m, Q, label, k)
        # base = None: the closed entry itself
        none = _np(eng.query_open(d_kn, d_lin, rows, dqw, dqt, None, q_k_lin=d_q, params=prm, want=ALL))
        assert all(_bits(none[k], closed[k]) for k in fields), m


def _cut_reference(model, avg, kn, lin, q, qw, qt, counts):
    idx = _index(kn, counts, qw, qt)
    N = kn.shape[1] - 1
    win = np.zeros((len(qw), N + 2, 7))
    for k, (w, t, i) in enumerate(zip(qw, qt, idx)):
        win[k, :i + 1] = kn[w, :i + 1]
        win[k, i + 1:] = kn[w, i]
        win[k, i + 1:, 0] = min(max(t, kn[w, 0, 0]), kn[w, counts[w], 0])
    return win, op.oracle().run(op.make_params(model, avg, 1), win, lin[qw], q[qw])


@pytest.mark.parametrize("avg", [0, 1])
def test_chain_then_open_query_end_to_end(eng, avg):
    """Two segments of cpi_running_resume_stj_batch cut on a pass (CH | CH + 1); every query of tests/test_gpu_query.py's list that falls
    into the second segment, against the oracle on the cut window; then out -> sqrt_information(P_sym) -> whitened factor_eval with
    idx_i = qwin against the same sweep fed by Engine.preintegrate on the cut windows (TOL_FACTOR)."""
    W, m, N = 3, CH, 2 * CH + 1
    kn, lin, q = (x[:W] for x in _windows(N))
    prm = eng.make_params(2, bool(avg))
    d_lin, d_q = _dev(lin, eng), _dev(q, eng)
    want = ("mean", "jac", "cov", "cov_sym")
    rows0, carry = eng.preintegrate_running_resume_stj(_dev(kn[:, :m + 1], eng), d_lin, d_q, prm, want=want)
    seg = _dev(kn[:, m:], eng)
    rows1, _ = eng.preintegrate_running_resume_stj(seg, d_lin, d_q, prm, want=want, carry_in=carry)
    counts = np.full(W, N, dtype=np.int32)
    qw, qt = _queries(kn, counts)
    keep = qt >= kn[qw, m, 0]
    qw, qt = qw[keep], qt[keep]
    got_t = eng.query_open(seg, d_lin, rows1, _dev(qw, eng), _dev(qt, eng), rows0, q_k_lin=d_q, params=prm, want=want)
    got = _np(got_t)
    win, ref = _cut_reference(2, avg, kn, lin, q, qw, qt, counts)
    keys = MEAN + JAC7 + ("P",)
    check_pre({k: got[k] for k in keys}, {k: ref[k] for k in keys}, what=("mean", "jac", "cov"), v2=True, label="open query avg%d" % avg)
    print("open query avg %d, %d queries: %s" % (avg, len(qw), ", ".join("%s %.2e" % (k, float(np.abs(got[k] - ref[k]).max())) for k in keys)))
    # the factor at the query times: 2 queries per window, inside intervals of the second segment
    pick = np.concatenate([np.flatnonzero((qw == w) & (_index(kn, counts, qw, qt) < N) & (qt > kn[qw, _index(kn, counts, qw, qt), 0]))[[0, -1]] for w in range(W)])
    pw = qw[pick]
    meas = {k: v[_dev(pick, eng)].contiguous() for k, v in got_t.items() if k != "P"}
    cut = eng.preintegrate(_dev(win[pick], eng), _dev(lin[pw], eng), _dev(q[pw], eng), params=prm, want=("mean", "jac", "cov_sym"))
    rc = {k: v.cpu() for k, v in cut.items()}
    xi, xjs = None, []
    for s_ in range(2):
        p2 = torch.arange(s_, len(pick), 2)
        a, b = synth.make_states(rc["alpha"][p2], rc["beta"][p2], rc["q"][p2], rc["DT"][p2], torch.from_numpy(lin), 2, seed=321)
        assert xi is None or torch.equal(a, xi)
        xi = a
        xjs.append(b)
    states = torch.cat([xi] + xjs).contiguous().to(eng.device)
    idx_i = _dev(pw, eng)
    idx_j = _dev((W + (np.arange(len(pick)) % 2) * W + pw).astype(np.int32), eng)
    lin_f, qk_f = _dev(lin[pw], eng), _dev(q[pw], eng)
    out = {}
    for label, mm in (("open", meas), ("cut", cut)):
        R = eng.sqrt_information(mm["P_sym"])
        mm = {k: v for k, v in mm.items() if k != "P_sym"}
        out[label] = _np(eng.factor_eval(2, mm, lin_f, qk_f, states, idx_i, idx_j, sqrt_info=R))
    for k in ("err", "H1", "H2"):
        e = float(np.abs(out["open"][k] - out["cut"][k]).max())
        print("whitened factor at open query times avg %d: %s max-abs difference %.3e" % (avg, k, e))
        assert np.isfinite(out["open"][k]).all() and e <= TOL_FACTOR, (k, e)


def test_nan_base_row_clamped_windows_and_refusals(eng):
    from cpi_amd import CpiError
    W, m, N = 3, CH, 2 * CH + 1
    kn, lin, q = (x[:W] for x in _windows(N))
    prm = eng.make_params(2)
    d_lin, d_q = _dev(lin, eng), _dev(q, eng)
    rows0, carry = eng.preintegrate_running_resume_stj(_dev(kn[:, :m + 1], eng), d_lin, d_q, prm, want=ALL)
    seg = _dev(kn[:, m:], eng)
    rows1, _ = eng.preintegrate_running_resume_stj(seg, d_lin, d_q, prm, want=ALL, carry_in=carry)
    qw, qt = _times(kn, m)
    dqw, dqt = _dev(qw, eng), _dev(qt, eng)
    clean = _np(eng.query_open(seg, d_lin, rows1, dqw, dqt, rows0, q_k_lin=d_q, params=prm, want=ALL))
    # a refused carry (window 1: no covariance state) leaves NaN rows; as base and as rows they give NaN for that window's queries only
    bad = carry.clone()
    bad[1, 0] = float(int(bad[1, 0].item()) & ~2)
    zero = _dev(np.zeros(W, dtype=np.int32), eng)
    base_bad, _ = eng.preintegrate_running_resume_stj(_dev(kn[:, m:m + 2], eng), d_lin, d_q, prm, want=ALL, carry_in=bad, count=zero)
    rows_bad, _ = eng.preintegrate_running_resume_stj(seg, d_lin, d_q, prm, want=ALL, carry_in=bad)
    assert torch.isnan(base_bad["q"][1]).all() and not torch.isnan(base_bad["q"][[0, 2]]).any()
    got = _np(eng.query_open(seg, d_lin, rows_bad, dqw, dqt, base_bad, q_k_lin=d_q, params=prm, want=ALL))
    sick = qw == 1
    for k in got:
        assert np.isnan(got[k][sick]).all(), k
        assert _bits(got[k][~sick], clean[k][~sick]), k
    # a NaN base row over healthy rows: the queries that gather it are NaN, the others of the window are not
    got = _np(eng.query_open(seg, d_lin, rows1, dqw, dqt, base_bad, q_k_lin=d_q, params=prm, want=ALL))
    from_base = sick & ~(qt >= kn[qw, m + 1, 0])
    for k in got:
        assert np.isnan(got[k][from_base]).all() and _bits(got[k][~from_base], clean[k][~from_base]), k
    # qwin out of range is clamped
    t4 = kn[[0, 0, W - 1, W - 1], m + 1, 0] + 1e-3
    wild = _np(eng.query_open(seg, d_lin, rows1, _dev(np.array([-5, 0, 99, W - 1], dtype=np.int32), eng), _dev(t4, eng), rows0, q_k_lin=d_q, params=prm, want=ALL))
    for k in wild:
        assert _bits(wild[k][0], wild[k][1]) and _bits(wild[k][2], wild[k][3]), k
    # N == 0: every query gets the base row, rows is not read
    got0 = _np(eng.query_open(_dev(kn[:, m:m + 1], eng), d_lin, {}, dqw, dqt, rows0, q_k_lin=d_q, params=prm, want=ALL))
    r0 = _np(rows0)
    ok = ~np.isnan(qt)
    for k in got0:
        assert _bits(got0[k][ok], r0[k][qw[ok], -1]) and np.isnan(got0[k][~ok]).all(), k
    # refusals
    who = "cpi_query_open_batch: "
    for f in ("q", "O_a"):
        with pytest.raises(CpiError, match=who + "base needs q and all seven Jacobian fields for the model-2 Jacobians; missing: %s" % f):
            eng.query_open(seg, d_lin, rows1, dqw, dqt, {k: v for k, v in rows0.items() if k != f}, q_k_lin=d_q, params=prm, want=("jac",))
    with pytest.raises(CpiError, match=who + "base needs P or P_sym"):
        eng.query_open(seg, d_lin, rows1, dqw, dqt, {k: v for k, v in rows0.items() if k not in ("P", "P_sym")}, q_k_lin=d_q, params=prm, want=("cov",))
    with pytest.raises(CpiError, match=who + "base needs DT, alpha, beta and q"):
        eng.query_open(seg, d_lin, rows1, dqw, dqt, {k: v for k, v in rows0.items() if k != "DT"}, q_k_lin=d_q, params=prm, want=("mean",))
    with pytest.raises(CpiError, match=who + "rows needs q and all seven"):
        eng.query_open(seg, d_lin, {k: v for k, v in rows1.items() if k != "H_b"}, dqw, dqt, rows0, q_k_lin=d_q, params=prm, want=("jac",))
    with pytest.raises(CpiError, match=who + ".*analytic O_a / O_b recursion has no running form"):
        eng.query_open(seg, d_lin, rows1, dqw, dqt, rows0, q_k_lin=d_q, params=eng.make_params(2, state_transition_jacobians=False), want=("jac",))
    with pytest.raises(CpiError, match=who + "model must be 1 or 2"):
        eng.query_open(seg, d_lin, rows1, dqw, dqt, rows0, q_k_lin=d_q, params=eng.make_params(3), want=("mean",))
    out = eng.alloc_outputs(len(qw), ALL, 2)
    ro, bo, oo = (eng._outputs_struct({k: v for k, v in x.items()}) for x in (rows1, rows0, out))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for bn in (0, -3):
        rc = eng.lib.cpi_query_open_batch(eng.ctx, C.byref(prm), W, N - m, ptr(seg), None, None, ptr(d_lin), ptr(d_q), C.byref(ro), len(qw), ptr(dqw),
                                          ptr(dqt), C.byref(oo), C.byref(bo), bn)
        assert rc == 1 and eng.lib.cpi_last_error(eng.ctx).decode() == who + "base_N must be >= 1 when base is given"


@pytest.mark.parametrize("model", [1, 2])
def test_host_form_is_the_device_composition(eng, model):
    """cpi_query_open_batch_host over two chunks: the bits of base row (N = 1, counts 0) + rows + cpi_query_open_batch with rows that
    hold P_sym, and of the records."""
    from cpi_amd import CpiError
    ch = CH if model == 2 else CH1
    W, m, N = 3, ch + 1, 2 * ch + 1
    kn, lin, q = (x[:W] for x in _windows(N))
    prm = eng.make_params(model, True)
    d_lin, d_q = _dev(lin, eng), (_dev(q, eng) if model == 2 else None)
    h_lin, h_q = torch.from_numpy(lin.copy()), (torch.from_numpy(q.copy()) if model == 2 else None)
    staged = ("mean", "jac", "cov_sym")
    zero = _dev(np.zeros(W, dtype=np.int32), eng)
    carry_d = carry_h = None
    for a, b in ((0, m), (m, N)):
        qw, qt = _times(kn[:, a:b + 1] if a else kn[:, :b + 1], 1)
        seg = _dev(kn[:, a:b + 1], eng)
        base, _ = eng.preintegrate_running_resume_stj(_dev(kn[:, a:a + 2], eng), d_lin, d_q, prm, want=staged, carry_in=carry_d, count=zero)
        rows, co = eng.preintegrate_running_resume_stj(seg, d_lin, d_q, prm, want=staged, carry_in=carry_d)
        dev = _np(eng.query_open(seg, d_lin, rows, _dev(qw, eng), _dev(qt, eng), base, q_k_lin=d_q, params=prm, want=ALL))
        host, hco = eng.query_open_host(torch.from_numpy(kn[:, a:b + 1].copy()), h_lin, torch.from_numpy(qw), torch.from_numpy(qt), q_k_lin=h_q,
                                        params=prm, want=ALL, carry_in=carry_h)
        assert set(host) == set(dev)
        for k in dev:
            assert _bits(host[k].numpy(), dev[k]), (a, k)
        cd, chh = co.cpu().numpy(), hco.numpy()
        off, size = (80, 27 * 18) if model == 2 else (62, 225)       # the covariance state of a record (cpi_args.hpp: carry::cov_off)
        assert _bits(cd[:, :17], chh[:, :17]) and _bits(cd[:, off:off + size], chh[:, off:off + size]), a
        if model == 1:
            assert _bits(cd[:, 17:62], chh[:, 17:62]), a
        carry_d, carry_h = co, hco
    with pytest.raises(CpiError, match=r"cpi_query_open_batch_host: qwin\[0\] = 7 is not a window"):
        eng.query_open_host(torch.from_numpy(kn[:, :3].copy()), h_lin, torch.tensor([7], dtype=torch.int32), torch.tensor([0.0], dtype=torch.float64),
                            q_k_lin=h_q, params=prm, want=("mean",))


def test_resume_then_open_query_replays_from_a_graph(eng):
    """One capture of cpi_running_resume_stj_batch followed by cpi_query_open_batch -- a chain on one stream -- replays to the bits of
    the eager calls."""
    W, m, N = 3, CH, 2 * CH + 1
    kn, lin, q = (x[:W] for x in _windows(N))
    prm = eng.make_params(2, True)
    d_lin, d_q = _dev(lin, eng), _dev(q, eng)
    want_r = ("mean", "jac", "cov_sym")
    rows0, carry = eng.preintegrate_running_resume_stj(_dev(kn[:, :m + 1], eng), d_lin, d_q, prm, want=want_r)
    seg = _dev(kn[:, m:], eng)
    qw_h, qt_h = _times(kn, m)
    qw, qt = _dev(qw_h, eng), _dev(qt_h, eng)
    rows, cout = eng.preintegrate_running_resume_stj(seg, d_lin, d_q, prm, want=want_r, carry_in=carry)
    out = eng.query_open(seg, d_lin, rows, qw, qt, rows0, q_k_lin=d_q, params=prm, want=ALL)

    def call():
        eng.preintegrate_running_resume_stj(seg, d_lin, d_q, prm, want=want_r, carry_in=carry, carry_out=cout, out=rows)
        eng.query_open(seg, d_lin, rows, qw, qt, rows0, q_k_lin=d_q, params=prm, want=ALL, out=out)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                          # warm-up on the side stream, as graph capture requires
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    eager_c = cout.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for v in list(out.values()) + list(rows.values()):
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in out:
        assert _bits(out[k].cpu().numpy(), eager[k].cpu().numpy()), k
    assert _bits(cout.cpu().numpy()[:, 80:], eager_c.cpu().numpy()[:, 80:])
