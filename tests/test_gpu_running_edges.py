"""GPU: the running family (cpi_preintegrate_running, _running_resume, _stream[s]_running) where the other running tests never
go -- window lengths on and beside the pass boundaries of the covariance kernel (cov_body: CH = 14 / 23 intervals per pass,
the rotation carried through LDS between passes) and the row groups of the mean kernel (CPI_RUN_T = 6), resume chains cut on
and beside a pass, stream windows whose tail interval opens a pass, rotations large enough for every branch of rot_2_quat,
the wide polynomial and the Cody-Waite reduction of sincos_fast and lane scans past 90 degrees, scaled inputs, and the longest
windows.  The inputs come from tests/running_cases.py; tests/test_running_cases_cpu.py keeps them honest.

Reference: the C restatement's trace (oracle_py.oracle().trace) of the whole window, every row of every window of every
case, at the gates of tests/tol.py -- absolute where the inputs are those of cpi_amd.synth, relative to max(1, |ref|.max())
of the field where they are scaled, as the stress tests of tests/test_gpu_parity.py apply them.  The row arrays are filled
with NaN before every call.  The largest error per field is printed (pytest -s); the figures measured on an MI355X are in
profiles/running_edges.md."""
import numpy as np
import pytest
import torch

from cpi_amd import stream as st
from cpi_amd import synth
from oracle import oracle_py as op
from tests.running_cases import EDGE_N, PASS, STREAM_CASES, tumbling_stream, tumbling_windows, wdt
from tests.test_gpu_running import (LANES, MEAN, MODES, ZERO_Q, _check_rows, _dev, _host, _keys, _ragged, _ragged_layout, _wants,
                                    _what, _Worst, trace_rows)
from tests.test_gpu_running_resume import _record_fields, _run_chain, _check_chain, _segment_ref
from tests.test_gpu_stream_running import _dense, _Guarded, _nan_rows, _stream_rows
from tests.tol import TOL_COV, TOL_JAC, TOL_MEAN, check_pre, cov_rel_err

pytestmark = pytest.mark.gpu
CHAIN_LANES = (0, 1, 3, 8, 64)


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _check_rel(got, ref, keys, label):
    """The gates of tests/tol.py relative to the magnitude of the quantity (the covariance gate is relative as it stands)."""
    msgs = []
    for k in keys:
        if k == "P":
            e, tol = cov_rel_err(got["P"], ref["P"]), TOL_COV
        else:
            e = float(np.abs(got[k] - ref[k]).max())
            tol = (TOL_MEAN if k in MEAN else TOL_JAC) * max(1.0, float(np.abs(ref[k]).max()))
        if not e <= tol:
            msgs.append("%s %s err %.3e (gate %.3e)" % (label, k, e, tol))
    assert not msgs, "; ".join(msgs)


def _check_rows_rel(got, ref, want, label, worst=None):
    _check_rel(got, ref, _keys(want), label)
    if worst is not None:
        worst.add(got, ref, _keys(want))
    if "cov_sym" in want and "cov" in want:      # P_sym: bit for bit the upper triangle of the P row
        from cpi_amd.engine import pack_sym
        assert np.array_equal(pack_sym(torch.from_numpy(got["P"].reshape(-1, 225))).numpy(), got["P_sym"].reshape(-1, 120)), label + " P_sym"


def _check_chain_rel(segs, ref, cuts, want, label, worst=None):
    for c, (rows, count, Ns) in enumerate(segs):
        _check_rows_rel(rows, _segment_ref(ref, cuts[:, c], cuts[:, c + 1], Ns), want, "%s segment %d" % (label, c), worst)


def _chain_equals_one_shot(segs, one, cuts, want):
    return all(np.array_equal(rows[k], _segment_ref(one, cuts[:, c], cuts[:, c + 1], Ns)[k])
               for c, (rows, _, Ns) in enumerate(segs) for k in _keys(want))


def _requests(model, lanes=LANES):
    """The full request with every lane count, the other requests with automatic lanes and one lane."""
    wants = _wants(model)
    return [(L, wants[-1]) for L in lanes] + [(L, w) for w in wants[:-1] for L in (0, 1)]


def _running(eng, prm, want, nwin, nrow, **args):
    """preintegrate_running into [nwin, nrow, ...] row arrays filled with NaN."""
    return _host(eng.preintegrate_running(params=prm, want=want, out=_nan_rows(eng, nwin, nrow, want, prm.model), **args))


# --------------------------------------------------------------------------- 1. window lengths on and beside every boundary
@pytest.mark.parametrize("mode", MODES)
def test_running_edge_lengths(eng, mode):
    """Every N of EDGE_N as a ragged batch with garbage counts, inside guard bands: every row against the oracle's trace, the
    rows from a window's count on equal to the row before them, the last row against Engine.preintegrate."""
    model, avg = mode
    W, G, SENT = 37, 4096, -7.25
    worst = _Worst()
    for N in EDGE_N:
        kn, lin, q, flat, first, count, given = _ragged(W, N, 700 + N, garbage=True)
        ref = trace_rows(model, avg, kn, lin, q, count)
        args = dict(knots=_dev(flat, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng), first=_dev(first, eng), count=_dev(given, eng), N=N)
        for L, want in _requests(model):
            label = "edge N%d m%d avg%d L%d %s" % (N, model, avg, L, "+".join(want))
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)
            bufs, views = {}, {}
            for k, v in eng.alloc_outputs(W * N, want, model).items():
                n = v[0].numel()
                bufs[k] = torch.full((2 * G + W * N * n,), SENT, dtype=torch.float64, device=eng.device)
                views[k] = bufs[k][G:G + W * N * n].view((W, N) + tuple(v.shape[1:]))
                views[k].fill_(float("nan"))
            got = _host(eng.preintegrate_running(params=prm, want=want, out=views, **args))
            assert all(v.shape[:2] == (W, N) for v in got.values())
            _check_rows(got, ref, want, label, worst)
            for k, b in bufs.items():
                assert torch.all(b[:G] == SENT) and torch.all(b[-G:] == SENT), (label, k)
            for k, v in got.items():
                zero = ZERO_Q if k == "q" else np.zeros(v.shape[2:])
                for w in range(W):
                    c = int(count[w])
                    assert np.array_equal(v[w, c:], np.broadcast_to(v[w, c - 1] if c > 0 else zero, v[w, c:].shape)), (label, k, w, c)
            bwant = tuple(g for g in want if g != "cov_sym")
            fin = _host(eng.preintegrate(params=prm, want=bwant, **args))
            check_pre({k: got[k][:, N - 1] for k in _keys(want)}, fin, what=_what(want), label=label + " last row vs preintegrate")
    worst.report("edge lengths vs oracle.trace, model %d imu_avg %d" % (model, avg))


# --------------------------------------------------------------------------- 2. chains cut on and beside a pass
def _pass_cuts(C, N, W):
    tables = [[0, C, 2 * C, 3 * C, N], [0, C - 1, 2 * C + 1, N], [0, C + 1, N], [0, 1, 1 + 2 * C, N], [0, N - C, N], [0, 0, N - 1, N]]
    tables = [[c for c in t if 0 <= c <= N] for t in tables]
    assert all(t == sorted(t) and t[0] == 0 and t[-1] == N for t in tables)
    parts = max(len(t) for t in tables)
    tables = [t + [N] * (parts - len(t)) for t in tables]   # padded with repeated cuts: segments of no interval
    return np.array([tables[w % len(tables)] for w in range(W)], dtype=np.int64)


@pytest.mark.parametrize("mode", MODES)
def test_running_resume_chains_cut_on_and_beside_passes(eng, mode):
    """Windows of 70 intervals as chains whose cuts fall on a pass boundary of the covariance kernel, one interval before and
    after it, with segments longer than a pass, of exactly one pass, of one interval and of none: every segment against the
    whole-window trace, the last record against the last row, and the record continued by a zero-interval preintegrate_resume
    against the window's measurement (model 2: its Jacobians included)."""
    model, avg = mode
    W, N = 37, 70
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=811))
    ref = trace_rows(model, avg, kn, lin, q)
    fin = op.oracle().run(op.make_params(model, avg, 1), kn, lin, q)
    cuts = _pass_cuts(PASS[model], N, W)
    end = _dev(kn[:, N:], eng)
    worst, bit_equal = _Worst(), []
    for L in CHAIN_LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        for want in _wants(model):
            label = "pass cuts m%d avg%d L%d %s" % (model, avg, L, "+".join(want))
            segs, carry = _run_chain(eng, prm, kn, lin, q, cuts, want, nan_rows=True)
            _check_chain(segs, ref, cuts, want, label, worst)
            rows, _, Ns = segs[-1]
            rec = _record_fields(carry.cpu().numpy(), model)
            for k in _keys(want):
                if k in rec and (k != "P" or model == 1):
                    assert np.array_equal(rec[k], rows[k][:, Ns - 1]), (label, "record vs last row", k)
            rwant = ("mean", "jac", "cov") if "cov" in want else tuple(g for g in want if g != "cov_sym")
            out, _ = eng.preintegrate_resume(end, _dev(lin, eng), _dev(q, eng), prm, want=rwant, carry_in=carry)
            check_pre(_host(out), fin, what=rwant, v2=(model == 2), label=label + " continued by preintegrate_resume")
            if L == 1:
                one = _running(eng, prm, want, W, N, knots=_dev(kn, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng))
                bit_equal.append(("+".join(want), _chain_equals_one_shot(segs, one, cuts, want)))
    worst.report("chains cut on and beside passes vs oracle.trace, model %d imu_avg %d" % (model, avg))
    print("one-lane chains bit-equal to the one-shot running call: %s" % ", ".join("%s: %s" % be for be in bit_equal))


# --------------------------------------------------------------------------- 3. the tail interval of a stream window opens a pass
@pytest.mark.parametrize("mode", MODES)
def test_stream_running_tail_on_a_pass_boundary(eng, mode):
    """Stream windows of n whole intervals and, with a phase, the tail interval -- whose closing knot is not in memory -- as
    interval n: slot 0 of a pass for (23, 0.37) and (46, 0.37) (model 2) and (14, 0.37) (model 1); (23, 0) and (28, 0) end
    exactly on a pass.  Bit-identity with preintegrate_running on the host-assembled windows, the oracle's trace on every row,
    and both sentinel runs of _stream_rows."""
    model, avg = mode
    want = _wants(model)[-1]
    worst = _Worst()
    for n, phase in STREAM_CASES:
        s, u, lin, q = tumbling_stream(n, phase)
        knots, first, count = st.assemble_windows(s, u)
        U, N = len(u), int(count.max())
        assert N == n + (1 if phase > 0 else 0) and np.all(count == N)
        ref = trace_rows(model, avg, _dense(knots, first, count, N), lin, q, count)
        g = _Guarded(eng, s, u)
        dl, dq = _dev(lin, eng), _dev(q, eng)
        ck, cf, cc = _dev(knots, eng), _dev(first, eng), _dev(count, eng)
        for L in LANES:
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)
            label = "tail n%d phase %g m%d avg%d L%d" % (n, phase, model, avg, L)
            got, cnt = _stream_rows(eng, g, dl, dq, prm, want, N, label)
            assert np.array_equal(cnt, count), label
            rag = _running(eng, prm, want, U, N, knots=ck, lin=dl, q_k_lin=dq, first=cf, count=cc, N=N)
            assert sorted(got) == sorted(rag)
            for k in rag:
                assert np.array_equal(got[k], rag[k]), (label, k)
            _check_rows(got, ref, want, label, worst)
    worst.report("stream windows with the tail on a pass boundary vs oracle.trace, model %d imu_avg %d" % (model, avg))


# --------------------------------------------------------------------------- 4. large rotations
@pytest.mark.parametrize("mode", MODES)
def test_running_family_under_large_rotations(eng, mode):
    """The tumbling windows (|w| dt up to ~1.16 rad per interval, all inside the stability region of the covariance's RK4, so all
    32 windows count) through preintegrate_running, through preintegrate_running_resume as chains cut beside and on the passes,
    and through the ragged route."""
    model, avg = mode
    kn, lin, q = tumbling_windows()
    W, N = kn.shape[0], kn.shape[1] - 1
    a = wdt(kn, lin)
    assert a.max() < 1.3 and (a > 1.0).sum() >= 10 and (a > 0.25).mean() >= 0.4
    ref = trace_rows(model, avg, kn, lin, q)
    dk, dl, dq = _dev(kn, eng), _dev(lin, eng), _dev(q, eng)
    worst = _Worst()
    one_lane = {}
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        for want in _wants(model):
            label = "tumbling m%d avg%d L%d %s" % (model, avg, L, "+".join(want))
            got = _running(eng, prm, want, W, N, knots=dk, lin=dl, q_k_lin=dq)
            _check_rows_rel(got, ref, want, label, worst)
            fin = _host(eng.preintegrate(dk, dl, dq, prm, want=tuple(g for g in want if g != "cov_sym")))
            _check_rel({k: got[k][:, N - 1] for k in _keys(want)}, fin, _keys(want), label + " last row vs preintegrate")
            if L == 1:
                one_lane[want] = got
    worst.report("tumbling windows, preintegrate_running vs oracle.trace, model %d imu_avg %d" % (model, avg))

    worst, bit_equal = _Worst(), []
    for table in ([0, 24, 47], [0, 23, 46, 47])[:model]:
        cuts = np.tile(np.array(table, dtype=np.int64), (W, 1))
        for L in CHAIN_LANES:
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)
            for want in _wants(model):
                segs, _ = _run_chain(eng, prm, kn, lin, q, cuts, want, nan_rows=True)
                _check_chain_rel(segs, ref, cuts, want, "tumbling chain %s m%d avg%d L%d %s" % (table, model, avg, L, "+".join(want)), worst)
                if L == 1:
                    bit_equal.append(("%s %s" % (table, "+".join(want)), _chain_equals_one_shot(segs, one_lane[want], cuts, want)))
    worst.report("tumbling windows, running_resume chains vs oracle.trace, model %d imu_avg %d" % (model, avg))
    print("one-lane chains bit-equal to the one-shot running call: %s" % ", ".join("%s: %s" % be for be in bit_equal))

    worst = _Worst()
    flat, first, count, given = _ragged_layout(kn, 902, garbage=True)
    ref_c = trace_rows(model, avg, kn, lin, q, count)
    for L, want in _requests(model, CHAIN_LANES):
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        got = _running(eng, prm, want, W, N, knots=_dev(flat, eng), lin=dl, q_k_lin=dq, first=_dev(first, eng), count=_dev(given, eng), N=N)
        _check_rows_rel(got, ref_c, want, "tumbling ragged m%d avg%d L%d %s" % (model, avg, L, "+".join(want)), worst)
    worst.report("tumbling windows, ragged route vs oracle.trace, model %d imu_avg %d" % (model, avg))


# --------------------------------------------------------------------------- 5. dynamic range
@pytest.mark.parametrize("dt_scale,w_scale,a_scale", [(0.02, 1.0, 1.0), (1.0, 4.0, 1.0), (4.0, 1.0, 1.0), (1.0, 1.0, 40.0),
                                                      (0.2, 8.0, 10.0)])
def test_running_dynamic_range(eng, dt_scale, w_scale, a_scale):
    """The scalings of test_dynamic_range_stress (50 Hz to 10 kHz, rates up to ~20 rad/s, specific forces up to ~500 m/s^2),
    applied the same way, on every row: relative parity must not depend on the scales."""
    W, N = 64, 29
    kn, lin, q = synth.make_windows(W, N, seed=31337, edge_cases=False)
    kn = kn.clone()
    t0 = kn[:, :1, 0].clone()
    kn[:, :, 0] = t0 + (kn[:, :, 0] - t0) * dt_scale
    kn[:, :, 1:4] *= w_scale
    kn[:, :, 4:7] *= a_scale
    lin = lin.clone()
    lin[:, 0:3] *= w_scale
    lin[:, 3:6] *= a_scale
    kn, lin, q = kn.numpy(), lin.numpy(), q.numpy()
    assert (np.abs(kn[:, :, 1:4]).max() * np.diff(kn[:, :, 0], axis=1).max()) < 1.3
    dk, dl, dq = _dev(kn, eng), _dev(lin, eng), _dev(q, eng)
    for model, avg in [(1, 0), (2, 0), (1, 1)]:
        ref = trace_rows(model, avg, kn, lin, q)
        want = _wants(model)[-1]
        worst = _Worst()
        for L in (0, 1, 5, 64):
            got = _running(eng, eng.make_params(model, bool(avg), lanes_per_window=L), want, W, N, knots=dk, lin=dl, q_k_lin=dq)
            _check_rows_rel(got, ref, want, "scales %g %g %g m%d avg%d L%d" % (dt_scale, w_scale, a_scale, model, avg, L), worst)
        worst.report("scales dt %g w %g a %g, model %d imu_avg %d" % (dt_scale, w_scale, a_scale, model, avg))


# --------------------------------------------------------------------------- 6. long windows
def test_running_long_windows(eng):
    """(a) N = 65535, the documented maximum (16-bit segment lengths in the mean kernel): one window, the gyro reading scaled as
    test_maximum_window_length does, the means of every row.  (b) N = 1000 with covariance rows (72 / 44 passes), one-shot
    and as the chain [0, 400, 700, 1000]."""
    N = 65535
    kn, lin, q = synth.make_windows(1, N, seed=99, edge_cases=False)
    kn = kn.clone()
    kn[:, :, 1:4] *= 0.05                      # keep the 5-minute window's rotation and drift moderate
    kn, lin, q = kn.numpy(), lin.numpy(), q.numpy()
    dk, dl, dq = _dev(kn, eng), _dev(lin, eng), _dev(q, eng)
    for model in (1, 2):
        ref = trace_rows(model, 0, kn, lin, q)
        worst = _Worst()
        for L in (0, 1, 64):
            got = _running(eng, eng.make_params(model, lanes_per_window=L), ("mean",), 1, N, knots=dk, lin=dl, q_k_lin=dq)
            _check_rows_rel(got, ref, ("mean",), "N 65535 m%d L%d" % (model, L), worst)
        worst.report("N = 65535 (|alpha| up to %.2g), model %d" % (np.abs(ref["alpha"]).max(), model))
        del ref
    W, N = 5, 1000
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=1001, edge_cases=True))
    dk, dl, dq = _dev(kn, eng), _dev(lin, eng), _dev(q, eng)
    cuts = np.tile(np.array([0, 400, 700, 1000], dtype=np.int64), (W, 1))
    for model in (1, 2):
        ref = trace_rows(model, 0, kn, lin, q)
        want = _wants(model)[-1]
        worst = _Worst()
        for L in (0, 1, 64):
            prm = eng.make_params(model, lanes_per_window=L)
            got = _running(eng, prm, want, W, N, knots=dk, lin=dl, q_k_lin=dq)
            _check_rows_rel(got, ref, want, "N 1000 m%d L%d" % (model, L), worst)
            segs, _ = _run_chain(eng, prm, kn, lin, q, cuts, want, nan_rows=True)
            _check_chain_rel(segs, ref, cuts, want, "N 1000 chain m%d L%d" % (model, L), worst)
        worst.report("N = 1000 one-shot and 400 + 300 + 300, model %d" % model)
