"""GPU: running preintegration from IMU stream(s), cut in place (cpi_preintegrate_stream_running / _streams_running, their _host
forms, Engine.preintegrate_stream[s]_running[_host], cpi_host::ImuStream::running / ImuStreamSet::running).

Two references.  (a) Bit for bit: Engine.preintegrate_running on the knots / first / count the host assembler
(cpi_amd/stream.py: assemble_windows) cuts from the same stream(s), count clamped to N -- the route a caller had before.
(b) The C restatement's trace, oracle_py.oracle().trace, on every assembled window at the contractual gates of tests/tol.py
(check_pre); the reference's IMU excerpt at the regression gates when the compiled reference (oracle/_ref) is present.

Every row of every window of every case is compared.  The row tensors are pre-filled with NaN (an unwritten row fails every
comparison); the stream and the update times are views into larger device buffers with a sentinel row / stamp on either side,
and every call runs twice, with sentinels +1e300 and -1e300: a read outside the K readings would change a row or a count.
The largest error per field is printed (pytest -s); the figures measured on an MI355X are in profiles/stream_running_bench.md."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import stream as st
from cpi_amd import synth
from oracle import oracle_py as op
from tests.test_gpu_running import JAC, LANES, MEAN, MODES, ZERO_Q, _check_rows, _keys, _wants, _what, _Worst, trace_rows
from tests.test_gpu_streams import _edge_runs, _lin_q, _pack, _ragged, _synth_runs
from tests.test_stream import DATA, _updates
from tests.tol import TOL_FACTOR, check_pre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINELS = (1e300, -1e300)


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _T(a, eng):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _nan_rows(eng, U, N, want, model):
    """[U, N, ...] views of NaN-filled row arrays: a row the call does not write fails every comparison."""
    flat = eng.alloc_outputs(U * N, eng._running_want(tuple(want), model), model)
    for v in flat.values():
        v.fill_(float("nan"))
    return {k: v.view((U, N) + tuple(v.shape[1:])) for k, v in flat.items()}


class _Guarded:
    """The stream [K, 7] and the update times [U] as views into buffers with one sentinel row / stamp on either side."""

    def __init__(self, eng, stream, ut):
        K, U = len(stream), len(ut)
        self.K, self.U = K, U
        self.sbuf = torch.zeros((K + 2, 7), dtype=torch.float64, device=eng.device)
        self.ubuf = torch.zeros((U + 2,), dtype=torch.float64, device=eng.device)
        if K:
            self.sbuf[1:K + 1] = _T(np.asarray(stream).reshape(-1, 7), eng)
        if U:
            self.ubuf[1:U + 1] = _T(ut, eng)
        self.s, self.u = self.sbuf[1:K + 1], self.ubuf[1:U + 1]
        assert self.s.is_contiguous() and self.u.is_contiguous()

    def set(self, sentinel):
        self.sbuf[0] = sentinel; self.sbuf[self.K + 1] = sentinel
        self.ubuf[0] = sentinel; self.ubuf[self.U + 1] = sentinel


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _twice(call, label):
    """call(sentinel) -> (rows dict of numpy arrays, counts); both sentinel runs must agree bit for bit."""
    (r1, c1), (r2, c2) = (call(s) for s in SENTINELS)
    assert np.array_equal(c1, c2), label
    for k in r1:
        assert _bits_equal(r1[k], r2[k]), (label, k, "depends on what lies outside the stream")
        assert np.isfinite(r1[k]).all(), (label, k, "a row was not written")
    return r1, c1


def _stream_rows(eng, g, dl, dq, prm, want, N, label, check_counts=True):
    def call(sentinel):
        g.set(sentinel)
        out, cnt = eng.preintegrate_stream_running(g.s, g.u, dl, dq, prm, want=want, N=N, out=_nan_rows(eng, g.U, N, want, prm.model),
                                                   return_counts=True, check_counts=check_counts)
        return _np(out), cnt.cpu().numpy()
    return _twice(call, label)


def _dense(knots, first, count, N):
    """[U, N + 1, 7] copy of the assembled windows (count clamped to N) for the oracle's trace."""
    U = len(first)
    kn = np.zeros((U, N + 1, 7))
    for u in range(U):
        n = min(int(count[u]), N)
        kn[u, :n + 1] = knots[first[u]:first[u] + n + 1]
        kn[u, n + 1:] = kn[u, n]
    return kn


def _irregular():
    """An update time before the first reading, two equal update times, one exactly on a stamp, one past the end of the stream,
    repeated stamps (dt = 0) inside a window and at a window's start, and one window much longer than the others."""
    s = synth.make_stream(12, 10, seed=77)[0].numpy().copy()
    t = s[:, 0].copy()
    s[1, 0] = t[0]                                           # dt = 0 at the start of the first window that has intervals
    s[20, 0] = t[19]; s[21, 0] = t[19]                       # dt = 0 twice inside a window
    ut = np.array([t[0] - 0.5, t[12] + 0.002, t[12] + 0.002, t[30], t[30] + 0.0213, t[55] + 0.001, t[100] + 0.003, t[-1] + 0.7])
    return s, ut


def _cases():
    out = []
    for name, phase in (("grid", 0.0), ("tails", 0.37)):
        s, u, _, _ = synth.make_stream(70, 9, seed=31, phase=phase)
        out.append((name, s.numpy(), u.numpy(), None))
    kn = st.parse_imu_text(open(DATA).read())
    out.append(("gazebo", kn, _updates(kn), None))
    s, ut = _irregular()
    out.append(("irregular", s, ut, None))
    out.append(("truncated", s, ut, 12))
    return out


CASES = _cases()


def _reference_rows(model, avg, kn, lin, q, count):
    """The compiled reference (oracle/_ref) on every prefix of every window: [U, N, ...] rows, means / Jacobians / P."""
    lib = op.reference()
    prm = op.make_params(model, avg, 1)
    U, n1, _ = kn.shape
    N = n1 - 1
    names = MEAN + (JAC if model == 1 else ()) + ("P",)
    ref = {k: np.zeros((U, N) + ((n,) if n > 1 else ())) for k, n in op.OUT_FIELDS if k in names}
    ref["q"][:, :, 3] = 1.0
    for u in range(U):
        n = min(int(count[u]), N)
        for i in range(n):
            r = lib.run(prm, kn[u:u + 1, :i + 2], lin[u:u + 1], q[u:u + 1])
            for k in names:
                ref[k][u, i] = r[k][0]
        for k in names:
            if n:
                ref[k][u, n:] = ref[k][u, n - 1]
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_stream_running_equals_the_ragged_route_and_the_oracle(eng, mode, case):
    """Items 1-3 of the issue on one stream: bit-identity with preintegrate_running on the host-assembled windows for every
    lanes_per_window and request, the oracle's trace on every row, the exact repeat rules, and the last row against
    preintegrate_stream."""
    model, avg = mode
    name, stream, ut, Nfix = case
    knots, first, count = st.assemble_windows(stream, ut)
    U = len(ut)
    N = int(Nfix or max(1, count.max()))
    clamped = np.minimum(count, N).astype(np.int32)
    lin, q = _lin_q(U, 5)
    kd = _dense(knots, first, count, N)
    ref = trace_rows(model, avg, kd, lin, q, clamped)
    g = _Guarded(eng, stream, ut)
    dl, dq = _T(lin, eng), _T(q, eng)
    ck, cf, cc = _T(knots, eng), _T(first, eng), _T(clamped, eng)
    worst = _Worst()
    # intervals that must repeat the previous row: skipped ones (dt <= 0) and everything from the window's count on
    kt = kd[:, :, 0]
    repeat = [sorted({i for i in range(N) if i >= clamped[u] or not (kt[u, i + 1] - kt[u, i] > 0)}) for u in range(U)]
    if name in ("irregular", "truncated"):
        assert count[0] == 0 and count[2] == 0 and count.max() > 12 and any(0 in r and clamped[u] > 0 for u, r in enumerate(repeat))
        with pytest.raises(ValueError, match="more than N"):
            eng.preintegrate_stream_running(g.s, g.u, dl, dq, eng.make_params(model), want=("mean",), N=int(count.max()) - 1)
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        for want in _wants(model):
            label = "%s m%d avg%d L%d %s" % (name, model, avg, L, "+".join(want))
            got, cnt = _stream_rows(eng, g, dl, dq, prm, want, N, label, check_counts=Nfix is None)
            assert np.array_equal(cnt, count), label                 # the TRUE counts, truncated windows included
            rag = _np(eng.preintegrate_running(ck, dl, dq, prm, want=want, first=cf, count=cc, N=N))
            assert sorted(got) == sorted(rag)
            for k in rag:
                assert np.array_equal(got[k], rag[k]), (label, k)
            _check_rows(got, ref, want, label, worst)
            for k in got:
                zero = ZERO_Q if k == "q" else np.zeros(got[k].shape[2:])
                for u in range(U):
                    for i in repeat[u]:
                        assert np.array_equal(got[k][u, i], got[k][u, i - 1] if i > 0 else zero), (label, k, u, i)
            # the window's measurement: row N - 1 of every window that was not truncated
            fin = _np(eng.preintegrate_stream(g.s, g.u, dl, dq, prm, want=tuple(w for w in want if w != "cov_sym"), N=N,
                                              check_counts=False))
            keep = count <= N
            check_pre({k: got[k][keep, N - 1] for k in _keys(want)}, {k: fin[k][keep] for k in _keys(want)}, what=_what(want),
                      label=label + " last row vs preintegrate_stream")
    worst.report("stream rows vs oracle.trace, %s, model %d imu_avg %d" % (name, model, avg))
    if name == "gazebo" and op.reference() is not None:
        reg = _reference_rows(model, avg, kd, lin, q, clamped)
        w2 = _Worst()
        for want in _wants(model):
            got, _ = _stream_rows(eng, g, dl, dq, eng.make_params(model, bool(avg)), want, N, "gazebo regression")
            _check_rows(got, reg, want, "gazebo vs the compiled reference m%d avg%d" % (model, avg), w2, regression=True)
        w2.report("stream rows vs the compiled reference, gazebo, model %d imu_avg %d" % (model, avg))


@pytest.mark.parametrize("mode", MODES)
def test_stream_running_on_both_sides_of_the_launch_policy(eng, mode):
    """The automatic lane choice is the same function of (U, N, request) as in preintegrate_running: N = 4 (no tails) and N = 5
    (tails), one window, one wavefront, 1 024 wavefronts of two lanes per window -1 / exactly / +1 window.  Means only at the
    large sizes (a dense-P row is 2 248 bytes); the oracle's trace on the first 64 windows."""
    model, avg = mode
    prm = eng.make_params(model, bool(avg))
    worst = _Worst()
    for phase in (0.0, 0.37):
        s, u, lin, q = (t.numpy() for t in synth.make_stream(32769, 4, seed=41, phase=phase))
        for U in (1, 31, 32, 33, 32767, 32768, 32769):
            ut = u[:U]
            knots, first, count = st.assemble_windows(s, ut)
            N = int(count.max())
            g = _Guarded(eng, s, ut)
            dl, dq = _T(lin[:U], eng), _T(q[:U], eng)
            ck, cf, cc = _T(knots, eng), _T(first, eng), _T(count, eng)
            for want in (_wants(model) if U <= 33 else [("mean",)]):
                label = "policy phase %g m%d avg%d U%d %s" % (phase, model, avg, U, "+".join(want))
                got, cnt = _stream_rows(eng, g, dl, dq, prm, want, N, label)
                assert np.array_equal(cnt, count), label
                rag = _np(eng.preintegrate_running(ck, dl, dq, prm, want=want, first=cf, count=cc, N=N))
                for k in rag:
                    assert np.array_equal(got[k], rag[k]), (label, k)
                V = min(U, 64)
                ref = trace_rows(model, avg, _dense(knots, first[:V], count[:V], N), lin[:V], q[:V], count[:V],
                                 key=("spolicy", phase, V))
                _check_rows({k: v[:V] for k, v in got.items()}, ref, want, label, worst)
    worst.report("stream rows at the launch-policy switches, model %d imu_avg %d" % (model, avg))


def _many_runs():
    runs = _synth_runs([(9, 10, 0.37), (4, 10, 0.0), (6, 7, 0.6)], seed=5)
    runs[1:1] = _edge_runs()                                  # runs of 0, 1, 2, 3 readings, no update times, gaps, repeated updates
    return runs


@pytest.mark.parametrize("mode", MODES)
def test_streams_running_many_runs(eng, mode):
    """Runs of unequal length whose clocks restart at 0: the whole call equals preintegrate_running on the concatenated
    host-assembled windows bit for bit (automatic lanes included); every run equals the single-stream call on that run alone
    at pinned lane counts; a bound smaller than the longest window truncates as the single-stream entry does."""
    model, avg = mode
    runs = _many_runs()
    stream, so, ut, uo = _pack(runs)
    knots, first, count = _ragged(runs)
    U = len(ut)
    lin, q = _lin_q(U, 21)
    g = _Guarded(eng, stream, ut)
    dl, dq = _T(lin, eng), _T(q, eng)
    ck, cf = _T(knots, eng), _T(first, eng)
    worst = _Worst()
    for N in (int(count.max()), 4):
        clamped = np.minimum(count, N).astype(np.int32)
        cc = _T(clamped, eng)
        ref = trace_rows(model, avg, _dense(knots, first, count, N), lin, q, clamped)
        for L in (0, 1, 2, 3, 5, 8, 16, 64):
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)
            for want in _wants(model):
                label = "runs m%d avg%d N%d L%d %s" % (model, avg, N, L, "+".join(want))

                def call(sentinel):
                    g.set(sentinel)
                    out, cnt = eng.preintegrate_streams_running(g.s, so, g.u, uo, dl, dq, prm, want=want, N=N, return_counts=True,
                                                                out=_nan_rows(eng, U, N, want, model), check_counts=False)
                    return _np(out), cnt.cpu().numpy()
                got, cnt = _twice(call, label)
                assert np.array_equal(cnt, count), label
                rag = _np(eng.preintegrate_running(ck, dl, dq, prm, want=want, first=cf, count=cc, N=N))
                for k in rag:
                    assert np.array_equal(got[k], rag[k]), (label, k)
                _check_rows(got, ref, want, label, worst)
                if L == 0:
                    continue
                for r, (s, u) in enumerate(runs):
                    a, b = int(uo[r]), int(uo[r + 1])
                    if a == b:
                        continue
                    if len(s) == 0:                          # a run without readings: N zero-state rows per window
                        for k in got:
                            zero = ZERO_Q if k == "q" else np.zeros(got[k].shape[2:])
                            assert np.array_equal(got[k][a:b], np.broadcast_to(zero, got[k][a:b].shape)), (label, r, k)
                        assert not cnt[a:b].any()
                        continue
                    g1 = _Guarded(eng, s, u)
                    one, c1 = _stream_rows(eng, g1, dl[a:b].contiguous(), dq[a:b].contiguous(), prm, want, N, label + " run %d" % r,
                                           check_counts=False)
                    assert np.array_equal(cnt[a:b], c1), (label, r)
                    for k in one:
                        assert np.array_equal(got[k][a:b], one[k]), (label, r, k)
    worst.report("multi-stream rows vs oracle.trace, model %d imu_avg %d" % (model, avg))
    # the list-of-runs form of preintegrate_streams, default N (streams_bound) and the count check
    prm = eng.make_params(model, bool(avg), lanes_per_window=1)
    lst = eng.preintegrate_streams_running([_T(s, eng).reshape(-1, 7) for s, _ in runs], None, [_T(u, eng) for _, u in runs], None,
                                           dl, dq, prm, want=("mean",))
    Nb = lst["DT"].shape[1]
    assert Nb >= count.max()
    same = _np(eng.preintegrate_streams_running(g.s, so, g.u, uo, dl, dq, prm, want=("mean",), N=Nb))
    for k, v in _np(lst).items():
        assert np.array_equal(v, same[k]), k
    with pytest.raises(ValueError, match="more than N"):
        eng.preintegrate_streams_running(g.s, so, g.u, uo, dl, dq, prm, want=("mean",), N=4)
    with pytest.raises(ValueError, match="explicit N"):
        eng.preintegrate_streams_running(g.s, so, g.u, uo, dl, dq, prm, want=("mean",), check_counts=False)
    with pytest.raises(ValueError, match="explicit N"):
        eng.preintegrate_stream_running(g.s, g.u, dl, dq, prm, want=("mean",), check_counts=False)


def test_streams_running_wrong_device_offsets_are_clamped(eng):
    """The cases of test_gpu_streams_wrong_device_offsets_are_clamped through the running entry: offsets the device entry
    cannot validate give wrong windows, never a read outside the stream -- the two sentinel runs agree bit for bit and the counts
    stay in [0, K]; the _host form refuses the same offsets."""
    from cpi_amd import CpiError
    runs = _synth_runs([(10, 10, 0.3), (5, 10, 0.0), (8, 10, 0.5)], seed=8)
    stream, so, ut, uo = _pack(runs)
    U, K = len(ut), len(stream)
    lin, _ = _lin_q(U, 3)
    dl = _T(lin, eng)
    g = _Guarded(eng, stream, ut)
    N = 12
    cases = (([0, K + 500, 3, K + 9], uo), (so, [0, -4, U + 100, U]), ([-9, 5, 2, 1 << 40], [1 << 40, 2, 1, -3]),
             (so, [-1, 5, 9, U]), ([0, K], [-1, U]), ([-5, K + 3], [-7, U + 2]))
    for s2, u2 in cases:
        s2, u2 = np.asarray(s2, np.int64), np.asarray(u2, np.int64)
        for lanes in (0, 1, 3):
            prm = eng.make_params(1, lanes_per_window=lanes)
            for want in (("mean",), ("mean", "jac", "cov")):
                label = "offsets %s %s L%d %s" % (s2.tolist(), u2.tolist(), lanes, "+".join(want))

                def call(sentinel):
                    g.set(sentinel)
                    out, cnt = eng.preintegrate_streams_running(g.s, s2, g.u, u2, dl, None, prm, want=want, N=N, return_counts=True,
                                                                out=_nan_rows(eng, U, N, want, 1), check_counts=False)
                    return _np(out), cnt.cpu().numpy()
                _, cnt = _twice(call, label)
                assert cnt.min() >= 0 and cnt.max() <= K, label
        with pytest.raises(CpiError, match="offsets"):
            eng.preintegrate_streams_running_host(torch.from_numpy(stream), s2, torch.from_numpy(ut), u2, torch.from_numpy(lin), None,
                                                  eng.make_params(1), want=("mean",), N=N)


@pytest.mark.parametrize("model", [1, 2])
def test_stream_running_rows_feed_predict(eng, model):
    """Engine.predict on the reshaped stream rows (F = U N, idx_i[row] = row // N) = oracle.predict on the trace rows."""
    s, u, lin, q = (t.numpy() for t in synth.make_stream(37, 12, seed=16, phase=0.41))
    knots, first, count = st.assemble_windows(s, u)
    U, N = len(u), int(count.max())
    ref = trace_rows(model, 0, _dense(knots, first, count, N), lin, q, count)
    dl = _T(lin, eng)
    rows = eng.preintegrate_stream_running(_T(s, eng), _T(u, eng), dl, _T(q, eng), eng.make_params(model), want=("mean",), N=N)
    meas = {k: v.reshape((U * N,) + tuple(v.shape[2:])) for k, v in rows.items()}
    zeros = torch.zeros((U, 3), dtype=torch.float64, device=eng.device)
    xi, _ = synth.make_states(zeros, zeros, torch.tensor([[0.0, 0, 0, 1]] * U, dtype=torch.float64, device=eng.device), zeros[:, 0], dl,
                              model, device=eng.device)
    idx = (torch.arange(U * N, device=eng.device) // N).to(torch.int32)
    got = eng.predict(model, meas, xi, idx_i=idx)
    torch.cuda.synchronize()
    flat = {k: ref[k].reshape((U * N,) + ref[k].shape[2:]) for k in MEAN}
    for k in JAC + (("O_a", "O_b") if model == 2 else ()):
        flat[k] = np.zeros((U * N, 9))                      # predict reads DT, alpha, beta, q only
    sel = np.repeat(np.arange(U), N)
    rec = op.factor_records(flat, lin[sel], q[sel] if model == 2 else None)
    want = op.oracle().predict(model, rec, xi.cpu().numpy()[sel])
    assert np.abs(got.cpu().numpy() - want).max() <= TOL_FACTOR * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("mode", MODES)
def test_stream_running_host_entries(eng, mode):
    """The _host forms (pinned and pageable memory) equal the device entries bit for bit at a pinned lanes_per_window and return
    the true counts; a call whose rows come back in several chunks (> 2^18 rows) equals the device entry too."""
    model, avg = mode
    prm = eng.make_params(model, bool(avg), lanes_per_window=2)
    want = _wants(model)[-1]
    s, ut = _irregular()
    _, _, count = st.assemble_windows(s, ut)
    U = len(ut)
    lin, q = _lin_q(U, 8)
    ts, tu, tl, tq = (torch.from_numpy(np.ascontiguousarray(a)) for a in (s, ut, lin, q))
    for N in (int(count.max()), 12):
        dev, dc = eng.preintegrate_stream_running(_T(s, eng), _T(ut, eng), _T(lin, eng), _T(q, eng), prm, want=want, N=N,
                                                  return_counts=True, check_counts=False)
        dev = _np(dev)
        for pinned in (False, True):
            got, cnt = eng.preintegrate_stream_running_host(ts, tu, tl, tq, prm, want=want, N=N, pinned=pinned, return_counts=True,
                                                            check_counts=False)
            assert np.array_equal(cnt.numpy(), count) and np.array_equal(dc.cpu().numpy(), count)
            assert sorted(got) == sorted(dev)
            for k in dev:
                assert np.array_equal(got[k].numpy(), dev[k]), (k, N, pinned)
    with pytest.raises(ValueError, match="N = 12"):
        eng.preintegrate_stream_running_host(ts, tu, tl, tq, prm, want=("mean",), N=12)
    runs = _many_runs()
    stream, so, uts, uo = _pack(runs)
    _, _, rcount = _ragged(runs)
    lin, q = _lin_q(len(uts), 9)
    N = int(rcount.max())
    dev = _np(eng.preintegrate_streams_running(_T(stream, eng), so, _T(uts, eng), uo, _T(lin, eng), _T(q, eng), prm, want=want, N=N))
    for pinned in (False, True):
        got, cnt = eng.preintegrate_streams_running_host(torch.from_numpy(stream), so, torch.from_numpy(uts), uo, torch.from_numpy(lin),
                                                         torch.from_numpy(q), prm, want=want, N=N, pinned=pinned, return_counts=True)
        assert np.array_equal(cnt.numpy(), rcount)
        for k in dev:
            assert np.array_equal(got[k].numpy(), dev[k]), (k, pinned)
    # N=None: the default bounds of the host forms (the longest window the stamps allow) -- the device entry's rows at that N
    got = eng.preintegrate_stream_running_host(ts, tu, tl, tq, prm, want=want)
    Nd = got["DT"].shape[1]
    assert int(count.max()) <= Nd <= int(count.max()) + 1
    dev = _np(eng.preintegrate_stream_running(_T(s, eng), _T(ut, eng), _T(tl.numpy(), eng), _T(tq.numpy(), eng), prm, want=want, N=Nd))
    for k in dev:
        assert np.array_equal(got[k].numpy(), dev[k]), (k, "default N")
    got = eng.preintegrate_streams_running_host(torch.from_numpy(stream), so, torch.from_numpy(uts), uo, torch.from_numpy(lin),
                                                torch.from_numpy(q), prm, want=want)
    Nd = got["DT"].shape[1]
    assert int(rcount.max()) <= Nd <= int(rcount.max()) + 1
    dev = _np(eng.preintegrate_streams_running(_T(stream, eng), so, _T(uts, eng), uo, _T(lin, eng), _T(q, eng), prm, want=want, N=Nd))
    for k in dev:
        assert np.array_equal(got[k].numpy(), dev[k]), (k, "default N, runs")
    # long windows: a chunk holds fewer than 64 windows (2^18 / 5 000 = 52), three chunks, the last one short; means only
    s, u, lin, q = synth.make_stream(130, 4999, seed=24, phase=0.6)
    got, cnt = eng.preintegrate_stream_running_host(s, u, lin, q, prm, want=("mean",), N=5000, return_counts=True)
    assert int(cnt.max()) == 5000
    dev = _np(eng.preintegrate_stream_running(s.to(eng.device), u.to(eng.device), lin.to(eng.device), q.to(eng.device), prm,
                                              want=("mean",), N=5000))
    for k in dev:
        assert np.array_equal(got[k].numpy(), dev[k]), (k, "52-window chunks")
    # several chunks: 6 000 windows x 51 rows, means only
    s, u, lin, q = synth.make_stream(6000, 50, seed=23, phase=0.2)
    assert 6000 * 51 > (1 << 18)
    got = eng.preintegrate_stream_running_host(s, u, lin, q, prm, want=("mean",), N=51)
    dev = _np(eng.preintegrate_stream_running(s.to(eng.device), u.to(eng.device), lin.to(eng.device), q.to(eng.device), prm,
                                              want=("mean",), N=51))
    for k in dev:
        assert np.array_equal(got[k].numpy(), dev[k]), k


def test_stream_running_argument_checks(eng):
    from cpi_amd import CpiError
    s, u, lin, q = synth.make_stream(8, 5, seed=19, device=eng.device, phase=0.3)
    N = 6
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_stream_running(s, u, lin, q, eng.make_params(3), want=("mean",), N=N)
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_stream_running(s, u, lin, q, eng.make_params(2), want=("mean", "jac"), N=N)
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_streams_running(s, [0, s.shape[0]], u, [0, 8], lin, q, eng.make_params(3), want=("mean",), N=N)
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_streams_running(s, [0, s.shape[0]], u, [0, 8], lin, q, eng.make_params(2), want=("jac",), N=N)
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_stream_running_host(s.cpu(), u.cpu(), lin.cpu(), q.cpu(), eng.make_params(3), want=("mean",), N=N)
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_streams_running_host(s.cpu(), [0, s.shape[0]], u.cpu(), [0, 8], lin.cpu(), q.cpu(), eng.make_params(2),
                                              want=("jac",), N=N)
    with pytest.raises(CpiError, match="q_k_lin"):
        eng.preintegrate_stream_running(s, u, lin, None, eng.make_params(2), want=("mean",), N=N)
    with pytest.raises(CpiError, match="lanes_per_window"):
        eng.preintegrate_stream_running(s, u, lin, q, eng.make_params(1, lanes_per_window=7), want=("mean",), N=N)
    dt = {"DT": torch.zeros((8, 65536), dtype=torch.float64, device=eng.device)}
    with pytest.raises(CpiError, match="65535"):
        eng.preintegrate_stream_running(s, u, lin, q, eng.make_params(1), N=65536, out=dt, check_counts=False)
    with pytest.raises(CpiError, match="the stream is empty"):
        eng.preintegrate_stream_running(s[:0], u, lin, q, eng.make_params(1), want=("mean",), N=N)
    with pytest.raises(CpiError, match="no run"):
        eng.preintegrate_streams_running(s, [0], u, [0], lin, q, eng.make_params(1), want=("mean",), N=N)
    with pytest.raises(CpiError, match="hold no reading"):
        eng.preintegrate_streams_running(s[:0], [0, 0], u, [0, 8], lin, q, eng.make_params(1), want=("mean",), N=N)
    # NULL workspace / stream / update_times / lin / rows, straight through the C entry
    import ctypes as C
    from cpi_amd._lib import CpiOutputs
    from cpi_amd.engine import _ptr
    lib, prm = eng.lib, eng.make_params(1)
    ws = eng.stream_workspace(8)
    o = CpiOutputs()
    full = [eng.ctx, C.byref(prm), s.shape[0], _ptr(s), 8, _ptr(u), N, _ptr(lin), _ptr(q), _ptr(ws), C.byref(o)]
    for i, word in ((3, "NULL argument"), (5, "NULL argument"), (7, "NULL argument"), (9, "NULL argument"), (10, "prm/rows is NULL")):
        a = list(full)
        a[i] = None
        assert lib.cpi_preintegrate_stream_running(*a) == 1
        assert word in lib.cpi_last_error(eng.ctx).decode(), (i, lib.cpi_last_error(eng.ctx))
    # the multi-stream entry: NULL offsets, stream, update_times, lin, workspace, rows
    so, uo = (torch.tensor(v, dtype=torch.int64, device=eng.device) for v in ([0, s.shape[0]], [0, 8]))
    fullm = [eng.ctx, C.byref(prm), 1, s.shape[0], _ptr(s), _ptr(so), 8, _ptr(u), _ptr(uo), N, _ptr(lin), _ptr(q), _ptr(ws), C.byref(o)]
    for i, word in ((4, "NULL argument"), (5, "NULL argument"), (7, "NULL argument"), (8, "NULL argument"), (10, "NULL argument"),
                    (12, "NULL argument"), (13, "prm/rows is NULL")):
        a = list(fullm)
        a[i] = None
        assert lib.cpi_preintegrate_streams_running(*a) == 1
        assert word in lib.cpi_last_error(eng.ctx).decode(), (i, lib.cpi_last_error(eng.ctx))
    assert lib.cpi_preintegrate_streams_running(*fullm) == 0       # the complete argument list is accepted (nothing asked for: counts only)
    # the _host forms: NULL arguments, K == 0, R == 0, N > 65535, by message
    hs, hu, hl, hq = (t.cpu().contiguous() for t in (s, u, lin, q))
    hso, huo = so.cpu(), uo.cpu()
    cnt = torch.zeros((8,), dtype=torch.int32)
    fullh = [eng.ctx, C.byref(prm), hs.shape[0], _ptr(hs), 8, _ptr(hu), N, _ptr(hl), _ptr(hq), C.byref(o), _ptr(cnt)]
    for i, word in ((3, "NULL argument"), (5, "NULL argument"), (7, "NULL argument"), (9, "prm/rows is NULL")):
        a = list(fullh)
        a[i] = None
        assert lib.cpi_preintegrate_stream_running_host(*a) == 1
        assert word in lib.cpi_last_error(eng.ctx).decode(), (i, lib.cpi_last_error(eng.ctx))
    for i, val, word in ((2, 0, "the stream is empty"), (6, 65536, "65535")):
        a = list(fullh)
        a[i] = val
        assert lib.cpi_preintegrate_stream_running_host(*a) == 1
        assert word in lib.cpi_last_error(eng.ctx).decode(), (i, lib.cpi_last_error(eng.ctx))
    fullhm = [eng.ctx, C.byref(prm), 1, hs.shape[0], _ptr(hs), _ptr(hso), 8, _ptr(hu), _ptr(huo), N, _ptr(hl), _ptr(hq), C.byref(o), _ptr(cnt)]
    for i, val, word in ((4, None, "NULL argument"), (5, None, "NULL argument"), (7, None, "NULL argument"), (8, None, "NULL argument"),
                         (10, None, "NULL argument"), (12, None, "prm/rows is NULL"), (2, 0, "no run"), (3, 0, "hold no reading"),
                         (9, 65536, "65535")):
        a = list(fullhm)
        a[i] = val
        assert lib.cpi_preintegrate_streams_running_host(*a) == 1
        assert word in lib.cpi_last_error(eng.ctx).decode(), (i, lib.cpi_last_error(eng.ctx))
    with pytest.raises(CpiError, match="q_k_lin"):
        eng.preintegrate_stream_running_host(hs, hu, hl, None, eng.make_params(2), want=("mean",), N=N)
    with pytest.raises(CpiError, match="lanes_per_window"):
        eng.preintegrate_streams_running_host(hs, hso, hu, huo, hl, hq, eng.make_params(1, lanes_per_window=7), want=("mean",), N=N)
    # U == 0 and N == 0 are no-ops (the workspace included); the default want of model 2 asks for no Jacobians
    sent = {"DT": torch.full((4,), 3.0, dtype=torch.float64, device=eng.device)}
    ws.fill_(5.0)
    eng.preintegrate_stream_running(s, u[:0], lin[:0], q[:0], eng.make_params(1), N=N, out=sent, workspace=ws)
    eng.preintegrate_stream_running(s, u, lin, q, eng.make_params(1), N=0, out=sent, workspace=ws, check_counts=False)
    torch.cuda.synchronize()
    assert torch.all(sent["DT"] == 3.0) and torch.all(ws == 5.0)
    assert sorted(eng.preintegrate_stream_running(s, u, lin, q, eng.make_params(2), N=N)) == sorted(MEAN + ("P",))
    assert eng.lib.cpi_abi_version() == 3


def test_stream_running_graph_capture_and_replay(eng):
    """The device entry captured on a single stream (cut kernel, mean kernel, covariance kernel: a chain, no parallel
    branches); a replay with new readings in the same buffers equals an eager call."""
    s, u, lin, q = synth.make_stream(300, 20, seed=17, device=eng.device, phase=0.37)
    U, N = 300, 21
    for model in (1, 2):
        prm = eng.make_params(model)
        want = _wants(model)[-1]
        ws = eng.stream_workspace(U)
        out = eng.preintegrate_stream_running(s, u, lin, q, prm, want=want, N=N, workspace=ws)

        def call():
            eng.preintegrate_stream_running(s, u, lin, q, prm, want=want, N=N, out=out, workspace=ws, check_counts=False)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            call()                                          # warm-up on the side stream, as graph capture requires
        torch.cuda.synchronize()
        eager = {k: v.clone() for k, v in out.items()}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for v in out.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], eager[k]), k
        s[:, 1:4] *= 1.01                                   # new measurements in the same buffers
        g.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        call()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], replayed[k]), k
            assert k == "DT" or not torch.equal(out[k], eager[k]), k    # (the stamps did not change)


@pytest.mark.parametrize("model", [1, 2])
def test_stream_running_cpp_facade(eng, model):
    """tests/cpp/test_stream_running.cpp: cpi_host::ImuStream::running and ImuStreamSet::running against the per-window
    CpiBatch::running results on the host-assembled windows (compared inside the program, bit for bit), the tight default bound,
    and the refusal of a bound smaller than the longest window."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    runs = [(s, u) for s, u in _many_runs() if len(s)]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_stream_running")
        subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_stream_running.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        path = os.path.join(tmp, "runs.txt")
        total = 0
        with open(path, "w") as f:
            f.write("%d\n" % len(runs))
            for s, u in runs:
                f.write("%d %d\n" % (len(s), len(u)))
                for row in s:
                    f.write(" ".join("%.17g" % v for v in row) + "\n")
                f.write(" ".join("%.17g" % v for v in u) + "\n")
                if len(u):
                    total += int(st.assemble_windows(s, u)[2].sum())
        for avg in (0, 1):
            p = subprocess.run([exe, path, str(model), str(avg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            assert p.returncode == 0, p.stdout + p.stderr
            assert "OK rows %d" % total in p.stdout, p.stdout
