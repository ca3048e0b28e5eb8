"""GPU: running preintegration (cpi_preintegrate_running, Engine.preintegrate_running[_host], cpi_host::CpiBatch::running) --
the measurement after EVERY interval.

Reference for every row: the C restatement's trace, oracle_py.oracle().trace(prm, knots[w], lin[w], q[w]) (the state after each
feed_IMU), at the contractual gates of tests/tol.py (TOL_MEAN 1e-9, TOL_JAC 1e-8, TOL_COV 1e-6 via check_pre); the pinned
traces of the compiled reference (tests/golden/trace_v*.npz) at the regression gates.  No row is left out: every row of every
window of every case is compared, rows past a window's count with the window's final state.  The largest error per field of a
test is printed (pytest -s); the figures measured on an MI355X are in profiles/running_bench.md."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import synth
from oracle import oracle_py as op
from tests.tol import TOL_FACTOR, check_pre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]
LANES = [0, 1, 2, 3, 4, 5, 6, 8, 12, 16, 32, 64]      # 0 = automatic; the others: include/cpi_amd.h, lanes_per_window
MEAN = ("DT", "alpha", "beta", "q")
JAC = ("J_q", "J_a", "J_b", "H_a", "H_b")
ZERO_Q = np.array([0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _dev(a, eng):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _wants(model):
    """means only / means + Jacobians / everything (model 2 has no running Jacobians)"""
    return [("mean",), ("mean", "jac"), ("mean", "jac", "cov", "cov_sym")] if model == 1 else [("mean",), ("mean", "cov", "cov_sym")]


def _what(want):
    return tuple(g for g in ("mean", "jac", "cov") if g in want)


def _keys(want):
    return (MEAN if "mean" in want else ()) + (JAC if "jac" in want else ()) + (("P",) if "cov" in want else ())


_trace_cache = {}


def trace_rows(model, avg, kn, lin, q, count=None, key=None):
    """[W, N, ...] rows of the oracle's trace; window w is cut at count[w] (clamped into [0, N]) and the rows from there on
    repeat its final state (count 0: the zero state)."""
    if key is not None and (key, model, avg) in _trace_cache:
        return _trace_cache[(key, model, avg)]
    W, n1, _ = kn.shape
    N = n1 - 1
    prm = op.make_params(model, avg, 1)
    names = MEAN + JAC + ("P",)
    ref = {k: np.zeros((W, N) + ((n,) if n > 1 else ())) for k, n in op.OUT_FIELDS if k in names}
    ref["q"][:, :, 3] = 1.0
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
        _trace_cache[(key, model, avg)] = ref
    return ref


class _Worst:
    def __init__(self):
        self.e = {}

    def add(self, got, ref, keys):
        for k in keys:
            self.e[k] = max(self.e.get(k, 0.0), float(np.abs(got[k] - ref[k]).max()))

    def report(self, label):
        print("%s: largest error per field: %s" % (label, ", ".join("%s %.2e" % kv for kv in sorted(self.e.items()))))


def _flat(d):
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in d.items()}


def _check_rows(got, ref, want, label, worst=None, regression=False):
    check_pre(_flat({k: got[k] for k in _keys(want)}), _flat({k: ref[k] for k in _keys(want)}), what=_what(want), label=label,
              regression=regression)
    if worst is not None:
        worst.add(got, ref, _keys(want))
    if "cov_sym" in want and "cov" in want:      # P_sym: bit for bit the upper triangle of the P row
        from cpi_amd.engine import pack_sym
        P = torch.from_numpy(got["P"].reshape(-1, 225))
        assert np.array_equal(pack_sym(P).numpy(), got["P_sym"].reshape(-1, 120)), label + " P_sym"


def _ragged(W, N, seed, garbage=False):
    """A ragged batch over one knot array: window w starts at first[w] (windows in shuffled order, a gap of unused knots between
    them) and has count[w] intervals; returns the dense view [W, N + 1, 7] the reference reads as well."""
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=seed))
    return (kn, lin, q) + _ragged_layout(kn, seed, garbage)


def _ragged_layout(kn, seed, garbage=False):
    """The layout of _ragged over the dense knots kn [W, N + 1, 7]: flat, first, count, given."""
    W, N = kn.shape[0], kn.shape[1] - 1
    rng = np.random.default_rng(seed)
    count = rng.integers(0, N + 1, size=W).astype(np.int32)
    count[:4] = [0, N, 1, max(N - 1, 0)][:min(4, W)]
    order = rng.permutation(W)
    stride = N + 3
    flat = np.full((W * stride + 2, 7), np.nan)            # what no window owns is NaN: a read of it would poison a row
    first = np.zeros(W, dtype=np.int64)
    for slot, w in enumerate(order):
        first[w] = 1 + slot * stride
        flat[first[w]:first[w] + count[w] + 1] = kn[w, :count[w] + 1]
    given = count.copy()
    if garbage:                                             # counts outside [0, N] are clamped into it
        given[1::5] = np.where(count[1::5] == N, N + 1 + np.arange(len(count[1::5])) * 1000, given[1::5])
        given[0::7] = np.where(count[0::7] == 0, -1 - np.arange(len(count[0::7])), given[0::7])
    return flat, first, count, given


@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("mode", MODES)
def test_running_rows_match_the_oracle_trace(eng, mode, layout):
    """Every row, every lanes_per_window the header lists plus auto, means only / + Jacobians / everything with P and P_sym;
    the last row against Engine.preintegrate on the same inputs at the same gates."""
    model, avg = mode
    W, N = 203, 20                                          # not a multiple of the windows per wavefront of any lane count
    if layout == "dense":
        kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=11))
        count = None
        args = dict(knots=_dev(kn, eng))
    else:
        kn, lin, q, flat, first, count, given = _ragged(W, N, 12, garbage=True)
        args = dict(knots=_dev(flat, eng), first=_dev(first, eng), count=_dev(given, eng), N=N)
    ref = trace_rows(model, avg, kn, lin, q, count)
    dl, dq = _dev(lin, eng), _dev(q, eng)
    worst, bit_equal = _Worst(), []
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        for want in _wants(model):
            label = "m%d avg%d %s L%d %s" % (model, avg, layout, L, "+".join(want))
            got = _host(eng.preintegrate_running(lin=dl, q_k_lin=dq, params=prm, want=want, **args))
            assert all(v.shape[:2] == (W, N) for v in got.values())
            _check_rows(got, ref, want, label, worst)
            bwant = tuple(g for g in want if g != "cov_sym")
            fin = _host(eng.preintegrate(lin=dl, q_k_lin=dq, params=prm, want=bwant, **args))
            last = {k: got[k][:, N - 1] for k in _keys(want)}
            check_pre(last, fin, what=_what(want), label=label + " last row vs preintegrate")
            if L == 1:
                bit_equal.append((want, all(np.array_equal(last[k], fin[k]) for k in _keys(want))))
    worst.report("running vs oracle.trace, model %d imu_avg %d %s" % (model, avg, layout))
    print("last row bit-equal to Engine.preintegrate at lanes_per_window = 1: %s"
          % ", ".join("%s: %s" % ("+".join(w), e) for w, e in bit_equal))


def test_running_matches_the_golden_traces(eng, golden_dir):
    """The compiled reference's own traces, every row, regression gates."""
    worst = _Worst()
    for model in (1, 2):
        d = np.load(os.path.join(golden_dir, "trace_v%d.npz" % model))
        ref = {k: d[k][None] for k in MEAN + JAC + ("P",)}
        kn, lin, q = (_dev(d[k][None], eng) for k in ("knots", "lin", "q_k_lin"))
        for L in LANES:
            for want in _wants(model):
                got = _host(eng.preintegrate_running(kn, lin, q, eng.make_params(model, lanes_per_window=L), want=want))
                _check_rows(got, ref, want, "golden m%d L%d %s" % (model, L, "+".join(want)), worst, regression=True)
    worst.report("running vs golden traces")


@pytest.mark.parametrize("mode", MODES)
def test_running_on_both_sides_of_the_launch_policy(eng, mode):
    """Automatic lane choice at N = 4 (choices: 1 and 2 lanes): one window, one wavefront, 1 024 wavefronts of two lanes per
    window -1 / exactly / +1 window (the last is the one-lane kernel: a batch large enough for L = 1)."""
    model, avg = mode
    N, Wmax = 4, 32769
    kn, lin, q = (t.numpy() for t in synth.make_windows(Wmax, N, seed=13))
    ref = trace_rows(model, avg, kn, lin, q, key="policy")
    prm = eng.make_params(model, bool(avg))
    worst = _Worst()
    for W in (1, 31, 32, 33, 32767, 32768, 32769):
        for want in _wants(model):
            got = _host(eng.preintegrate_running(_dev(kn[:W], eng), _dev(lin[:W], eng), _dev(q[:W], eng), prm, want=want))
            _check_rows(got, {k: v[:W] for k, v in ref.items()}, want, "policy m%d avg%d W%d %s" % (model, avg, W, "+".join(want)), worst)
    worst.report("running at the launch-policy switches, model %d imu_avg %d" % (model, avg))


def _skipping_windows(N, seed):
    """Windows with repeated stamps (interval 0, a middle one and its neighbour), a stamp that steps back, and a NaN-stamp
    separator knot; returns the batch and, per window, the intervals that must repeat the previous row."""
    kn, lin, q = (t.numpy() for t in synth.make_windows(64, N, seed=seed, edge_cases=False))
    kn = kn.copy()
    skipped = []
    for w in range(64):
        s, kind = [], w % 4
        if kind == 0:
            for i in sorted({0, (w // 4) % N, min(N - 1, (w // 4) % N + 1)}):
                kn[w, i + 1:, 0] -= kn[w, i + 1, 0] - kn[w, i, 0]
                s.append(i)
        elif kind == 1:
            i = (w // 4) % N
            kn[w, i + 1:, 0] -= 2.0 * (kn[w, i + 1, 0] - kn[w, i, 0])
            s.append(i)
        elif kind == 2:
            i = 1 + (w // 4) % (N - 1)
            kn[w, i] = 0.0
            kn[w, i, 0] = np.nan
            s += [i - 1, i]
        skipped.append([i for i in s if i < N])
    return kn, lin, q, skipped


@pytest.mark.parametrize("mode", MODES)
def test_running_repeat_rows_are_exact(eng, mode):
    """Skipped intervals, rows i >= count and count = 0: exactly the previous row (row 0: exactly the zero state)."""
    model, avg = mode
    N = 20
    kn, lin, q, skipped = _skipping_windows(N, 14)
    W = kn.shape[0]
    ref = trace_rows(model, avg, kn, lin, q)
    count = (np.arange(W) * 7 % (N + 1)).astype(np.int32)
    count[:3] = [0, N, 1]
    ref_c = trace_rows(model, avg, kn, lin, q, count)
    want = _wants(model)[-1]
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        got = _host(eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=want))
        _check_rows(got, ref, want, "skips m%d avg%d L%d" % (model, avg, L))
        got_c = _host(eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=want, count=_dev(count, eng)))
        _check_rows(got_c, ref_c, want, "counts m%d avg%d L%d" % (model, avg, L))
        for k in _keys(want) + ("P_sym",):
            zero = np.zeros(got[k].shape[2:])
            if k == "q":
                zero = ZERO_Q
            for w in range(W):
                for i in skipped[w]:
                    assert np.array_equal(got[k][w, i], got[k][w, i - 1] if i > 0 else zero), (k, L, w, i)
                n = int(count[w])
                rep = {i for i in skipped[w] if i < n} | set(range(n, N))
                for i in sorted(rep):
                    assert np.array_equal(got_c[k][w, i], got_c[k][w, i - 1] if i > 0 else zero), (k, L, w, i, n)


@pytest.mark.parametrize("mode", MODES)
def test_running_writes_nothing_outside_its_rows(eng, mode):
    """Guard bands before and after every array: W not a multiple of the windows per wavefront, garbage counts, idle lanes."""
    model, avg = mode
    N, G, SENT = 10, 4096, -7.25
    want = _wants(model)[-1]
    for W in (1, 67, 130):
        kn, lin, q, flat, first, count, given = _ragged(W, N, 15 + W, garbage=True)
        ref = trace_rows(model, avg, kn, lin, q, count)
        for L in (0, 1, 3, 5, 6, 12, 64):
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)
            bufs, views = {}, {}
            for k, v in eng.alloc_outputs(W * N, want, model).items():
                n = v[0].numel()
                bufs[k] = torch.full((2 * G + W * N * n,), SENT, dtype=torch.float64, device=eng.device)
                views[k] = bufs[k][G:G + W * N * n].view((W, N) + tuple(v.shape[1:]))
            out = eng.preintegrate_running(_dev(flat, eng), _dev(lin, eng), _dev(q, eng), prm, want=want, first=_dev(first, eng),
                                           count=_dev(given, eng), N=N, out=views)
            got = _host(out)
            _check_rows(got, ref, want, "guards m%d avg%d W%d L%d" % (model, avg, W, L))
            for k, b in bufs.items():
                assert torch.all(b[:G] == SENT) and torch.all(b[-G:] == SENT), (k, W, L)


@pytest.mark.parametrize("model", [1, 2])
def test_running_rows_feed_predict(eng, model):
    """Engine.predict on the reshaped rows (F = W N, idx_i[row] = row // N) = oracle.predict on the trace rows."""
    W, N = 37, 20
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=16))
    ref = trace_rows(model, 0, kn, lin, q)
    dl = _dev(lin, eng)
    rows = eng.preintegrate_running(_dev(kn, eng), dl, _dev(q, eng), eng.make_params(model), want=("mean",))
    meas = {k: v.reshape((W * N,) + tuple(v.shape[2:])) for k, v in rows.items()}
    zeros = torch.zeros((W, 3), dtype=torch.float64, device=eng.device)
    xi, _ = synth.make_states(zeros, zeros, torch.tensor([[0.0, 0, 0, 1]] * W, dtype=torch.float64, device=eng.device), zeros[:, 0], dl,
                              model, device=eng.device)
    idx = (torch.arange(W * N, device=eng.device) // N).to(torch.int32)
    got = eng.predict(model, meas, xi, idx_i=idx)
    torch.cuda.synchronize()
    flat = {k: ref[k].reshape((W * N,) + ref[k].shape[2:]) for k in MEAN}
    for k in JAC + (("O_a", "O_b") if model == 2 else ()):
        flat[k] = np.zeros((W * N, 9))                      # predict reads DT, alpha, beta, q only
    sel = np.repeat(np.arange(W), N)
    rec = op.factor_records(flat, lin[sel], q[sel] if model == 2 else None)
    want = op.oracle().predict(model, rec, xi.cpu().numpy()[sel])
    assert np.abs(got.cpu().numpy() - want).max() <= TOL_FACTOR * max(1.0, np.abs(want).max())


def test_running_graph_capture_and_replay(eng):
    """One call captured on a single stream; a replay with new knots in the same buffers equals an eager call."""
    W, N = 300, 20
    kn, lin, q = synth.make_windows(W, N, seed=17, device=eng.device)
    for model in (1, 2):
        prm = eng.make_params(model)
        want = _wants(model)[-1]
        out = eng.preintegrate_running(kn, lin, q, prm, want=want)

        def call():
            eng.preintegrate_running(kn, lin, q, prm, want=want, out=out)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
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
        kn[:, :, 1:4] *= 1.01                               # new measurements in the same buffers
        g.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        call()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], replayed[k]), k
            assert k == "DT" or not torch.equal(out[k], eager[k]), k    # (the stamps did not change)


@pytest.mark.parametrize("mode", MODES)
def test_running_host_entry(eng, mode):
    """Host pointers: one chunk and several chunks of the pipeline (<= 65 536 rows each), per-window counts; equal to the device
    entry with the lane split pinned, and to the oracle's trace."""
    model, avg = mode
    prm = eng.make_params(model, bool(avg), lanes_per_window=1)
    want = _wants(model)[-1]
    for W, N in ((50, 20), (4500, 30)):
        kn, lin, q = synth.make_windows(W, N, seed=18)
        count = torch.from_numpy((np.arange(W) * 5 % (N + 1)).astype(np.int32))
        for cnt in (None, count):
            got = eng.preintegrate_running_host(kn, lin, q, prm, want=want, count=cnt)
            dev = _host(eng.preintegrate_running(kn.to(eng.device), lin.to(eng.device), q.to(eng.device), prm, want=want,
                                                 count=None if cnt is None else cnt.to(eng.device)))
            for k in dev:
                assert np.array_equal(got[k].numpy(), dev[k]), (k, W, cnt is None)
        if W <= 100:
            ref = trace_rows(model, avg, kn.numpy(), lin.numpy(), q.numpy(), count.numpy())
            _check_rows({k: v.numpy() for k, v in got.items()}, ref, want, "host m%d avg%d" % (model, avg))


def test_running_argument_checks(eng):
    W, N = 8, 5
    kn, lin, q = synth.make_windows(W, N, seed=19, device=eng.device)
    from cpi_amd import CpiError
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_running(kn, lin, q, eng.make_params(3), want=("mean",))
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_running(kn, lin, q, eng.make_params(2), want=("mean", "jac"))
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_running_host(kn.cpu(), lin.cpu(), q.cpu(), eng.make_params(3), want=("mean",))
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_running_host(kn.cpu(), lin.cpu(), q.cpu(), eng.make_params(2), want=("jac",))
    with pytest.raises(CpiError, match="q_k_lin"):
        eng.preintegrate_running(kn, lin, None, eng.make_params(2), want=("mean",))
    with pytest.raises(CpiError, match="lanes_per_window"):
        eng.preintegrate_running(kn, lin, q, eng.make_params(1, lanes_per_window=7), want=("mean",))
    big = torch.zeros((1, 65537, 7), dtype=torch.float64, device=eng.device)
    with pytest.raises(CpiError, match="65535"):
        eng.preintegrate_running(big, lin[:1], q[:1], eng.make_params(1), want=("mean",),
                                 out={"DT": torch.zeros((1, 65536), dtype=torch.float64, device=eng.device)})
    # W == 0 and N == 0 are no-ops; the default want of model 2 asks for no Jacobians
    sent = {"DT": torch.full((4,), 3.0, dtype=torch.float64, device=eng.device)}
    eng.preintegrate_running(kn[:0], lin[:0], q[:0], eng.make_params(1), out=sent)
    eng.preintegrate_running(kn[:, :1].contiguous(), lin, q, eng.make_params(1), out=sent)
    torch.cuda.synchronize()
    assert torch.all(sent["DT"] == 3.0)
    assert sorted(eng.preintegrate_running(kn, lin, q, eng.make_params(2))) == sorted(MEAN + ("P",))
    assert eng.lib.cpi_abi_version() == 3


@pytest.mark.parametrize("model", [1, 2])
def test_running_cpp_facade(eng, model):
    """tests/cpp/test_running.cpp: cpi_host::CpiBatch::running against libcpi_amd.so -- per window one result per fed interval,
    equal to Engine.preintegrate_running on the same ragged batch; the windows' own members after flush() agree with their
    last rows at the gates."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    W, N = 9, 12
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=20, edge_cases=False))
    count = np.array([12, 1, 5, 12, 7, 3, 12, 2, 9], dtype=np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_running")
        subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_running.cpp"), "-o", exe,
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
            lines = p.stdout.splitlines()
            sizes = [int(ln.split()[1]) for ln in lines if ln.startswith("ROWS")]
            assert sizes == count.tolist()
            nrow = int(count.sum())
            body = [ln for ln in lines if not ln.startswith(("ROWS", "FINAL"))]
            assert len(body) == nrow + W
            vals = np.array([[float(x) for x in ln.split()] for ln in body])
            rows, final = vals[:nrow], vals[nrow:]
            want = ("mean", "jac", "cov") if model == 1 else ("mean", "cov")
            out = _host(eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), eng.make_params(model, bool(avg)),
                                                 want=want, count=_dev(count, eng)))
            cols = [out["DT"][..., None], out["alpha"], out["beta"], out["q"]] + ([out[k] for k in JAC] if model == 1 else []) + [out["P"]]
            full = np.concatenate(cols, axis=2)
            expect = np.concatenate([full[w, :count[w]] for w in range(W)], axis=0)
            assert rows.shape == expect.shape and np.array_equal(rows, expect), (model, avg)
            last = np.stack([full[w, count[w] - 1] for w in range(W)])
            nm = 11 + (45 if model == 1 else 0)
            assert np.abs(final[:, :11] - last[:, :11]).max() <= 1e-9
            if model == 1:
                assert np.abs(final[:, 11:nm] - last[:, 11:nm]).max() <= 1e-8
            check_pre({"P": final[:, nm:]}, {"P": last[:, nm:]}, what=("cov",), label="facade final vs last row")
