"""GPU: many IMU streams (runs) in one call (cpi_preintegrate_streams, Engine.preintegrate_streams, the _host entry and
cpi_host::ImuStreamSet).  Window u of run r must be, bit for bit, window u - update_offsets[r] of the single-stream entry on
run r alone (same N, same lane split), and the whole call must equal cpi_preintegrate_batch on the windows the host assembler
cuts out of every run -- every run starting its clock at 0, as the reference's Monte-Carlo datasets do."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import stream as st
from oracle import oracle_py as op
from tests.tol import check_pre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "imu_gazebo200_excerpt.dat")
WANTS = [("mean",), ("mean", "jac"), ("mean", "jac", "cov"), ("cov",), ("cov_sym",)]


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _lin_q(U, seed):
    rng = np.random.default_rng(seed)
    lin = np.concatenate([0.01 * rng.standard_normal((U, 3)), 0.05 * rng.standard_normal((U, 3))], axis=1)
    q = rng.standard_normal((U, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1
    return lin, q


def _synth_runs(spec, seed=0):
    """spec: (windows, samples per window, phase) per run -> [(stream [K,7], update_times [U])], each run re-based to t = 0."""
    from cpi_amd import synth
    runs = []
    for r, (W, n, phase) in enumerate(spec):
        s, u, _, _ = synth.make_stream(W, n, seed=seed + 17 * r, phase=phase)
        s, u = s.numpy().copy(), u.numpy().copy()
        t0 = s[0, 0]
        s[:, 0] -= t0
        u -= t0
        runs.append((s, u))
    return runs


def _pack(runs):
    stream = np.concatenate([s for s, _ in runs]).reshape(-1, 7)
    ut = np.concatenate([u for _, u in runs])
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in runs])]).astype(np.int64)
    uo = np.concatenate([[0], np.cumsum([len(u) for _, u in runs])]).astype(np.int64)
    return stream, so, ut, uo


def _ragged(runs):
    """Every run's windows by the host assembler (cpi_amd/stream.py), concatenated: (knots, first, count).  A run without
    readings gets windows of 0 intervals on knot 0 (the batch entry's zero-length window)."""
    ks, fs, cs, base = [], [], [], 0
    for s, u in runs:
        if len(s) == 0:
            fs.append(np.zeros(len(u), np.int64)); cs.append(np.zeros(len(u), np.int32))
            continue
        k, f, c = st.assemble_windows(s, u) if len(u) else (np.zeros((0, 7)), np.zeros(0, np.int64), np.zeros(0, np.int32))
        ks.append(k); fs.append(f + base); cs.append(c)
        base += len(k)
    return np.concatenate(ks), np.concatenate(fs), np.concatenate(cs)


def _T(a, eng):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _out_keys(out):
    return [k for k in out if not k.startswith("_")]


@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("avg", [0, 1])
def test_gpu_streams_bitwise_equal_the_ragged_batch(eng, model, avg):
    """One multi-run call == cpi_preintegrate_batch on the concatenated host-assembled windows (same W, same N: same lane
    split), for every output set, bit for bit.  Mean-only requests take the fused route (CUT = 3), the others the cut kernel."""
    runs = _synth_runs([(40, 20, 0.37), (7, 20, 0.0), (65, 10, 0.8), (1, 20, 0.5), (30, 13, 0.25)], seed=model * 10 + avg)
    # ragged update grids: one run jittered, one with an update before its first reading and one past its last
    s, u = runs[2]
    u = np.sort(u + np.random.default_rng(3).uniform(-0.02, 0.02, len(u)))
    runs[2] = (s, u)
    s, u = runs[4]
    runs[4] = (s, np.sort(np.concatenate([u, [-0.5, s[-1, 0] + 0.3]])))
    stream, so, ut, uo = _pack(runs)
    knots, first, count = _ragged(runs)
    U, N = len(ut), int(count.max())
    lin, q = _lin_q(U, 7)
    dk, dso, du, duo, dl, dq = (_T(a, eng) for a in (stream, so, ut, uo, lin, q))
    ck, cf, cc = _T(knots, eng), _T(first, eng), _T(count, eng)
    prm = eng.make_params(model, bool(avg))
    for want in WANTS:
        out, cnt = eng.preintegrate_streams(dk, dso, du, duo, dl, dq, prm, want=want, N=N, return_counts=True)
        ref = eng.preintegrate(ck, dl, dq, prm, want=want, first=cf, count=cc, N=N)
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), count), want
        for k in _out_keys(ref):
            assert torch.equal(out[k], ref[k]), (model, avg, want, k)


@pytest.mark.parametrize("model", [1, 2])
def test_gpu_streams_equal_per_run_stream_calls(eng, model):
    """Pinned lanes: every run's windows equal a cpi_preintegrate_stream call on that run alone, bit for bit (counts too).
    Automatic lanes: the split depends on the number of windows, so the runs agree at the tolerance gates."""
    runs = _synth_runs([(30, 20, 0.37), (12, 20, 0.0), (50, 10, 0.6), (3, 25, 0.9)], seed=40 + model)
    stream, so, ut, uo = _pack(runs)
    U = len(ut)
    lin, q = _lin_q(U, 11)
    N = eng.streams_bound(_T(stream, eng), so, _T(ut, eng), uo)
    dk, dso, du, duo, dl, dq = (_T(a, eng) for a in (stream, so, ut, uo, lin, q))
    for lanes in (1, 2, 3, 8, 16, 0):
        prm = eng.make_params(model, lanes_per_window=lanes)
        for want in (("mean",), ("mean", "jac", "cov")):
            out, cnt = eng.preintegrate_streams(dk, dso, du, duo, dl, dq, prm, want=want, N=N, return_counts=True)
            for r, (s, u) in enumerate(runs):
                a, b = uo[r], uo[r + 1]
                one, c1 = eng.preintegrate_stream(_T(s, eng), _T(u, eng), dl[a:b].contiguous(), dq[a:b].contiguous(), prm, want=want,
                                                  N=N, return_counts=True)
                torch.cuda.synchronize()
                assert torch.equal(cnt[a:b], c1), (lanes, r)
                for k in _out_keys(one):
                    if lanes:
                        assert torch.equal(out[k][a:b], one[k]), (lanes, want, r, k)
                check_pre({k: out[k][a:b].cpu().numpy() for k in _out_keys(one)}, {k: v.cpu().numpy() for k, v in one.items()},
                          what=tuple(w for w in want), v2=(model == 2), label="run %d L%d" % (r, lanes))


@pytest.mark.parametrize("model", [1, 2])
def test_gpu_streams_one_run_is_the_single_stream_entry(eng, model):
    """R = 1 with the same arguments is cpi_preintegrate_stream bit for bit -- automatic lanes included, and at a size where the
    mean-only request takes the three-knot kernel (model 1, >= 100 000 windows)."""
    from cpi_amd import synth
    for W, n, phase in ((300, 20, 0.37), (2000, 10, 0.0), (120_000 if model == 1 else 5000, 20, 0.45)):
        s, u, lin, q = synth.make_stream(W, n, seed=W + model, device=eng.device, phase=phase)
        prm = eng.make_params(model)
        for want in (("mean",), ("mean", "jac", "cov")) if W < 100_000 else (("mean",),):
            a, ca = eng.preintegrate_streams(s, [0, s.shape[0]], u, [0, W], lin, q, prm, want=want, N=n + 1, return_counts=True)
            b, cb = eng.preintegrate_stream(s, u, lin, q, prm, want=want, N=n + 1, return_counts=True)
            torch.cuda.synchronize()
            assert torch.equal(ca, cb), W
            for k in _out_keys(b):
                assert torch.equal(a[k], b[k]), (W, want, k)


def _edge_runs():
    rng = np.random.default_rng(9)
    runs = []
    s = _synth_runs([(20, 10, 0.4)], seed=3)[0][0]

    def run(K, ut):
        return (s[:K].copy(), np.asarray(ut, dtype=np.float64))
    t = s[:, 0]
    runs.append(run(0, [0.01, 0.02, 0.02]))                                    # no readings
    runs.append(run(1, [-0.1, 0.0, 0.003, 0.5]))                               # one reading
    runs.append(run(2, [t[0] - 0.1, t[1], t[1] + 0.001, t[1] + 0.001]))          # two, repeated update
    runs.append(run(3, [t[1] + 0.002, t[2] + 0.4]))                            # three, past the end
    runs.append(run(120, []))                                                   # no update times
    g = s[:150].copy()
    g[70:, 0] += 0.25                                                           # a gap
    runs.append((g, np.sort(np.concatenate([[-0.2, -0.1], rng.uniform(0, g[-1, 0] + 0.1, 15), [g[-1, 0] + 1.0]]))))
    runs.append(run(4, [t[3]]))
    runs.append(run(60, np.sort(rng.uniform(t[0], t[59], 6))))
    return runs


@pytest.mark.parametrize("model", [1, 2, 3])
def test_gpu_streams_edge_runs(eng, model):
    """Runs of 0, 1, 2 and 3 readings, a run without update times, update times before a run's first reading and after its
    last, repeated update times, gaps; and a window bound N too small: the true counts are reported and every window is
    truncated exactly as the single-stream entry truncates it."""
    runs = _edge_runs()
    stream, so, ut, uo = _pack(runs)
    U = len(ut)
    lin, q = _lin_q(U, 13)
    dk, dso, du, duo, dl, dq = (_T(a, eng) for a in (stream, so, ut, uo, lin, q))
    Nx = eng.streams_bound(dk, dso, du, duo)
    for N in (Nx, 3):
        for lanes in (1, 3):
            prm = eng.make_params(model, lanes_per_window=lanes)
            for want in (("mean",), ("mean", "jac", "cov")):
                out, cnt = eng.preintegrate_streams(dk, dso, du, duo, dl, dq, prm, want=want, N=N, return_counts=True,
                                                    check_counts=(N == Nx))
                torch.cuda.synchronize()
                for r, (s, u) in enumerate(runs):
                    a, b = uo[r], uo[r + 1]
                    if a == b:
                        continue
                    if len(s) == 0:
                        # no readings: zero-length windows, the batch entry's identity / zero state
                        zero = eng.preintegrate(dk, dl[a:b].contiguous(), dq[a:b].contiguous(), prm, want=want,
                                                first=torch.zeros(b - a, dtype=torch.int64, device=eng.device),
                                                count=torch.zeros(b - a, dtype=torch.int32, device=eng.device), N=N)
                        torch.cuda.synchronize()
                        assert int(cnt[a:b].abs().sum()) == 0
                        for k in _out_keys(zero):
                            assert torch.equal(out[k][a:b], zero[k]), (r, k)
                        continue
                    one, c1 = eng.preintegrate_stream(_T(s, eng), _T(u, eng), dl[a:b].contiguous(), dq[a:b].contiguous(), prm,
                                                      want=want, N=N, return_counts=True, check_counts=False)
                    torch.cuda.synchronize()
                    assert torch.equal(cnt[a:b], c1), (N, r, cnt[a:b], c1)
                    for k in _out_keys(one):
                        if model == 3 and k in ("P", "P_sym"):
                            continue      # the Forster covariance of a window depends on its wavefront's neighbours to rounding
                        assert torch.equal(out[k][a:b], one[k]), (N, lanes, want, r, k)
                    if model == 3 and "cov" in want:
                        check_pre({k: out[k][a:b].cpu().numpy() for k in _out_keys(one)}, {k: v.cpu().numpy() for k, v in one.items()},
                                  what=want, label="Forster run %d" % r)
                if N < Nx:
                    assert int(cnt.max()) > N
                    with pytest.raises(ValueError):
                        eng.preintegrate_streams(dk, dso, du, duo, dl, dq, prm, want=want, N=N)


@pytest.mark.parametrize("mode", [(1, 0, 1), (2, 1, 1)])
def test_gpu_streams_golden_excerpt_split_into_runs(eng, mode):
    """The reference's IMU excerpt cut into four runs, each re-based to t = 0 (the stamps go backwards at every boundary): the
    multi-run call against the oracle's restatement of the deque loop on each run, and against per-run stream calls bitwise."""
    kn = st.parse_imu_text(open(DATA).read())
    cuts = [0, 97, 230, 231 + 60, len(kn)]
    runs = []
    for r in range(4):
        s = kn[cuts[r]:cuts[r + 1]].copy()
        s[:, 0] -= s[0, 0]
        ut = 0.0237 + 0.1 * np.arange(int(s[-1, 0] / 0.1) + 1)
        runs.append((s, ut))
    stream, so, ut, uo = _pack(runs)
    U = len(ut)
    lin, q = _lin_q(U, 21)
    dk, dso, du, duo, dl, dq = (_T(a, eng) for a in (stream, so, ut, uo, lin, q))
    prm = eng.make_params(mode[0], bool(mode[1]), bool(mode[2]), lanes_per_window=2)
    out = eng.preintegrate_streams(dk, dso, du, duo, dl, dq, prm)
    torch.cuda.synchronize()
    for r, (s, u) in enumerate(runs):
        a, b = uo[r], uo[r + 1]
        ref = op.oracle().stream(op.make_params(*mode), s, u, lin[a:b], q[a:b])
        check_pre({k: out[k][a:b].cpu().numpy() for k in _out_keys(out)}, ref, v2=(mode[0] == 2), label="golden run %d" % r)
        one = eng.preintegrate_stream(_T(s, eng), _T(u, eng), dl[a:b].contiguous(), dq[a:b].contiguous(), prm,
                                      N=eng.streams_bound(dk, dso, du, duo))
        torch.cuda.synchronize()
        for k in _out_keys(one):
            assert torch.equal(out[k][a:b], one[k]), (r, k)


@pytest.mark.parametrize("want", [("mean",), ("mean", "jac", "cov")])
def test_gpu_streams_graph_capture(eng, want):
    """The device entry with an integer N and check_counts=False is free of host synchronisations: it captures into a graph,
    and a replay reproduces the eager outputs."""
    runs = _synth_runs([(30, 20, 0.37), (9, 20, 0.0), (45, 10, 0.6)], seed=77)
    stream, so, ut, uo = _pack(runs)
    U = len(ut)
    lin, q = _lin_q(U, 5)
    dk, dso, du, duo, dl, dq = (_T(a, eng) for a in (stream, so, ut, uo, lin, q))
    N = eng.streams_bound(dk, dso, du, duo)
    prm = eng.make_params(1)
    out = eng.alloc_outputs(U, want, 1)
    ws = eng.streams_workspace(len(runs), U)

    def call():
        eng.preintegrate_streams(dk, dso, du, duo, dl, dq, prm, want=want, N=N, out=out, check_counts=False, workspace=ws)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()
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


@pytest.mark.parametrize("model", [1, 2])
def test_gpu_streams_host_entry(eng, model):
    """cpi_preintegrate_streams_host on pageable and on pinned inputs equals the device entry; invalid offsets return
    CPI_ERR_INVALID before anything is enqueued (the caller's outputs and counts stay untouched)."""
    from cpi_amd import _lib
    runs = _edge_runs()[:4] + _synth_runs([(20, 20, 0.3), (11, 10, 0.0)], seed=90)
    stream, so, ut, uo = _pack(runs)
    U = len(ut)
    lin, q = _lin_q(U, 17)
    N = eng.streams_bound(torch.from_numpy(stream), so, torch.from_numpy(ut), uo)
    prm = eng.make_params(model)
    dev, dc = eng.preintegrate_streams(*(_T(a, eng) for a in (stream, so, ut, uo, lin, q)), prm, N=N, return_counts=True)
    torch.cuda.synchronize()
    H = lambda a, pin: (torch.from_numpy(np.ascontiguousarray(a)).pin_memory() if pin else torch.from_numpy(np.ascontiguousarray(a)))
    for pinned in (False, True):
        host, hc = eng.preintegrate_streams_host(H(stream, pinned), so, H(ut, pinned), uo, H(lin, pinned), H(q, pinned), prm, N=N,
                                                 pinned=pinned, return_counts=True)
        assert torch.equal(hc, dc.cpu())
        for k in _out_keys(dev):
            assert torch.equal(host[k], dev[k].cpu()), (pinned, k)
    # invalid offsets: not starting at 0, decreasing, not ending at K / U
    lib = eng.lib
    R, K = len(runs), len(stream)
    ts, tu, tl, tq = (H(a, False) for a in (stream, ut, lin, q))
    out = {k: torch.full(v.shape, -7.0, dtype=torch.float64) for k, v in dev.items()}
    o = eng._outputs_struct(out)
    cnt = torch.full((U,), -7, dtype=torch.int32)
    P = lambda t: C.c_void_p(t.data_ptr())
    bad = []
    for which in (0, 1):
        for kind in ("start", "decrease", "end"):
            s2, u2 = so.copy(), uo.copy()
            x = s2 if which == 0 else u2
            if kind == "start":
                x[0] = 1
            elif kind == "decrease":
                x[2], x[3] = x[3], x[2] - 1
            else:
                x[-1] -= 1
            bad.append((s2, u2))
    for s2, u2 in bad:
        rc = lib.cpi_preintegrate_streams_host(eng.ctx, C.byref(prm), R, K, P(ts), P(torch.from_numpy(s2)), U, P(tu),
                                               P(torch.from_numpy(u2)), N, P(tl), P(tq), C.byref(o), P(cnt))
        assert rc == _lib.CPI_ERR_INVALID, (s2, u2)
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in out.values()) and bool((cnt == -7).all())


def test_gpu_streams_device_entry_refuses_invalid_calls_before_enqueueing_anything(eng):
    """NULL offsets, no run, no reading, a bad model or N: CPI_ERR_INVALID and the workspace untouched."""
    from cpi_amd import _lib
    runs = _synth_runs([(10, 10, 0.3), (5, 10, 0.0)], seed=4)
    stream, so, ut, uo = _pack(runs)
    U, K, R = len(ut), len(stream), len(runs)
    lin, q = _lin_q(U, 2)
    dk, dso, du, duo, dl, dq = (_T(a, eng) for a in (stream, so, ut, uo, lin, q))
    out = eng.alloc_outputs(U, ("mean", "jac", "cov"), 2)
    o = eng._outputs_struct(out)
    ws = eng.streams_workspace(R, U)
    ws.fill_(-7.0)
    torch.cuda.synchronize()
    good = eng.make_params(2)
    bad_model = eng.make_params(2); bad_model.model = 9
    P = lambda t: C.c_void_p(t.data_ptr())
    calls = [
        (C.byref(good), R, K, None, P(duo), 11, P(dq)),             # stream_offsets NULL
        (C.byref(good), R, K, P(dso), None, 11, P(dq)),             # update_offsets NULL
        (C.byref(good), 0, K, P(dso), P(duo), 11, P(dq)),           # U windows, no run
        (C.byref(good), R, 0, P(dso), P(duo), 11, P(dq)),           # no reading
        (C.byref(good), R, K, P(dso), P(duo), 11, None),            # model 2 without q_k_lin
        (C.byref(bad_model), R, K, P(dso), P(duo), 11, P(dq)),      # unknown model
        (C.byref(good), R, K, P(dso), P(duo), 70000, P(dq)),        # N > 65535
    ]
    for prm, r, k, s_off, u_off, N, qq in calls:
        rc = eng.lib.cpi_preintegrate_streams(eng.ctx, prm, r, k, P(dk), s_off, U, P(du), u_off, N, P(dl), qq, P(ws), C.byref(o))
        assert rc == _lib.CPI_ERR_INVALID, (r, k, N)
    torch.cuda.synchronize()
    assert bool((ws == -7.0).all()), "an invalid call wrote the workspace"
    assert eng.lib.cpi_preintegrate_streams(eng.ctx, C.byref(good), R, K, P(dk), P(dso), 0, P(du), P(duo), 11, P(dl), P(dq), P(ws),
                                            C.byref(o)) == 0   # U == 0: a no-op


def test_gpu_streams_wrong_device_offsets_are_clamped(eng):
    """Offsets the device entry cannot validate (past K / U, decreasing, negative) give wrong windows, never an out-of-bounds
    read.  The stream and the update times are views into larger buffers with a sentinel row / stamp on either side; the call
    runs twice with different sentinels (+1e300, then -1e300), and a read of any of them would change an output or a count."""
    runs = _synth_runs([(10, 10, 0.3), (5, 10, 0.0), (8, 10, 0.5)], seed=8)
    stream, so, ut, uo = _pack(runs)
    U, K = len(ut), len(stream)
    lin, q = _lin_q(U, 3)
    dl = _T(lin, eng)
    sbuf = torch.zeros((K + 2, 7), dtype=torch.float64, device=eng.device)
    ubuf = torch.zeros((U + 2,), dtype=torch.float64, device=eng.device)
    sbuf[1:K + 1] = _T(stream, eng)
    ubuf[1:U + 1] = _T(ut, eng)
    dk, du = sbuf[1:K + 1], ubuf[1:U + 1]
    assert dk.is_contiguous() and du.is_contiguous()
    bits = lambda t: t.contiguous().view(torch.int64)
    cases = (([0, K + 500, 3, K + 9], uo), (so, [0, -4, U + 100, U]), ([-9, 5, 2, 1 << 40], [1 << 40, 2, 1, -3]),
             (so, [-1, 5, 9, U]), ([0, K], [-1, U]), ([-5, K + 3], [-7, U + 2]))
    for s2, u2 in cases:
        for lanes in (0, 1, 3):
            for want in (("mean",), ("mean", "jac", "cov")):
                got = []
                for sentinel in (1e300, -1e300):
                    sbuf[0] = sentinel; sbuf[K + 1] = sentinel
                    ubuf[0] = sentinel; ubuf[U + 1] = sentinel
                    out, cnt = eng.preintegrate_streams(dk, np.asarray(s2, np.int64), du, np.asarray(u2, np.int64), dl, None,
                                                        eng.make_params(1, lanes_per_window=lanes), want=want, N=12,
                                                        return_counts=True, check_counts=False)
                    torch.cuda.synchronize()
                    got.append((out, cnt.clone()))
                (o1, c1), (o2, c2) = got
                assert torch.equal(c1, c2), (s2, u2, lanes, want)
                c = c1.cpu().numpy()
                assert c.min() >= 0 and c.max() <= K, (s2, u2)
                for k in _out_keys(o1):
                    assert torch.equal(bits(o1[k]), bits(o2[k])), (s2, u2, lanes, want, k)


@pytest.mark.parametrize("avg", [0, 1])
def test_gpu_streams_three_knot_kernel_across_run_boundaries(eng, avg):
    """Mean-only, one lane per window, >= 100 000 windows: the three-knot (BIG) instantiation of CUT = 3, with wavefronts that
    straddle run boundaries (per-lane run lookup under the wavefront's staging base), a jittered run (per-element path) and a
    run on the IMU grid (no tail).  Bit for bit against per-run cpi_preintegrate_stream calls (30 000 windows each: the
    two-knot kernel)."""
    from cpi_amd import synth
    spec = ((30001, 20, 0.37), (29950, 20, 0.0), (30010, 20, 0.6), (30039, 20, 0.45))
    runs = []
    for r, (W, n, phase) in enumerate(spec):
        s, u, _, _ = synth.make_stream(W, n, seed=500 + r, device=eng.device, phase=phase)
        s = s.clone(); u = u.clone()
        t0 = s[0, 0].item()
        s[:, 0] -= t0
        u -= t0
        if r == 2:
            g = torch.Generator(device=eng.device); g.manual_seed(3)
            u = torch.sort(u + 0.02 * (torch.rand(u.shape, generator=g, dtype=torch.float64, device=eng.device) - 0.5)).values
        runs.append((s.contiguous(), u.contiguous()))
    U = sum(u.shape[0] for _, u in runs)
    assert U >= 100_000
    lin, _ = _lin_q(U, 19)
    dl = _T(lin, eng)
    prm = eng.make_params(1, bool(avg), lanes_per_window=1)
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in runs])])
    uo = np.concatenate([[0], np.cumsum([u.shape[0] for _, u in runs])])
    N = eng.streams_bound(torch.cat([s for s, _ in runs]), so, torch.cat([u for _, u in runs]), uo)
    assert N >= 16    # the three-knot kernel's minimum window length
    out, cnt = eng.preintegrate_streams([s for s, _ in runs], None, [u for _, u in runs], None, dl, None, prm, want=("mean",), N=N,
                                        return_counts=True)
    for r, (s, u) in enumerate(runs):
        a, b = int(uo[r]), int(uo[r + 1])
        one, c1 = eng.preintegrate_stream(s, u, dl[a:b].contiguous(), None, prm, want=("mean",), N=N, return_counts=True)
        torch.cuda.synchronize()
        assert torch.equal(cnt[a:b], c1), r
        for k in _out_keys(one):
            assert torch.equal(out[k][a:b], one[k]), (r, k)


def test_gpu_streams_cpp_facade(eng):
    """tests/cpp/test_streams.cpp: cpi_host::ImuStreamSet against libcpi_amd.so -- one call for all runs, results per run per
    update time -- must print exactly what the Python entry computes."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    runs = _edge_runs()[:5] + _synth_runs([(12, 20, 0.4), (6, 10, 0.0)], seed=31)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_streams")
        subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_streams.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        stream, so, ut, uo = _pack(runs)
        U = len(ut)
        lin, q = _lin_q(U, 23)
        with open(os.path.join(tmp, "runs.txt"), "w") as f:
            f.write("%d\n" % len(runs))
            for r, (s, u) in enumerate(runs):
                f.write("%d %d\n" % (len(s), len(u)))
                for row in s:
                    f.write(" ".join("%.17g" % v for v in row) + "\n")
                for j in range(len(u)):
                    w = uo[r] + j
                    f.write(" ".join("%.17g" % v for v in [u[j], *lin[w], *q[w]]) + "\n")
        for model in (1, 2):
            N = eng.streams_bound(torch.from_numpy(stream), so, torch.from_numpy(ut), uo)
            p = subprocess.run([exe, os.path.join(tmp, "runs.txt"), str(model), str(N)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            lines = p.stdout.splitlines()
            got = np.array([[float(x) for x in ln.split()] for ln in lines if not ln.startswith("COUNT")])
            counts = [int(x) for ln in lines if ln.startswith("COUNT") for x in ln.split()[1:]]
            prm = eng.make_params(model, lanes_per_window=1)
            out, cnt = eng.preintegrate_streams(*(_T(a, eng) for a in (stream, so, ut, uo, lin, q)), prm, N=N, return_counts=True)
            torch.cuda.synchronize()
            assert counts == cnt.cpu().tolist()
            cols = [out["DT"][:, None], out["alpha"], out["beta"], out["q"], out["J_q"], out["J_a"], out["J_b"], out["H_a"], out["H_b"]]
            if model == 2:
                cols += [out["O_a"], out["O_b"]]
            want = torch.cat(cols + [out["P"]], dim=1).cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), model
