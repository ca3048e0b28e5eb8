"""GPU: the mean kernels (cpi_mean_kernel, cpi_mean_carry_kernel, cpi_mean_runs_kernel, cpi_mean_tiled_kernel) under large
rotations, through every entry that launches them: Engine.preintegrate (dense and ragged, every lanes_per_window),
preintegrate_resume, preintegrate_stream / preintegrate_streams (the wavefront-cut routes CUT = 2 and 3 and the workspace route
CUT = 1, with the held tail knot), preintegrate_tiled (split across wavefronts) and the three-knot BIG instantiation.  The inputs
are those of tests/mean_cases.py (|w| dt up to ~1.2 rad per interval: every wavefront mixes lanes on the short polynomial of
sincos_fast, on the long one and on the Cody-Waite reduction -- the wave-uniform ballot, which no host emulation covers --, the
composition tree joins segment rotations past 90 degrees, and the final rotations reach every branch of rot_2_quat);
tests/test_mean_cases_cpu.py keeps them honest.

Reference: the oracle (oracle_py.oracle().run) on the same window, cut at its count; every window of every case, none left out.
One gate per field and per kind of comparison (tests/mean_cases.py: GATE = 100 x the floor measured on an MI355X, never looser
than TOL_MEAN / TOL_JAC / TOL_COV).  Every output array is filled with NaN before each call and lies between guard bands; each
test prints its table (pytest -s; profiles/mean_edges.md).  Exact equality is asserted only where the header, DESIGN.md or an
existing test promises it; what turned out equal without a promise is printed, not asserted."""
import numpy as np
import pytest
import torch

from cpi_amd.engine import pack_sym
from tests import mean_cases as mc
from tests import running_cases as rc
from tests.mean_cases import GATE, JAC5, JAC7, MEAN, MEAN_LANES, MODES
from tests.test_gpu_running import _dev, _ragged_layout
from tests.test_gpu_stream_running import _bits_equal, _Guarded, _twice
from tests.tol import FieldTable

pytestmark = pytest.mark.gpu
REQUESTS = (("mean",), ("mean", "jac"), ("mean", "jac", "cov", "cov_sym"))     # means only, means + Jacobians, everything
RESUME_LANES = (0, 1, 3, 8, 64)
STREAM_LANES = (0, 1, 2, 5, 8, 16, 32, 64)   # 32 and 64: two windows / one window per wavefront, segments of unequal length
TILE_SPLITS = (0, 1, 2, 4, 5, 8)             # wavefronts per tile; model 2: 5 and 8 take more than 64 KB of dynamic LDS
G, SENT = 1024, -7.25                        # doubles of guard band on either side of every output array, and what they hold


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _fields(model, want):
    """The fields of a request that are compared here (model 2's Jacobians have their gates in tests/test_gpu_stj_edges.py)."""
    return MEAN + (JAC5 if model == 1 and "jac" in want else ()) + (("P",) if "cov" in want else ())


def _keys(model, want):
    return set(MEAN + ((JAC5 if model == 1 else JAC7) if "jac" in want else ()) + (("P",) if "cov" in want else ())
               + (("P_sym",) if "cov_sym" in want else ()))


class _Out:
    """Output arrays for W windows, NaN-filled, each inside its own buffer with G sentinel doubles on either side."""

    def __init__(self, eng, W, want, model):
        self.bufs, self.views = {}, {}
        for k, v in eng.alloc_outputs(W, tuple(want), model).items():
            self.bufs[k] = torch.full((2 * G + v.numel(),), SENT, dtype=torch.float64, device=eng.device)
            self.views[k] = self.bufs[k][G:G + v.numel()].view(v.shape)
            self.views[k].fill_(float("nan"))

    def host(self, label):
        torch.cuda.synchronize()
        for k, b in self.bufs.items():
            assert torch.all(b[:G] == SENT) and torch.all(b[-G:] == SENT), (label, k, "written outside the output array")
        return {k: v.cpu().numpy() for k, v in self.views.items()}


def _add(t, got, ref, fields, label):
    """The fields of this request into the table (the others stand in as the reference itself: error 0)."""
    assert all(k in got for k in fields), (label, sorted(got))
    t.add({k: got[k] if k in fields else ref[k] for k in t.fields}, ref, label)


def _same(a, b, label, keys=None):
    for k in (keys or a):
        assert _bits_equal(a[k], b[k]), (label, k)


def _differ(a, b, label, keys=None):
    """The fields in which two results do not agree bit for bit, as (label, field): collected, and asserted empty once the table
    is printed and checked, so that a wrong number shows its size against the oracle as well."""
    return [(label, k) for k in (keys or a) if not _bits_equal(np.asarray(a[k]), np.asarray(b[k]))]


def _cpu(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _p_sym(got, label):
    if "P_sym" in got:      # P_sym: bit for bit the upper triangle of P
        assert np.array_equal(pack_sym(torch.from_numpy(got["P"].reshape(-1, 225))).numpy(), got["P_sym"].reshape(-1, 120)), label + " P_sym"


# ------------------------------------------------------------------------------------------------ a. the batch entry
@pytest.mark.parametrize("N", mc.MEAN_EDGE_N)
@pytest.mark.parametrize("mode", MODES)
def test_batch_entry_dense_and_ragged(eng, mode, N):
    """Engine.preintegrate on the 32 tumbling windows of N intervals, dense and as the ragged layout with garbage counts (0, N, 1,
    N - 1, counts outside [0, N], NaN in every knot no window owns): the three requests at lanes_per_window 0 and every L of
    kMeanLanes.  Model 2 honours L for the mean-only request only: its other requests give the same bits at every L.  A NULL
    carry_in reproduces the batch call bit for bit (tests/test_gpu_resume.py)."""
    model, avg = mode
    kn, lin, q = mc.mean_edge_windows(N)
    W = kn.shape[0]
    flat, first, count, given = _ragged_layout(kn, mc.MEAN_LAYOUT_SEED, garbage=True)
    dl, dq = _dev(lin, eng), _dev(q, eng)
    layouts = [("dense", dict(knots=_dev(kn, eng)), None),
               ("ragged", dict(knots=_dev(flat, eng), first=_dev(first, eng), count=_dev(given, eng), N=N), count)]
    seen = []
    for name, args, cnt in layouts:
        ref = mc.oracle_windows(model, avg, kn, lin, q, cnt, key=(name, N))
        t = FieldTable(_fields(model, REQUESTS[-1]))
        one = FieldTable(t.fields)        # one lane per window on its own: no composition tree
        at_L = {}
        for want in REQUESTS:
            base = None
            for L in [0] + MEAN_LANES:
                label = "%s N%d m%d avg%d L%d %s" % (name, N, model, avg, L, "+".join(want))
                prm = eng.make_params(model, bool(avg), lanes_per_window=L)
                o = _Out(eng, W, want, model)
                eng.preintegrate(lin=dl, q_k_lin=dq, params=prm, want=want, out=o.views, **args)
                got = o.host(label)
                assert set(got) == _keys(model, want), label
                for tab in ((t, one) if L == 1 else (t,)):
                    _add(tab, got, ref, _fields(model, want), label)
                _p_sym(got, label)
                at_L[(want, L)] = got
                if model == 2 and want != ("mean",):
                    base = base or got
                    _same(got, base, label + ": model 2 honours lanes_per_window for the mean-only request only")
                if L in (0, 3, 16):
                    r = _Out(eng, W, want, model)
                    eng.preintegrate_resume(lin=dl, q_k_lin=dq, params=prm, want=want, out=r.views, **args)
                    _same(r.host(label + " resume"), got, label + ": a NULL carry_in is the batch call")
        # observed, not promised: the means of the mean-only request beside those of means + Jacobians at the same L
        seen.append("%s: %s" % (name, ", ".join("L%d %s" % (L, all(_bits_equal(at_L[(REQUESTS[0], L)][k], at_L[(REQUESTS[1], L)][k]) for k in MEAN))
                                                  for L in (1, 2, 8, 16, 64))))
        one.report("[batch] Engine.preintegrate, mean_edge_windows(%d) %s, model %d imu_avg %d, L = 1, every request, vs the oracle"
                   % (N, name, model, avg), GATE["batch"])
        t.report("[batch] Engine.preintegrate, mean_edge_windows(%d) %s, model %d imu_avg %d, every L and request, vs the oracle"
                 % (N, name, model, avg), GATE["batch"])
        one.check(GATE["batch"], "batch entry %s N%d, one lane per window" % (name, N))
        t.check(GATE["batch"], "batch entry %s N%d" % (name, N))
    print("observed: means of the mean-only request bit-equal to those of means + Jacobians -- %s" % "; ".join(seen))


# ------------------------------------------------------------------------------------------------ b. the resume entry
@pytest.mark.parametrize("N", [47, 65])
@pytest.mark.parametrize("mode", MODES)
def test_resume_entry_cut_once(eng, mode, N):
    """Every window cut once, at 1, N // 2 and N - 1 intervals (one segment then has fewer intervals than L): the first call against
    the oracle on the cut window, the second call -- continued from the carry record -- against the oracle on the whole window."""
    model, avg = mode
    kn, lin, q = mc.mean_edge_windows(N)
    W = kn.shape[0]
    dl, dq = _dev(lin, eng), _dev(q, eng)
    whole = mc.oracle_windows(model, avg, kn, lin, q, key=("dense", N))
    t = FieldTable(_fields(model, REQUESTS[1]))
    for cut in (1, N // 2, N - 1):
        head = mc.oracle_windows(model, avg, kn[:, :cut + 1], lin, q, key=("head", N, cut))
        ka, kb = _dev(kn[:, :cut + 1], eng), _dev(kn[:, cut:], eng)
        for want in REQUESTS[:2]:
            for L in RESUME_LANES:
                label = "N%d cut %d m%d avg%d L%d %s" % (N, cut, model, avg, L, "+".join(want))
                prm = eng.make_params(model, bool(avg), lanes_per_window=L)
                a, b = _Out(eng, W, want, model), _Out(eng, W, want, model)
                _, carry = eng.preintegrate_resume(ka, dl, dq, prm, want=want, out=a.views)
                eng.preintegrate_resume(kb, dl, dq, prm, want=want, carry_in=carry, out=b.views)
                _add(t, a.host(label), head, _fields(model, want), label + " first call")
                got = b.host(label)
                assert set(got) == _keys(model, want), label
                _add(t, got, whole, _fields(model, want), label + " second call")
    t.report("[resume] Engine.preintegrate_resume, mean_edge_windows(%d) cut once, model %d imu_avg %d, vs the oracle" % (N, model, avg),
             GATE["resume"])
    t.check(GATE["resume"], "resume entry N%d" % N)


# ------------------------------------------------------------------------------------------------ c. the stream entries
def _pack(runs):
    s = np.concatenate([r[0] for r in runs])
    u = np.concatenate([r[1] for r in runs])
    so = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])]).astype(np.int64)
    uo = np.concatenate([[0], np.cumsum([len(r[1]) for r in runs])]).astype(np.int64)
    return s, so, u, uo, np.concatenate([r[2] for r in runs]), np.concatenate([r[3] for r in runs])


@pytest.mark.parametrize("n,phase", mc.STREAM_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_stream_entries(eng, mode, n, phase):
    """The stream cases (a gyro scale that rises along the stream: tails on the short polynomial in early windows, on the wide path
    in late ones) as one stream and as two runs.  Mean-only requests take the routes on which the wavefront cuts its own windows
    (CUT = 2, CUT = 3), means + Jacobians the workspace route (CUT = 1); everything is asked for once, for P.  Every window against
    the oracle on the host-assembled windows; the stream between two sentinels, both runs agreeing bit for bit; and the promised
    equalities: the stream entries give the bits of the batch call on the host-assembled windows (tests/test_gpu_streams.py:
    same W, same N, same lane split), one run is the single-stream entry, at pinned lanes window u of run r is window
    u - update_offsets[r] of the single-stream call on that run alone (include/cpi_amd.h), and the host forms
    (preintegrate_stream_host, preintegrate_streams_host) give the bits of the device entries (tests/test_stream.py,
    tests/test_gpu_streams.py).  The equalities are collected and asserted after the table is printed and checked."""
    model, avg = mode
    runs = [mc.mean_stream(n, phase, r) for r in (0, 1)]
    t = FieldTable(_fields(model, REQUESTS[-1]))
    unequal = []
    # ---- one stream
    s, u, lin, q = runs[0]
    knots, first, count, dense, N = mc.stream_windows(s, u)
    U = len(u)
    ref = mc.oracle_windows(model, avg, dense, lin, q, count, key=("stream", n, phase, 0))
    g = _Guarded(eng, s, u)
    dl, dq = _dev(lin, eng), _dev(q, eng)
    ck, cf, cc = _dev(knots, eng), _dev(first, eng), _dev(count, eng)
    for want in REQUESTS:
        for L in (STREAM_LANES if want != REQUESTS[-1] else (0,)):
            label = "stream n%d phase %g m%d avg%d L%d %s" % (n, phase, model, avg, L, "+".join(want))
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)

            def call(sentinel):
                g.set(sentinel)
                o = _Out(eng, U, want, model)
                _, cnt = eng.preintegrate_stream(g.s, g.u, dl, dq, prm, want=want, N=N, out=o.views, return_counts=True)
                return o.host(label), cnt.cpu().numpy()
            got, cnt = _twice(call, label)
            assert np.array_equal(cnt, count) and set(got) == _keys(model, want), label
            _add(t, got, ref, _fields(model, want), label)
            _p_sym(got, label)
            b = _Out(eng, U, want, model)
            eng.preintegrate(ck, dl, dq, prm, want=want, first=cf, count=cc, N=N, out=b.views)
            unequal += _differ(b.host(label + " batch"), got, label + ": the batch call on the host-assembled windows")
            one = _Out(eng, U, want, model)
            eng.preintegrate_streams(g.s, [0, len(s)], g.u, [0, U], dl, dq, prm, want=want, N=N, out=one.views)
            unequal += _differ(one.host(label + " R = 1"), got, label + ": one run is the single-stream entry")
            if L and want != REQUESTS[-1]:
                host, hc = eng.preintegrate_stream_host(_cpu(s), _cpu(u), _cpu(lin), _cpu(q), prm, want=want, N=N, return_counts=True)
                assert np.array_equal(hc.numpy(), count) and set(host) == set(got), label
                unequal += _differ({k: v.numpy() for k, v in host.items()}, got, label + ": the host form")
    # ---- two runs
    s2, so, u2, uo, lin2, q2 = _pack(runs)
    parts = [mc.stream_windows(r[0], r[1]) for r in runs]
    assert parts[1][4] == N
    refs = [ref, mc.oracle_windows(model, avg, parts[1][3], runs[1][2], runs[1][3], parts[1][2], key=("stream", n, phase, 1))]
    ref2 = {k: np.concatenate([r[k] for r in refs]) for k in ref}
    k2 = np.concatenate([parts[0][0], parts[1][0]])
    f2 = np.concatenate([parts[0][1], parts[1][1] + len(parts[0][0])])
    c2 = np.concatenate([parts[0][2], parts[1][2]])
    g2 = _Guarded(eng, s2, u2)
    dl2, dq2, dso, duo = _dev(lin2, eng), _dev(q2, eng), _dev(so, eng), _dev(uo, eng)
    ck2, cf2, cc2 = _dev(k2, eng), _dev(f2, eng), _dev(c2, eng)
    for want in REQUESTS[:2]:
        for L in STREAM_LANES:
            label = "runs n%d phase %g m%d avg%d L%d %s" % (n, phase, model, avg, L, "+".join(want))
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)

            def call(sentinel):
                g2.set(sentinel)
                o = _Out(eng, 2 * U, want, model)
                _, cnt = eng.preintegrate_streams(g2.s, dso, g2.u, duo, dl2, dq2, prm, want=want, N=N, out=o.views, return_counts=True)
                return o.host(label), cnt.cpu().numpy()
            got, cnt = _twice(call, label)
            assert np.array_equal(cnt, c2) and set(got) == _keys(model, want), label
            _add(t, got, ref2, _fields(model, want), label)
            b = _Out(eng, 2 * U, want, model)
            eng.preintegrate(ck2, dl2, dq2, prm, want=want, first=cf2, count=cc2, N=N, out=b.views)
            unequal += _differ(b.host(label + " batch"), got, label + ": the batch call on the host-assembled windows")
            if L:
                for r, (sr, ur, linr, qr) in enumerate(runs):
                    alone = _Out(eng, U, want, model)
                    eng.preintegrate_stream(_dev(sr, eng), _dev(ur, eng), _dev(linr, eng), _dev(qr, eng), prm, want=want, N=N, out=alone.views)
                    unequal += _differ(alone.host(label + " run alone"), {k: v[r * U:(r + 1) * U] for k, v in got.items()},
                                       label + ": run %d alone through the single-stream entry" % r)
                host, hc = eng.preintegrate_streams_host(_cpu(s2), so, _cpu(u2), uo, _cpu(lin2), _cpu(q2), prm, want=want, N=N, return_counts=True)
                assert np.array_equal(hc.numpy(), c2) and set(host) == set(got), label
                unequal += _differ({k: v.numpy() for k, v in host.items()}, got, label + ": the host form")
    t.report("[stream] preintegrate_stream / preintegrate_streams, mean_stream(%d, %g), model %d imu_avg %d, vs the oracle on the "
             "host-assembled windows" % (n, phase, model, avg), GATE["stream"])
    t.check(GATE["stream"], "stream entries n%d phase %g" % (n, phase))
    assert not unequal, "promised bit-equalities that do not hold: %s" % unequal


# ------------------------------------------------------------------------------------------------ d. the tiled entry
@pytest.mark.parametrize("N", [47, 65])
@pytest.mark.parametrize("mode", MODES)
def test_tiled_entry_split_across_wavefronts(eng, mode, N):
    """Engine.preintegrate_tiled on the tiles of Engine.tile_knots, with and without counts (the knots behind a window's count are
    NaN), lanes_per_window -- here: wavefronts per tile -- 0, 1, 2, 4, 5 and 8."""
    model, avg = mode
    kn, lin, q = mc.mean_edge_windows(N)
    W = kn.shape[0]
    _, _, count, given = _ragged_layout(kn, mc.MEAN_LAYOUT_SEED, garbage=True)
    holes = kn.copy()
    for w in range(W):
        holes[w, int(count[w]) + 1:] = np.nan
    dl, dq = _dev(lin, eng), _dev(q, eng)
    cases = [("whole", eng.tile_knots(_dev(kn, eng)), None, mc.oracle_windows(model, avg, kn, lin, q, key=("dense", N))),
             ("counted", eng.tile_knots(_dev(holes, eng)), _dev(given, eng), mc.oracle_windows(model, avg, kn, lin, q, count, key=("ragged", N)))]
    t = FieldTable(MEAN)
    for name, tiles, cnt, ref in cases:
        for S in TILE_SPLITS:
            label = "tiled %s N%d m%d avg%d S%d" % (name, N, model, avg, S)
            o = _Out(eng, W, ("mean",), model)
            eng.preintegrate_tiled(tiles, W, dl, dq, eng.make_params(model, bool(avg), lanes_per_window=S), count=cnt, out=o.views)
            got = o.host(label)
            assert set(got) == set(MEAN), label
            t.add(got, ref, label)
            if S == 1 and cnt is None:
                d = _Out(eng, W, ("mean",), model)
                eng.preintegrate(_dev(kn, eng), dl, dq, eng.make_params(model, bool(avg), lanes_per_window=1), want=("mean",), out=d.views)
                d = d.host(label + " dense")
                print("observed: one wavefront per tile bit-equal to the dense one-lane kernel: %s" % all(_bits_equal(d[k], got[k]) for k in MEAN))
    t.report("[tiled] Engine.preintegrate_tiled, mean_edge_windows(%d), model %d imu_avg %d, vs the oracle" % (N, model, avg), GATE["tiled"])
    t.check(GATE["tiled"], "tiled entry N%d" % N)


# ------------------------------------------------------------------------------------------------ e. the three-knot kernel
def _mean_out(eng, W, model):
    out = eng.alloc_outputs(W, ("mean",), model)
    for v in out.values():
        v.fill_(float("nan"))
    return out


@pytest.mark.parametrize("model", [1, 2])
def test_three_knot_kernel_dense(eng, model):
    """700 003 dense windows of 17 intervals, one lane per window, mean-only: the launcher's BIG instantiation (five chunks of three
    knots and a padded last one).  The batch is a base of 191 tumbling windows indexed by w % 191 on the device -- 191 is prime, so
    every base window visits every lane position.  Bit for bit the two-knot kernel (the same call with full counts:
    tests/test_gpu_parity.py) and out[w] == out[w % 191]; the first 191 and the last 70 windows against the oracle."""
    W, N, B = mc.BIG_DENSE
    kn, lin, q = mc.big_dense_base()
    idx = torch.arange(W, device=eng.device) % B
    dk, dl, dq = _dev(kn, eng)[idx].contiguous(), _dev(lin, eng)[idx].contiguous(), _dev(q, eng)[idx].contiguous()
    full = torch.full((W,), N, dtype=torch.int32, device=eng.device)
    sel = np.concatenate([np.arange(B), np.arange(W - 70, W)])
    t = FieldTable(MEAN)
    for avg in (0, 1):
        prm = eng.make_params(model, bool(avg), lanes_per_window=1)
        big = eng.preintegrate(dk, dl, dq, prm, want=("mean",), out=_mean_out(eng, W, model))
        two = eng.preintegrate(dk, dl, dq, prm, want=("mean",), count=full, out=_mean_out(eng, W, model))
        torch.cuda.synchronize()
        for k in MEAN:
            assert torch.isfinite(big[k]).all() and torch.equal(big[k], two[k]), (model, avg, k, "three knots per chunk vs two")
            assert torch.equal(big[k], big[k][:B][idx]), (model, avg, k, "a window's result depends on where it stands in the batch")
        ref = mc.oracle_windows(model, avg, kn, lin, q, key=("big dense",))
        t.add({k: big[k][torch.from_numpy(sel).to(eng.device)].cpu().numpy() for k in MEAN}, {k: ref[k][sel % B] for k in MEAN},
              "big dense m%d avg%d" % (model, avg))
    t.report("[big] BIG dense, %d windows of %d intervals over a base of %d, model %d, vs the oracle" % (W, N, B, model), GATE["big"])
    t.check(GATE["big"], "three-knot kernel, dense, model %d" % model)


@pytest.mark.parametrize("model", [1, 2])
def test_three_knot_kernel_stream(eng, model):
    """100 003 update times with 16 whole intervals and a tail each, ramped gyro, one lane per window, mean-only: model 1 takes the
    BIG instantiations of the stream entries (CUT = 2; CUT = 3 through preintegrate_streams with one run, which must give the same
    bits), model 2 -- admitted from 700 000 windows only -- the two-knot kernel on the uniform-grid fast path with the tail peeled
    off.  The first 130 windows, the last 70 and every 1013th against the oracle on the host-assembled windows."""
    U, n, phase = mc.BIG_STREAM
    s, u, lin, q = mc.big_stream()
    sel = np.unique(np.concatenate([np.arange(130), np.arange(U - 70, U), np.arange(0, U, 1013)]))
    dense = np.zeros((len(sel), n + 2, 7))
    for i, w in enumerate(sel):             # window w from the readings around it: the update before it, then its own
        a = max(w * n - 1, 0)
        kk, ff, cc = mc.st.assemble_windows(s[a:(w + 1) * n + 2], u[max(w - 1, 0):w + 1])
        assert cc[-1] == n + 1
        dense[i] = kk[ff[-1]:ff[-1] + n + 2]
    ds, du, dl, dq = _dev(s, eng), _dev(u, eng), _dev(lin, eng), _dev(q, eng)
    pick = torch.from_numpy(sel).to(eng.device)
    t = FieldTable(MEAN)
    for avg in (0, 1):
        prm = eng.make_params(model, bool(avg), lanes_per_window=1)
        got, cnt = eng.preintegrate_stream(ds, du, dl, dq, prm, want=("mean",), N=n + 1, out=_mean_out(eng, U, model), return_counts=True)
        one = eng.preintegrate_streams(ds, [0, len(s)], du, [0, U], dl, dq, prm, want=("mean",), N=n + 1, out=_mean_out(eng, U, model))
        torch.cuda.synchronize()
        assert bool((cnt == n + 1).all())
        for k in MEAN:
            assert torch.isfinite(got[k]).all() and torch.equal(got[k], one[k]), (model, avg, k, "one run is the single-stream entry")
        ref = mc.oracle_windows(model, avg, dense, lin[sel], q[sel])
        t.add({k: got[k][pick].cpu().numpy() for k in MEAN}, ref, "big stream m%d avg%d" % (model, avg))
    t.report("[big] BIG stream, %d windows of %d intervals and a tail, model %d, %d windows vs the oracle" % (U, n, model, len(sel)), GATE["big"])
    t.check(GATE["big"], "three-knot kernel, stream, model %d" % model)
