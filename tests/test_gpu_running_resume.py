"""GPU: running preintegration from a carry record (cpi_preintegrate_running_resume, Engine.preintegrate_running_resume[_host],
_CpiBase.read_rows, cpi_host::CpiBase::read_rows) -- IMU-rate rows for windows that arrive in chunks.

References: the C restatement's trace of the WHOLE window, oracle_py.oracle().trace (contractual gates of tests/tol.py through
check_pre: 1e-9 / 1e-8 / 1e-6), and the compiled reference's pinned traces tests/golden/trace_v*.npz (regression gates).  Every
row of every window of every segment is compared: the rows of segment c with trace rows cut_c .. cut_{c+1} - 1, the rows past a
segment's count with the state at its end.  The largest error per field is printed (pytest -s)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import synth
from oracle import oracle_py as op
from tests.test_gpu_running import JAC, LANES, MEAN, MODES, _check_rows, _dev, _host, _keys, _ragged, _wants, _Worst, trace_rows
from tests.tol import TOL_FACTOR, check_pre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = {1: ("mean", "jac", "cov", "cov_sym"), 2: ("mean", "cov", "cov_sym")}


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _cuts(rng, count, parts):
    """[W, parts + 1] per-window cut points 0 = c_0 <= ... <= c_parts = count[w]; repeats are segments of 0 intervals."""
    W = len(count)
    inner = np.sort((rng.random((W, parts - 1)) * (count[:, None] + 1)).astype(np.int64), axis=1)
    inner[0] = 0                                            # window 0: every segment but the last is empty
    if W > 1:
        inner[1] = count[1]                                 # window 1: every segment but the first is empty
    return np.concatenate([np.zeros((W, 1), np.int64), inner, count[:, None].astype(np.int64)], axis=1)


def _segment_ref(ref, lo, hi, Ns):
    """Rows of a segment [lo[w], hi[w]) of the whole-window rows ref [W, N, ...] as the entry must return them: Ns rows per
    window, row i = whole-window row lo + i, rows past the segment's count = the state at its end (hi = 0: the zero state)."""
    W = len(lo)
    idx = np.minimum(lo[:, None] + np.arange(Ns)[None, :], hi[:, None] - 1) + 1        # into the rows with the zero state in front
    out = {}
    for k, v in ref.items():
        zero = np.zeros((W, 1) + v.shape[2:])
        if k == "q":
            zero[..., 3] = 1.0
        vp = np.concatenate([zero, v], axis=1)
        out[k] = vp[np.arange(W)[:, None], idx]
    return out


def _run_chain(eng, prm, kn, lin, q, cuts, want, nan_rows=False):
    """Window w as a chain over the cut points cuts[w]: returns per segment (rows on the host, count, Ns) and the last record.
    nan_rows: the row arrays are filled with NaN before every call (a row the call does not write fails every comparison)."""
    W, n1, _ = kn.shape
    flat, base = _dev(kn.reshape(W * n1, 7), eng), np.arange(W, dtype=np.int64) * n1
    dl, dq = _dev(lin, eng), _dev(q, eng)
    carry, segs = None, []
    for c in range(cuts.shape[1] - 1):
        count = (cuts[:, c + 1] - cuts[:, c]).astype(np.int32)
        Ns = max(int(count.max()), 1)
        out = None
        if nan_rows:
            out = {k: v.fill_(float("nan")).view((W, Ns) + tuple(v.shape[1:]))
                   for k, v in eng.alloc_outputs(W * Ns, eng._running_want(tuple(want), prm.model), prm.model).items()}
        rows, carry = eng.preintegrate_running_resume(flat, dl, dq, prm, want=want, first=_dev(base + cuts[:, c], eng), count=_dev(count, eng), N=Ns,
                                                      carry_in=carry, out=out)
        segs.append((_host(rows), count, Ns))
    return segs, carry


def _check_chain(segs, ref, cuts, want, label, worst=None, regression=False):
    for c, (rows, count, Ns) in enumerate(segs):
        _check_rows(rows, _segment_ref(ref, cuts[:, c], cuts[:, c + 1], Ns), want, "%s segment %d" % (label, c), worst, regression)


def _live(model):
    """The parts of a record a full request writes (model 2 leaves the block of the analytic Jacobians alone; model 1's last
    double is padding)."""
    return [slice(0, 287)] if model == 1 else [slice(0, 17), slice(80, 566)]


def _record_fields(c, model):
    """The parts of carry records [W, cd] a caller can compare with a row without the device's rot_2_quat."""
    d = {"DT": c[:, 1], "alpha": c[:, 2:5], "beta": c[:, 5:8]}
    for i, k in enumerate(JAC):
        d[k] = c[:, 17 + 9 * i:26 + 9 * i]
    if model == 1:
        d["P"] = c[:, 62:287]
    return d


# --------------------------------------------------------------------------- 1. carry_in = None is preintegrate_running, bit for bit
@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("mode", MODES)
def test_null_carry_is_the_running_call(eng, mode, layout):
    model, avg = mode
    W, N = 203, 20
    if layout == "dense":
        kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=11))
        args = dict(knots=_dev(kn, eng))
    else:
        kn, lin, q, flat, first, count, given = _ragged(W, N, 12, garbage=True)
        args = dict(knots=_dev(flat, eng), first=_dev(first, eng), count=_dev(given, eng), N=N)
    dl, dq = _dev(lin, eng), _dev(q, eng)
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        for want in _wants(model):
            a = _host(eng.preintegrate_running(lin=dl, q_k_lin=dq, params=prm, want=want, **args))
            rows, carry = eng.preintegrate_running_resume(lin=dl, q_k_lin=dq, params=prm, want=want, **args)
            b = _host(rows)
            assert set(a) == set(b)
            for k in a:
                assert np.array_equal(a[k], b[k]), (mode, layout, L, want, k)
            rec = _record_fields(carry.cpu().numpy(), model)
            for k in _keys(want):
                if k in rec and (k != "P" or model == 1):
                    assert np.array_equal(rec[k], b[k][:, N - 1]), ("record vs row N - 1", mode, layout, L, want, k)


# --------------------------------------------------------------------------- 2. chains vs the whole-window trace
@pytest.mark.parametrize("mode", MODES)
def test_chains_match_the_oracle_trace(eng, mode):
    model, avg = mode
    W, N = 203, 20
    worst, bit_equal = _Worst(), []
    for layout, seed in (("dense", 11), ("ragged", 12)):
        if layout == "dense":
            kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=seed))
            count = np.full(W, N, np.int64)
        else:
            kn, lin, q, _, _, count, _ = _ragged(W, N, seed)
        ref = trace_rows(model, avg, kn, lin, q, count)
        rng = np.random.default_rng(1000 * model + 100 * avg + seed)
        for parts in (2, 3, 5):
            cuts = _cuts(rng, count.astype(np.int64), parts)
            for L in LANES:
                prm = eng.make_params(model, bool(avg), lanes_per_window=L)
                for want in _wants(model):
                    label = "chain m%d avg%d %s parts%d L%d %s" % (model, avg, layout, parts, L, "+".join(want))
                    segs, _ = _run_chain(eng, prm, kn, lin, q, cuts, want)
                    _check_chain(segs, ref, cuts, want, label, worst)
                    if L == 1 and layout == "dense":
                        one = _host(eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=want))
                        eq = True
                        for c, (rows, cnt, Ns) in enumerate(segs):
                            exp = _segment_ref(one, cuts[:, c], cuts[:, c + 1], Ns)
                            eq = eq and all(np.array_equal(rows[k], exp[k]) for k in _keys(want))
                        bit_equal.append(("parts%d %s" % (parts, "+".join(want)), eq))
    worst.report("running_resume chains vs oracle.trace, model %d imu_avg %d" % (model, avg))
    print("one-lane chains bit-equal to the one-shot running call: %s" % ", ".join("%s: %s" % be for be in bit_equal))


def test_chains_match_the_golden_traces(eng, golden_dir):
    worst = _Worst()
    for model in (1, 2):
        d = np.load(os.path.join(golden_dir, "trace_v%d.npz" % model))
        ref = {k: d[k][None] for k in MEAN + JAC + ("P",)}
        kn, lin, q = d["knots"][None], d["lin"][None], d["q_k_lin"][None]
        n = kn.shape[1] - 1
        rng = np.random.default_rng(model)
        for parts in (2, 3, 5):
            cuts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, size=parts - 1)), [n]]).astype(np.int64)[None]
            for L in LANES:
                for want in _wants(model):
                    segs, _ = _run_chain(eng, eng.make_params(model, lanes_per_window=L), kn, lin, q, cuts, want)
                    _check_chain(segs, ref, cuts, want, "golden m%d parts%d L%d %s" % (model, parts, L, "+".join(want)), worst, True)
    worst.report("running_resume chains vs golden traces")


# --------------------------------------------------------------------------- 3. the record is the state of row N - 1
@pytest.mark.parametrize("mode", MODES)
def test_record_and_last_row_agree_across_calls(eng, mode):
    model, avg = mode
    W, N = 131, 20
    kn, lin, q, _, _, count, _ = _ragged(W, N, 31)
    want = FULL[model]
    dl, dq = _dev(lin, eng), _dev(q, eng)
    still = kn[:, :6].copy()
    still[:, :, 0] = still[:, :1, 0]                        # a segment whose every interval has dt = 0
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        rows, carry = eng.preintegrate_running_resume(_dev(kn, eng), dl, dq, prm, want=want, count=_dev(count.astype(np.int32), eng))
        rows = _host(rows)
        last = {k: v[:, N - 1] for k, v in rows.items()}
        rec = _record_fields(carry.cpu().numpy(), model)
        for k in _keys(want):
            if k in rec and (k != "P" or model == 1):
                assert np.array_equal(rec[k], last[k]), (mode, L, k)
        zero = _dev(np.zeros(W, np.int32), eng)
        for label, kw in (("count 0", dict(knots=_dev(kn[:, :6], eng), count=zero)), ("dt 0", dict(knots=_dev(still, eng)))):
            r2, c2 = eng.preintegrate_running_resume(lin=dl, q_k_lin=dq, params=prm, want=want, carry_in=carry, **kw)
            r3, c3 = eng.preintegrate_running_resume(lin=dl, q_k_lin=dq, params=prm, want=want, carry_in=c2, **kw)
            for r in (_host(r2), _host(r3)):
                for k in _keys(want) + ("P_sym",):
                    for i in range(5):
                        assert np.array_equal(r[k][:, i], last[k]), (mode, L, label, k, i)
            assert torch.equal(c2[:, 0], carry[:, 0]) and torch.equal(c3[:, 0], carry[:, 0])


@pytest.mark.parametrize("mode", MODES)
def test_repeat_rows_are_exact_on_and_next_to_a_cut(eng, mode):
    """dt = 0, a backward stamp and a NaN separator on and beside the cut: the repeated rows equal the row before them, across
    the call boundary too (row 0 of a segment repeats the last row of the previous call)."""
    from tests.test_gpu_running import _skipping_windows
    model, avg = mode
    N = 20
    kn, lin, q, skipped = _skipping_windows(N, 14)
    W = kn.shape[0]
    ref = trace_rows(model, avg, kn, lin, q)
    want = FULL[model]
    cuts = np.zeros((W, 3), np.int64)
    cuts[:, 2] = N
    for w in range(W):                                      # the cut ON the first skipped interval, just before or just after it
        s = skipped[w][0] if skipped[w] else w % N
        cuts[w, 1] = min(max(s + (w // 4) % 3 - 1 + 1, 0), N)
    for L in LANES:
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        segs, _ = _run_chain(eng, prm, kn, lin, q, cuts, want)
        _check_chain(segs, ref, cuts, want, "skips at cuts m%d avg%d L%d" % (model, avg, L))
        for k in _keys(want) + ("P_sym",):
            whole = np.zeros((W, N) + segs[0][0][k].shape[2:])
            for w in range(W):
                c = cuts[w, 1]
                whole[w, :c] = segs[0][0][k][w, :c]
                whole[w, c:] = segs[1][0][k][w, :N - c]
            for w in range(W):
                for i in skipped[w]:
                    if i > 0:
                        assert np.array_equal(whole[w, i], whole[w, i - 1]), (k, L, w, i, int(cuts[w, 1]))


# --------------------------------------------------------------------------- 4. the two resume entries share their records
@pytest.mark.parametrize("mode", MODES)
def test_records_interchange_with_preintegrate_resume(eng, mode):
    model, avg = mode
    W, N = 67, 20
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=41))
    ref = trace_rows(model, avg, kn, lin, q)
    final = {k: v[:, N - 1] for k, v in ref.items()}
    rwant = ("mean", "jac", "cov") if model == 1 else ("mean", "cov")
    dl, dq = _dev(lin, eng), _dev(q, eng)
    for L in (0, 1, 4):
        prm = eng.make_params(model, bool(avg), lanes_per_window=L)
        a, b = _dev(kn[:, :9], eng), _dev(kn[:, 8:], eng)
        _, carry = eng.preintegrate_running_resume(a, dl, dq, prm, want=rwant)
        out, _ = eng.preintegrate_resume(b, dl, dq, prm, want=rwant, carry_in=carry)
        check_pre(_host(out), final, what=rwant, label="running_resume -> resume m%d avg%d L%d" % (model, avg, L))
        _, carry = eng.preintegrate_resume(a, dl, dq, prm, want=("mean", "jac", "cov"))
        rows, _ = eng.preintegrate_running_resume(b, dl, dq, prm, want=rwant, carry_in=carry)
        _check_rows(_host(rows), {k: v[:, 8:] for k, v in ref.items()}, rwant, "resume -> running_resume m%d avg%d L%d" % (model, avg, L))


def test_model2_jacobians_after_a_running_chain(eng, golden_dir):
    d = np.load(os.path.join(golden_dir, "trace_v2.npz"))
    kn, lin, q = (_dev(d[k][None], eng) for k in ("knots", "lin", "q_k_lin"))
    n = d["knots"].shape[0] - 1
    prm = eng.make_params(2)
    carry = None
    for lo in range(0, n, 7):
        _, carry = eng.preintegrate_running_resume(kn[:, lo:min(lo + 7, n) + 1].contiguous(), lin, q, prm, want=("mean", "cov"), carry_in=carry)
    out, _ = eng.preintegrate_resume(kn[:, n:].contiguous(), lin, q, prm, want=("mean", "jac", "cov"), carry_in=carry)
    ref = {k: d[k][-1:] for k in d.files if k not in ("knots", "lin", "q_k_lin")}
    check_pre(_host(out), ref, v2=True, label="model-2 Jacobians from a zero-interval resume after a running chain", regression=True)


# --------------------------------------------------------------------------- 5. tag mismatch
@pytest.mark.parametrize("model", [1, 2])
def test_tag_mismatch_poisons_exactly_those_windows(eng, model):
    W, N = 70, 20
    kn, lin, q = synth.make_windows(W, N, seed=77, device=eng.device)
    a, b = kn[:, :9].contiguous(), kn[:, 8:].contiguous()
    want = FULL[model]
    other_tag = float(1 + 2 + 4 + (16 if model == 1 else 0) + 32 * (3 - model))   # a full record that says it is the other model's
    for L in (0, 1, 3, 64):
        prm = eng.make_params(model, lanes_per_window=L)
        _, full = eng.preintegrate_running_resume(a, lin, q, prm, want=want)
        _, means = eng.preintegrate_running_resume(a, lin, q, prm, want=("mean",))
        _, other = eng.preintegrate_running_resume(a, lin, q, eng.make_params(model, imu_avg=True, lanes_per_window=L), want=want)
        mixed = full.clone()
        bad = np.zeros(W, bool)
        bad[0::3] = True
        for j, w in enumerate(np.nonzero(bad)[0]):
            kind = j % 5
            if kind == 0:
                mixed[w] = means[w]                         # a means-only record, P wanted
            elif kind == 1:
                mixed[w] = other[w]                         # imu_avg differs
            elif kind == 2:
                mixed[w, 0] = other_tag
            elif kind == 3:
                mixed[w, 0] = 0.0
            else:
                mixed[w, 0] = float("nan")
        before = mixed.clone()
        clean, cc = eng.preintegrate_running_resume(b, lin, q, prm, want=want, carry_in=full)
        rows, carry = eng.preintegrate_running_resume(b, lin, q, prm, want=want, carry_in=mixed)
        clean, rows, c, cc = _host(clean), _host(rows), carry.cpu().numpy(), cc.cpu().numpy()
        assert torch.equal(mixed.view(torch.int64), before.view(torch.int64)), "carry_in is read only"
        for k, v in rows.items():
            assert np.all(np.isnan(v[bad])), (model, L, k)
            assert np.array_equal(v[~bad], clean[k][~bad]), (model, L, k)
        assert np.all(np.isnan(c[bad, 0])) and np.array_equal(c[~bad, :17], cc[~bad, :17])
        rows, _ = eng.preintegrate_running_resume(b, lin, q, prm, want=("mean",), carry_in=full)   # needs the means only: fine
        assert all(np.all(np.isfinite(v)) for v in _host(rows).values())


# --------------------------------------------------------------------------- 6. guard bands
@pytest.mark.parametrize("mode", MODES)
def test_writes_nothing_outside_rows_and_records(eng, mode):
    model, avg = mode
    N, G, SENT = 10, 4096, -7.25
    want = FULL[model]
    cd = eng.carry_doubles(model)
    for W in (1, 67, 130):
        kn, lin, q, flat, first, count, given = _ragged(W, N, 15 + W, garbage=True)
        ref = trace_rows(model, avg, kn, lin, q, count)
        half = count // 2
        for L in (0, 1, 3, 5, 6, 12, 64):
            prm = eng.make_params(model, bool(avg), lanes_per_window=L)
            _, cin = eng.preintegrate_running_resume(_dev(flat, eng), _dev(lin, eng), _dev(q, eng), prm, want=want, first=_dev(first, eng),
                                                     count=_dev(half.astype(np.int32), eng), N=N)
            keep = cin.clone()
            bufs, views = {}, {}
            for k, v in eng.alloc_outputs(W * N, want, model).items():
                n = v[0].numel()
                bufs[k] = torch.full((2 * G + W * N * n,), SENT, dtype=torch.float64, device=eng.device)
                views[k] = bufs[k][G:G + W * N * n].view((W, N) + tuple(v.shape[1:]))
            cbuf = torch.full((2 * G + W * cd,), SENT, dtype=torch.float64, device=eng.device)
            given2 = (count - half).astype(np.int32)
            given2[0::7] = np.where(given2[0::7] == 0, -1 - np.arange(len(given2[0::7])), given2[0::7])   # garbage: clamped to 0
            rows, cout = eng.preintegrate_running_resume(_dev(flat, eng), _dev(lin, eng), _dev(q, eng), prm, want=want,
                                                         first=_dev(first + half, eng), count=_dev(given2, eng), N=N, carry_in=cin,
                                                         carry_out=cbuf[G:G + W * cd].view(W, cd), out=views)
            got = _host(rows)
            exp = _segment_ref(ref, half.astype(np.int64), count.astype(np.int64), N)
            _check_rows(got, exp, want, "guards m%d avg%d W%d L%d" % (model, avg, W, L))
            for k, bb in bufs.items():
                assert torch.all(bb[:G] == SENT) and torch.all(bb[-G:] == SENT), (k, W, L)
            assert torch.all(cbuf[:G] == SENT) and torch.all(cbuf[-G:] == SENT), (W, L)
            assert torch.equal(cin.view(torch.int64), keep.view(torch.int64)), (W, L)


# --------------------------------------------------------------------------- 7. both sides of the launch policy
@pytest.mark.parametrize("mode", MODES)
def test_on_both_sides_of_the_launch_policy(eng, mode):
    """Automatic lane choice at N = 4 per call (1 or 2 lanes): windows of 8 intervals as a chain of 4 + 4, at one window, one
    wavefront, and 1 024 wavefronts of two lanes per window - 1 / exactly / + 1 window."""
    model, avg = mode
    N, Wmax = 4, 32769
    kn, lin, q = (t.numpy() for t in synth.make_windows(Wmax, 2 * N, seed=13))
    ref = trace_rows(model, avg, kn, lin, q, key="policy 4 + 4")
    prm = eng.make_params(model, bool(avg))
    worst = _Worst()
    for W in (1, 31, 32, 33, 32767, 32768, 32769):
        for want in _wants(model):
            dk, dl, dq = _dev(kn[:W], eng), _dev(lin[:W], eng), _dev(q[:W], eng)
            r1, carry = eng.preintegrate_running_resume(dk[:, :N + 1].contiguous(), dl, dq, prm, want=want)
            r2, _ = eng.preintegrate_running_resume(dk[:, N:].contiguous(), dl, dq, prm, want=want, carry_in=carry)
            h1, h2 = _host(r1), _host(r2)
            got = {k: np.concatenate([h1[k], h2[k]], axis=1) for k in h1}
            _check_rows(got, {k: v[:W] for k, v in ref.items()}, want, "policy m%d avg%d W%d %s" % (model, avg, W, "+".join(want)), worst)
    worst.report("running_resume at the launch-policy switches, model %d imu_avg %d" % (model, avg))


# --------------------------------------------------------------------------- 8. graph capture on one stream
def test_graph_capture_and_replay(eng):
    W, N = 300, 20
    kn, lin, q = synth.make_windows(W, N, seed=17, device=eng.device)
    first = kn[:, :11].contiguous()
    seg = kn[:, 10:].contiguous()
    for model in (1, 2):
        prm = eng.make_params(model)
        want = FULL[model]
        _, cin = eng.preintegrate_running_resume(first, lin, q, prm, want=want)
        out, cout = eng.preintegrate_running_resume(seg, lin, q, prm, want=want, carry_in=cin)

        def call():
            eng.preintegrate_running_resume(seg, lin, q, prm, want=want, carry_in=cin, carry_out=cout, out=out)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            call()
        torch.cuda.synchronize()
        eager = {k: v.clone() for k, v in out.items()}
        eager_c = cout.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for v in out.values():
            v.zero_()
        cout.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], eager[k]), k
        for sl in _live(model):
            assert torch.equal(cout[:, sl], eager_c[:, sl])
        seg[:, :, 1:4] *= 1.01                              # new measurements and a new record in the same buffers
        first2 = first.clone()
        first2[:, :, 1:4] *= 0.99
        _, cin2 = eng.preintegrate_running_resume(first2, lin, q, prm, want=want)
        cin.copy_(cin2)
        g.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        replayed_c = cout.clone()
        call()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], replayed[k]), k
            assert k == "DT" or not torch.equal(out[k], eager[k]), k    # (the stamps did not change)
        for sl in _live(model):
            assert torch.equal(cout[:, sl], replayed_c[:, sl])


# --------------------------------------------------------------------------- 9. the host entry
@pytest.mark.parametrize("mode", MODES)
def test_host_entry_equals_the_device_entry(eng, mode):
    model, avg = mode
    prm = eng.make_params(model, bool(avg), lanes_per_window=1)
    want = FULL[model]
    for W, N in ((50, 20), (4500, 30)):
        kn, lin, q = synth.make_windows(W, N, seed=18)
        cut = N // 2
        count = torch.from_numpy((np.arange(W) * 5 % (N - cut + 1)).astype(np.int32))
        a, b = kn[:, :cut + 1].contiguous(), kn[:, cut:].contiguous()
        _, hc = eng.preintegrate_running_resume_host(a, lin, q, prm, want=want)
        _, dc = eng.preintegrate_running_resume(a.to(eng.device), lin.to(eng.device), q.to(eng.device), prm, want=want)
        torch.cuda.synchronize()
        for sl in _live(model):
            assert np.array_equal(hc.numpy()[:, sl], dc.cpu().numpy()[:, sl])
        for cnt in (None, count):
            got, hc2 = eng.preintegrate_running_resume_host(b, lin, q, prm, want=want, count=cnt, carry_in=hc)
            dev, dc2 = eng.preintegrate_running_resume(b.to(eng.device), lin.to(eng.device), q.to(eng.device), prm, want=want,
                                                       count=None if cnt is None else cnt.to(eng.device), carry_in=dc)
            dev = _host(dev)
            for k in dev:
                assert np.array_equal(got[k].numpy(), dev[k]), (k, W, cnt is None)
            for sl in _live(model):
                assert np.array_equal(hc2.numpy()[:, sl], dc2.cpu().numpy()[:, sl]), (W, cnt is None)
        if W <= 100:
            ref = trace_rows(model, avg, kn.numpy(), lin.numpy(), q.numpy(), (cut + count.numpy()))
            _check_rows({k: v.numpy() for k, v in got.items()}, {k: v[:, cut:] for k, v in ref.items()}, want, "host m%d avg%d" % (model, avg))


# --------------------------------------------------------------------------- 10. argument checks
def test_argument_checks(eng):
    from cpi_amd import CpiError
    W, N = 8, 5
    kn, lin, q = synth.make_windows(W, N, seed=19, device=eng.device)
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_running_resume(kn, lin, q, eng.make_params(3), want=("mean",),
                                        carry_out=torch.zeros((W, 288), dtype=torch.float64, device=eng.device))
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_running_resume(kn, lin, q, eng.make_params(2), want=("mean", "jac"))
    with pytest.raises(CpiError, match="Forster"):
        eng.preintegrate_running_resume_host(kn.cpu(), lin.cpu(), q.cpu(), eng.make_params(3), want=("mean",),
                                             carry_out=torch.zeros((W, 288), dtype=torch.float64))
    with pytest.raises(CpiError, match="not available for model 2"):
        eng.preintegrate_running_resume_host(kn.cpu(), lin.cpu(), q.cpu(), eng.make_params(2), want=("jac",))
    with pytest.raises(CpiError, match="q_k_lin"):
        eng.preintegrate_running_resume(kn, lin, None, eng.make_params(2), want=("mean",))
    with pytest.raises(CpiError, match="lanes_per_window"):
        eng.preintegrate_running_resume(kn, lin, q, eng.make_params(1, lanes_per_window=7), want=("mean",))
    prm = eng.make_params(1)
    buf = torch.zeros((20, 288), dtype=torch.float64, device=eng.device)
    with pytest.raises(CpiError, match="overlap"):
        eng.preintegrate_running_resume(kn, lin, q, prm, carry_in=buf[:8], carry_out=buf[4:12])
    o = eng._outputs_struct(eng.alloc_outputs(W * N, ("mean",), 1))
    rc = eng.lib.cpi_preintegrate_running_resume(eng.ctx, C.byref(prm), W, N, C.c_void_p(kn.data_ptr()), None, None,
                                                 C.c_void_p(lin.data_ptr()), C.c_void_p(q.data_ptr()), None, None, C.byref(o))
    assert rc == 1 and b"carry_out" in eng.lib.cpi_last_error(eng.ctx)
    big = torch.zeros((1, 65537, 7), dtype=torch.float64, device=eng.device)
    with pytest.raises(CpiError, match="65535"):
        eng.preintegrate_running_resume(big, lin[:1], q[:1], prm, want=("mean",),
                                        out={"DT": torch.zeros((1, 65536), dtype=torch.float64, device=eng.device)})
    # W == 0 writes nothing
    sent = {"DT": torch.full((4,), 3.0, dtype=torch.float64, device=eng.device)}
    rec = torch.full((4, 288), 5.0, dtype=torch.float64, device=eng.device)
    eng.preintegrate_running_resume(kn[:0], lin[:0], q[:0], prm, out=sent, carry_out=rec)
    torch.cuda.synchronize()
    assert torch.all(sent["DT"] == 3.0) and torch.all(rec == 5.0)
    # N == 0 writes no rows and passes the state through: the zero state for no record, the record's state otherwise
    for model in (1, 2):
        prm = eng.make_params(model)
        want = FULL[model]
        sent = {k: torch.full((4,), 3.0, dtype=torch.float64, device=eng.device) for k in _keys(want) + ("P_sym",)}
        knot0 = kn[:, :1].contiguous()
        _, c0 = eng.preintegrate_running_resume(knot0, lin, q, prm, out=sent)
        torch.cuda.synchronize()
        assert all(torch.all(v == 3.0) for v in sent.values())
        c0 = c0.cpu().numpy()
        assert np.all(c0[:, 1:8] == 0.0) and np.array_equal(c0[:, 8:17], np.tile(np.eye(3).reshape(-1), (W, 1))) and np.all(c0[:, 0] >= 1)
        rows, c1 = eng.preintegrate_running_resume(kn, lin, q, prm, want=want)
        _, c2 = eng.preintegrate_running_resume(knot0, lin, q, prm, out=sent, carry_in=c1)
        again, _ = eng.preintegrate_running_resume(kn[:, :3].contiguous(), lin, q, prm, want=want, carry_in=c2,
                                                   count=torch.zeros(W, dtype=torch.int32, device=eng.device))
        rows, again = _host(rows), _host(again)
        assert all(torch.all(v == 3.0) for v in sent.values())
        for k in rows:
            assert np.array_equal(again[k][:, 0], rows[k][:, N - 1]) and np.array_equal(again[k][:, 1], rows[k][:, N - 1]), (model, k)
    assert sorted(eng.preintegrate_running_resume(kn, lin, q, eng.make_params(2))[0]) == sorted(MEAN + ("P",))
    assert eng.lib.cpi_abi_version() == 3


# --------------------------------------------------------------------------- 11. rows feed predict
@pytest.mark.parametrize("model", [1, 2])
def test_rows_of_a_later_segment_feed_predict(eng, model):
    W, N, cut = 37, 20, 8
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=16))
    ref = trace_rows(model, 0, kn, lin, q)
    dl, dq = _dev(lin, eng), _dev(q, eng)
    prm = eng.make_params(model)
    _, carry = eng.preintegrate_running_resume(_dev(kn[:, :cut + 1], eng), dl, dq, prm, want=("mean",))
    rows, _ = eng.preintegrate_running_resume(_dev(kn[:, cut:], eng), dl, dq, prm, want=("mean",), carry_in=carry)
    Ns = N - cut
    meas = {k: v.reshape((W * Ns,) + tuple(v.shape[2:])) for k, v in rows.items()}
    zeros = torch.zeros((W, 3), dtype=torch.float64, device=eng.device)
    xi, _ = synth.make_states(zeros, zeros, torch.tensor([[0.0, 0, 0, 1]] * W, dtype=torch.float64, device=eng.device), zeros[:, 0], dl,
                              model, device=eng.device)
    idx = (torch.arange(W * Ns, device=eng.device) // Ns).to(torch.int32)
    got = eng.predict(model, meas, xi, idx_i=idx)
    torch.cuda.synchronize()
    flat = {k: ref[k][:, cut:].reshape((W * Ns,) + ref[k].shape[2:]) for k in MEAN}
    for k in JAC + (("O_a", "O_b") if model == 2 else ()):
        flat[k] = np.zeros((W * Ns, 9))
    sel = np.repeat(np.arange(W), Ns)
    rec = op.factor_records(flat, lin[sel], q[sel] if model == 2 else None)
    want = op.oracle().predict(model, rec, xi.cpu().numpy()[sel])
    assert np.abs(got.cpu().numpy() - want).max() <= TOL_FACTOR * max(1.0, np.abs(want).max())


# --------------------------------------------------------------------------- 12. the facades
def _feed_pattern(n):
    sizes, i = [], 0
    while sum(sizes) < n:
        sizes.append(min((1, 3, 7)[i % 3], n - sum(sizes)))
        i += 1
    return sizes


def _python_read_rows(eng, d, model):
    import cpi_amd
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    cpi = (cpi_amd.CpiV1 if model == 1 else cpi_amd.CpiV2)(0.005, 4e-6, 0.01, 2e-4, engine=eng)
    cpi.set_incremental(True)
    cpi.setLinearizationPoints(lin[:3], lin[3:], q, (0.0, 0.0, 9.8))
    assert cpi.read_rows() == []
    out, i = [], 0
    for size in _feed_pattern(kn.shape[0] - 1):
        for _ in range(size):
            a, b = kn[i], kn[i + 1]
            cpi.feed_IMU(a[0], b[0], a[1:4], a[4:7], b[1:4], b[4:7])
            i += 1
        rows = cpi.read_rows()
        assert len(rows) == size and len(cpi._iv) == 0
        out += rows
        assert np.array_equal(cpi.alpha_tau, rows[-1]["alpha"]) and cpi.DT == float(rows[-1]["DT"])
        assert np.array_equal(cpi.P_meas.T.reshape(225), rows[-1]["P"])
    return cpi, out


@pytest.mark.parametrize("model", [1, 2])
def test_python_read_rows_vs_trace(eng, golden_dir, model):
    import cpi_amd
    d = dict(np.load(os.path.join(golden_dir, "trace_v%d.npz" % model)))
    cpi, out = _python_read_rows(eng, d, model)
    keys = MEAN + (JAC if model == 1 else ()) + ("P",)
    got = {k: np.stack([r[k] for r in out])[None] for k in keys}
    ref = {k: d[k][None] for k in keys}
    want = ("mean", "jac", "cov") if model == 1 else ("mean", "cov")
    worst = _Worst()
    _check_rows(got, ref, want, "read_rows m%d" % model, worst, regression=True)
    worst.report("Python read_rows vs golden trace, model %d" % model)
    if model == 2:                                          # the members' Jacobians: out of the carried state-transition columns
        fin = {k: getattr(cpi, k).T.reshape(1, 9) for k in JAC + ("O_a", "O_b")}
        fin.update({"DT": np.array([cpi.DT]), "alpha": cpi.alpha_tau[None], "beta": cpi.beta_tau[None], "q": cpi.q_k2tau[None],
                    "P": cpi.P_meas.T.reshape(1, 225)})
        check_pre(fin, {k: d[k][-1:] for k in fin}, v2=True, label="members after read_rows", regression=True)
    plain = cpi_amd.CpiV1(0.005, 4e-6, 0.01, 2e-4, engine=eng)
    with pytest.raises(RuntimeError):
        plain.read_rows()
    with pytest.raises((ValueError, RuntimeError)):
        cpi_amd.ForsterDiscrete(0.005, 4e-6, 0.01, 2e-4, engine=eng).read_rows()


@pytest.mark.parametrize("model", [1, 2])
def test_cpp_read_rows_vs_trace_and_python(eng, golden_dir, model):
    """tests/cpp/test_running_resume.cpp: cpi_host::CpiV1 / CpiV2::read_rows with the same feed pattern -- every trace row at the
    regression gates, and bit for bit the rows of the Python mirror."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    d = dict(np.load(os.path.join(golden_dir, "trace_v%d.npz" % model)))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_running_resume")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_running_resume.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        path = os.path.join(tmp, "trace.bin")
        with open(path, "wb") as f:
            np.array([kn.shape[0]], dtype=np.float64).tofile(f)
            kn.tofile(f); lin.tofile(f); q.tofile(f)
        p = subprocess.run([exe, path, str(model)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-400:] + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
    n = kn.shape[0] - 1
    assert len(lines) == n and "GUARDS 1 1" in p.stdout.splitlines()
    vals = np.array([[float(x) for x in ln.split()[1:]] for ln in lines])
    keys = MEAN + (JAC if model == 1 else ()) + ("P",)
    widths = [1, 3, 3, 4] + ([9] * 5 if model == 1 else []) + [225]
    assert vals.shape[1] == sum(widths)
    got, o = {}, 0
    for k, wd in zip(keys, widths):
        got[k] = vals[:, o:o + wd].reshape((1, n) + ((wd,) if wd > 1 else ()))
        o += wd
    want = ("mean", "jac", "cov") if model == 1 else ("mean", "cov")
    _check_rows(got, {k: d[k][None] for k in keys}, want, "C++ read_rows m%d" % model, regression=True)
    _, py = _python_read_rows(eng, d, model)
    for k in keys:
        assert np.array_equal(got[k][0], np.stack([r[k] for r in py])), (model, k)


# --------------------------------------------------------------------------- 13. full size: 100 k x 50 as 25 + 25
@pytest.mark.parametrize("model", [1, 2])
def test_full_size_two_call_chain(eng, model):
    W, N = 100_000, 50
    kn, lin, q = synth.make_windows(W, N, seed=404 + model, device=eng.device)
    prm = eng.make_params(model)
    want = ("mean", "jac", "cov") if model == 1 else ("mean", "cov")
    one = _host(eng.preintegrate(kn, lin, q, prm, want=want))
    a, carry = eng.preintegrate_running_resume(kn[:, :26].contiguous(), lin, q, prm, want=want)
    sample = torch.arange(0, W, 997, device=eng.device)
    ra = {k: v[sample].cpu().numpy() for k, v in a.items()}
    del a
    b, _ = eng.preintegrate_running_resume(kn[:, 25:].contiguous(), lin, q, prm, want=want, carry_in=carry)
    torch.cuda.synchronize()
    last = {k: v[:, 24].cpu().numpy() for k, v in b.items()}
    check_pre(last, one, what=want, v2=(model == 2), label="100k x 50 as 25 + 25, last rows, model %d" % model, regression=True)
    rb = {k: v[sample].cpu().numpy() for k, v in b.items()}
    ref = trace_rows(model, 0, kn[sample].cpu().numpy(), lin[sample].cpu().numpy(), q[sample].cpu().numpy())
    worst = _Worst()
    _check_rows({k: np.concatenate([ra[k], rb[k]], axis=1) for k in ra}, ref, want, "100k x 50 sample, model %d" % model, worst)
    worst.report("full size 25 + 25 sample vs oracle.trace, model %d" % model)
