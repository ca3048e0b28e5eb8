"""GPU: resumable preintegration (cpi_preintegrate_resume, Engine.preintegrate_resume, the incremental mode of the Python
mirror and of the C++ facade).  A window integrated as a chain of calls, each continuing from the previous call's carry
record, must agree with one cpi_preintegrate_batch call on the whole window and with the compiled reference (regression
gates, tests/tol.py); a NULL carry_in must reproduce the batch call bit for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.tol import check_pre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, 0, 1), (1, 1, 1), (2, 0, 1), (2, 1, 1), (2, 0, 0), (2, 1, 0)]
WANTS = [("mean", "jac", "cov"), ("mean",), ("mean", "jac"), ("cov",)]


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _dev(a, eng):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _mode_out(d, m):
    key = "m%d_avg%d_stj%d__" % m
    return {k[len(key):]: v for k, v in d.items() if k.startswith(key)}


def _what(want):
    return tuple(w for w in ("mean", "jac", "cov") if w in want)


def _chain(eng, prm, kn, lin, q, cuts, want):
    """Integrates every window of the dense batch kn [W, N+1, 7] as a chain of calls on the ragged layout: call c covers
    knots cuts[:, c] .. cuts[:, c+1] of each window (consecutive segments share their boundary knot)."""
    W, n1, _ = kn.shape
    flat = _dev(kn.reshape(W * n1, 7), eng)
    base = np.arange(W, dtype=np.int64) * n1
    carry, out = None, None
    for c in range(cuts.shape[1] - 1):
        first = base + cuts[:, c]
        count = (cuts[:, c + 1] - cuts[:, c]).astype(np.int32)
        N = max(int(count.max()), 0)
        out, carry = eng.preintegrate_resume(flat, _dev(lin, eng), _dev(q, eng), prm, want=want, first=_dev(first, eng),
                                             count=_dev(count, eng), N=N, carry_in=carry)
    return _host(out), carry


def _random_cuts(rng, W, n, parts):
    inner = np.sort(rng.integers(0, n + 1, size=(W, parts - 1)), axis=1)   # repeats = empty segments
    inner[0] = 0   # window 0: every segment but the last is empty
    return np.concatenate([np.zeros((W, 1), np.int64), inner, np.full((W, 1), n, np.int64)], axis=1)


# --------------------------------------------------------------------------- 1. NULL carry_in == the batch call, bit for bit
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("lanes", [0, 3, 16])
def test_null_carry_is_the_batch_call(eng, mode, ragged, lanes):
    from cpi_amd import synth
    W, N = 100, 50
    kn, lin, q = synth.make_windows(W, N, seed=701 + mode[0] + 2 * mode[1], edge_cases=True)
    kn, lin, q = kn.numpy(), lin.numpy(), q.numpy()
    prm = eng.make_params(*mode, lanes_per_window=lanes)
    kw = {}
    if ragged:
        rng = np.random.default_rng(5)
        count = rng.integers(0, N + 1, size=W).astype(np.int32)
        kw = dict(first=_dev(np.arange(W, dtype=np.int64) * (N + 1), eng), count=_dev(count, eng), N=N)
        knd = _dev(kn.reshape(W * (N + 1), 7), eng)
    else:
        knd = _dev(kn, eng)
    for want in WANTS:
        a = _host(eng.preintegrate(knd, _dev(lin, eng), _dev(q, eng), prm, want=want, **kw))
        b, carry = eng.preintegrate_resume(knd, _dev(lin, eng), _dev(q, eng), prm, want=want, **kw)
        b = _host(b)
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (mode, ragged, lanes, want, k)
        c = carry.cpu().numpy()
        assert np.all(np.isfinite(c[:, :17])), "the means are always carried"


# --------------------------------------------------------------------------- 2. chains vs the golden outputs and the one-shot call
@pytest.mark.parametrize("fname", ["pre_w48.npz", "pre_cfg1.npz"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("parts", [2, 5])
def test_chain_vs_golden_and_one_shot(eng, golden_dir, fname, mode, parts):
    d = dict(np.load(os.path.join(golden_dir, fname)))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    W, n1, _ = kn.shape
    rng = np.random.default_rng(100 * parts + 10 * mode[0] + mode[1] + 3 * mode[2])
    cuts = _random_cuts(rng, W, n1 - 1, parts)
    for want, lanes in [(("mean", "jac", "cov"), 0), (("mean",), 0), (("mean",), 2), (("mean",), 5), (("mean",), 16), (("mean",), 64),
                        (("mean", "jac"), 2), (("mean", "jac"), 4), (("mean", "jac"), 64)]:
        prm = eng.make_params(*mode, lanes_per_window=lanes)
        out, _ = _chain(eng, prm, kn, lin, q, cuts, want)
        label = "%s %s parts=%d want=%s L=%d" % (fname, mode, parts, want, lanes)
        check_pre(out, _mode_out(d, mode), what=_what(want), v2=(mode[0] == 2), label=label, regression=True)
        one = _host(eng.preintegrate(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=want))
        check_pre(out, one, what=_what(want), v2=(mode[0] == 2), label=label + " vs one-shot", regression=True)


@pytest.mark.parametrize("split", [0, 1, 17, 49, 50])
@pytest.mark.parametrize("mode", MODES)
def test_split_points_vs_golden(eng, golden_dir, split, mode):
    d = dict(np.load(os.path.join(golden_dir, "pre_w48.npz")))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    W = kn.shape[0]
    cuts = np.stack([np.zeros(W, np.int64), np.full(W, split, np.int64), np.full(W, 50, np.int64)], axis=1)
    out, _ = _chain(eng, eng.make_params(*mode), kn, lin, q, cuts, ("mean", "jac", "cov"))
    check_pre(out, _mode_out(d, mode), v2=(mode[0] == 2), label="split %d %s" % (split, mode), regression=True)


@pytest.mark.parametrize("split", [0, 1, 17, 49, 50])
@pytest.mark.parametrize("mode,want,lanes", [((1, 0, 1), ("mean", "jac", "cov"), 0), ((1, 0, 1), ("mean", "jac"), 2),
                                             ((1, 0, 1), ("mean",), 64), ((2, 0, 1), ("mean", "jac", "cov"), 0),
                                             ((2, 0, 1), ("mean",), 2), ((2, 0, 1), ("mean",), 64)])
def test_split_state_vs_trace(eng, golden_dir, split, mode, want, lanes):
    """The FIRST call's outputs against the trace snapshot at the split, the second's against the final state."""
    model = mode[0]
    d = dict(np.load(os.path.join(golden_dir, "trace_v%d.npz" % model)))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    prm = eng.make_params(*mode, lanes_per_window=lanes)
    what = _what(want)
    a, carry = eng.preintegrate_resume(_dev(kn[None, :split + 1], eng), _dev(lin[None], eng), _dev(q[None], eng), prm, want=want)
    a = _host(a)
    if split == 0:
        ref = {k: np.zeros((1,) + d[k].shape[1:]) for k in ("DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b", "P")}
        ref["q"][0, 3] = 1.0
    else:
        ref = {k: d[k][split - 1:split] for k in d if k not in ("knots", "lin", "q_k_lin")}
    check_pre(a, ref, what=what, v2=(model == 2), label="split %d %s first call" % (split, mode), regression=True)
    b, _ = eng.preintegrate_resume(_dev(kn[None, split:], eng), _dev(lin[None], eng), _dev(q[None], eng), prm, want=want,
                                   carry_in=carry)
    ref = {k: d[k][-1:] for k in d if k not in ("knots", "lin", "q_k_lin")}
    check_pre(_host(b), ref, what=what, v2=(model == 2), label="split %d %s final" % (split, mode), regression=True)


@pytest.mark.parametrize("model", [1, 2])
def test_null_carry_is_the_batch_call_at_big_kernel_shapes(eng, model):
    """Dense mean-only batches of >= 700 k windows x >= 16 intervals run the batch entry's BIG kernel; the resume entry runs
    the plain one.  Same per-interval arithmetic: the outputs must still be identical."""
    from cpi_amd import synth
    W, N = 700_000, 16
    kn, lin, q = synth.make_windows(W, N, seed=808 + model, device=eng.device)
    prm = eng.make_params(model)
    a = _host(eng.preintegrate(kn, lin, q, prm, want=("mean",)))
    b, _ = eng.preintegrate_resume(kn, lin, q, prm, want=("mean",))
    b = _host(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (model, k)


# --------------------------------------------------------------------------- 3. the incremental facades against the trace
def _trace_check(row, d, i, model, label):
    ref = {k: d[k][i:i + 1] for k in ("DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b", "P")}
    check_pre(row, ref, v2=(model == 2), label="%s read %d" % (label, i), regression=True)


@pytest.mark.parametrize("model", [1, 2])
def test_python_mirror_incremental_vs_trace(eng, golden_dir, model):
    import cpi_amd
    d = dict(np.load(os.path.join(golden_dir, "trace_v%d.npz" % model)))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    cls = cpi_amd.CpiV1 if model == 1 else cpi_amd.CpiV2
    cpi = cls(0.005, 4e-6, 0.01, 2e-4, engine=eng)
    cpi.set_incremental(True)
    cpi.setLinearizationPoints(lin[:3], lin[3:], q, (0.0, 0.0, 9.8))
    for i in range(kn.shape[0] - 1):
        a, b = kn[i], kn[i + 1]
        cpi.feed_IMU(a[0], b[0], a[1:4], a[4:7], b[1:4], b[4:7])
        row = {"DT": np.array([cpi.DT]), "alpha": cpi.alpha_tau[None], "beta": cpi.beta_tau[None], "q": cpi.q_k2tau[None],
               "P": cpi.P_meas.T.reshape(1, 225)}
        for k in ("J_q", "J_a", "J_b", "H_a", "H_b") + (("O_a", "O_b") if model == 2 else ()):
            row[k] = getattr(cpi, k).T.reshape(1, 9)
        _trace_check(row, d, i, model, "mirror m%d" % model)
        assert len(cpi._iv) == 0 and cpi._tail is not None, "only the last knot is kept after a read"
    with pytest.raises(RuntimeError):
        cpi.setLinearizationPoints(lin[:3], lin[3:], q, (0.0, 0.0, 9.8))
    with pytest.raises(ValueError):
        cpi_amd.ForsterDiscrete(0.005, 4e-6, 0.01, 2e-4, engine=eng).set_incremental(True)
    # a read before the first feed_IMU integrates nothing: the linearisation point may still be set
    fresh = cls(0.005, 4e-6, 0.01, 2e-4, engine=eng)
    fresh.set_incremental(True)
    assert fresh.DT == 0.0
    fresh.setLinearizationPoints(lin[:3], lin[3:], q, (0.0, 0.0, 9.8))


@pytest.fixture(scope="module")
def inc_exe():
    from cpi_amd import _lib
    _lib.load()
    out = os.path.join(tempfile.mkdtemp(), "test_incremental")
    libdir = os.path.join(ROOT, "cpi_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_incremental.cpp"), "-o", out,
                           "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("model", [1, 2])
def test_cpp_facade_incremental_vs_trace(inc_exe, golden_dir, model):
    d = dict(np.load(os.path.join(golden_dir, "trace_v%d.npz" % model)))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        np.array([kn.shape[0]], dtype=np.float64).tofile(f)
        kn.tofile(f); lin.tofile(f); q.tofile(f)
        path = f.name
    p = subprocess.run([inc_exe, path, str(model)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-400:] + p.stderr
    lines = p.stdout.strip().split("\n")
    reads = [ln for ln in lines if ln.startswith("READ ")]
    assert len(reads) == kn.shape[0] - 1

    def parse(ln):
        v = np.array([float(x) for x in ln.split()[1:]])
        row, o = {"DT": v[0:1], "alpha": v[1:4][None], "beta": v[4:7][None], "q": v[7:11][None]}, 11
        for k in ("J_q", "J_a", "J_b", "H_a", "H_b") + (("O_a", "O_b") if model == 2 else ()):
            row[k] = v[o:o + 9][None]
            o += 9
        row["P"] = v[o:o + 225][None]
        assert o + 225 == v.size
        return row

    for i, ln in enumerate(reads):
        _trace_check(parse(ln), d, i, model, "C++ facade m%d" % model)
    copy = [ln for ln in lines if ln.startswith("COPY ")]
    assert len(copy) == 1
    _trace_check(parse(copy[0]), d, kn.shape[0] - 2, model, "C++ facade copy m%d" % model)
    assert "GUARDS 1 1 1" in lines


# --------------------------------------------------------------------------- 4. guards
def test_tag_mismatch_poisons_exactly_those_windows(eng):
    from cpi_amd import synth
    W, N = 70, 20
    kn, lin, q = synth.make_windows(W, N, seed=77)
    kn, lin, q = _dev(kn.numpy(), eng), _dev(lin.numpy(), eng), _dev(q.numpy(), eng)
    for model in (1, 2):
        prm = eng.make_params(model)
        _, full = eng.preintegrate_resume(kn, lin, q, prm, want=("mean", "jac", "cov"))
        _, means = eng.preintegrate_resume(kn, lin, q, prm, want=("mean",))
        _, other = eng.preintegrate_resume(kn, lin, q, eng.make_params(model, imu_avg=True), want=("mean", "jac", "cov"))
        mixed = full.clone()
        bad = np.zeros(W, bool)
        bad[1::3] = True                     # a means-only record resumed with P / Jacobians requested
        bad[2::7] = True                     # imu_avg differs
        bad[5] = True                        # tag 0
        idx = torch.from_numpy(np.arange(1, W, 3)).to(eng.device)
        mixed[idx] = means[idx]
        idx2 = torch.from_numpy(np.arange(2, W, 7)).to(eng.device)
        mixed[idx2] = other[idx2]
        mixed[5, 0] = 0.0
        out, carry = eng.preintegrate_resume(kn, lin, q, prm, want=("mean", "jac", "cov"), carry_in=mixed)
        out = _host(out)
        c = carry.cpu().numpy()
        for k, v in out.items():
            v = v.reshape(W, -1)
            assert np.all(np.isnan(v[bad])), (model, k)
            assert np.all(np.isfinite(v[~bad])), (model, k)
        assert np.all(np.isnan(c[bad, 0])) and np.all(np.isfinite(c[~bad, :17]))
        # a means-only continuation of a full record is fine: it needs the means only
        out, _ = eng.preintegrate_resume(kn, lin, q, prm, want=("mean",), carry_in=full)
        assert all(np.all(np.isfinite(v)) for v in _host(out).values())


def test_invalid_calls(eng):
    import cpi_amd
    from cpi_amd import synth
    kn, lin, q = synth.make_windows(8, 10, seed=3, device=eng.device)
    prm = eng.make_params(1)
    cd = eng.carry_doubles(1)
    assert (eng.carry_doubles(1), eng.carry_doubles(2), eng.carry_doubles(3), eng.carry_doubles(0)) == (288, 566, 0, 0)
    buf = torch.zeros((20, cd), dtype=torch.float64, device=eng.device)
    with pytest.raises(cpi_amd.CpiError) as e:
        eng.preintegrate_resume(kn, lin, q, prm, carry_in=buf[:8], carry_out=buf[4:12])
    assert e.value.code == 1
    with pytest.raises(cpi_amd.CpiError) as e:
        eng.preintegrate_resume(kn, lin, q, eng.make_params(3), carry_out=buf[:8])
    assert e.value.code == 1
    o = eng._outputs_struct(eng.alloc_outputs(8, ("mean",), 1))
    rc = eng.lib.cpi_preintegrate_resume(eng.ctx, C.byref(prm), 8, 10, C.c_void_p(kn.data_ptr()), None, None,
                                         C.c_void_p(lin.data_ptr()), C.c_void_p(q.data_ptr()), None, None, C.byref(o))
    assert rc == 1


# --------------------------------------------------------------------------- 5. full size: 100 k x 50 as 25 + 25
@pytest.mark.parametrize("model", [1, 2])
def test_full_size_two_call_chain(eng, model):
    from cpi_amd import synth
    W, N = 100_000, 50
    kn, lin, q = synth.make_windows(W, N, seed=404 + model, device=eng.device)
    prm = eng.make_params(model)
    one = _host(eng.preintegrate(kn, lin, q, prm))
    a, carry = eng.preintegrate_resume(kn[:, :26].contiguous(), lin, q, prm)
    b, _ = eng.preintegrate_resume(kn[:, 25:].contiguous(), lin, q, prm, carry_in=carry)
    check_pre(_host(b), one, v2=(model == 2), label="100k x 50 as 25 + 25, model %d" % model, regression=True)
