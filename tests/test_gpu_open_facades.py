"""GPU: at(times) of the incremental preintegrators -- Python (cpi_amd.CpiV1 / CpiV2) and C++ (cpi_host::CpiBase::at,
tests/cpp/test_open_at.cpp) -- across several reads: the bits of Engine.query_open on the same chunks, and the oracle on the cut
window at tests/tol.py's TOL_*."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import synth
from oracle import oracle_py as op
from tests.test_gpu_stj import JAC7, MEAN, _bits, _dev, _np
from tests.tol import check_pre

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = (0.005, 4e-6, 0.01, 2e-4)
GRAV = (0.0, 0.0, 9.8)
N = 12
READS = (3, 5, 4)


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _window():
    kn, lin, q = (t.numpy()[0] for t in synth.make_windows(1, N, seed=515, edge_cases=False))
    return kn, lin, q


def _chunk_times(kn, a, b):
    t = kn[:, 0]
    return np.array([t[a] - 1e-3, t[a]] + [t[i] + 0.4 * (t[i + 1] - t[i]) for i in range(a, b)] + [t[b]])


def _cut_reference(model, kn, lin, q, times):
    t = kn[:, 0]
    idx = np.clip(np.searchsorted(t, times, side="right") - 1, 0, N)
    win = np.zeros((len(times), N + 2, 7))
    for k, (tq, i) in enumerate(zip(times, idx)):
        win[k, :i + 1] = kn[:i + 1]
        win[k, i + 1:] = kn[i]
        win[k, i + 1:, 0] = min(max(tq, t[0]), t[N])
    return op.oracle().run(op.make_params(model, 0, 1), win, np.repeat(lin[None], len(times), 0), np.repeat(q[None], len(times), 0))


@pytest.mark.parametrize("model", [1, 2])
def test_python_at_across_three_reads(eng, model):
    import cpi_amd
    kn, lin, q = _window()
    cls = cpi_amd.CpiV1 if model == 1 else cpi_amd.CpiV2
    cpi = cls(*SIG, engine=eng)
    cpi.set_incremental(True)
    cpi.setLinearizationPoints(lin[:3], lin[3:], q, GRAV)
    assert cpi.at([]) == []
    prm = eng.make_params(model, False, True, SIG, GRAV)
    d_lin, d_q = _dev(lin[None], eng), _dev(q[None], eng)
    fields = MEAN + (JAC7 if model == 2 else JAC7[:5]) + ("P",)
    zero = torch.zeros(1, dtype=torch.int32, device=eng.device)
    carry, a = None, 0
    for size in READS:
        b = a + size
        for i in range(a, b):
            cpi.feed_IMU(kn[i, 0], kn[i + 1, 0], kn[i, 1:4], kn[i, 4:7])
        times = _chunk_times(kn, a, b)
        got = cpi.at(times)
        assert len(got) == len(times) and set(got[0]) == set(fields)
        # the same chunk through the engine: the facade's knots hold this interval's reading at its opening knot
        seg = kn[a:b + 1].copy()
        if a:
            seg[0] = kn[a]
        seg[-1, 1:] = 0.0                        # (imu_avg off: the closing reading of the last fed interval was not given)
        d_seg = _dev(seg[None], eng)
        base, _ = eng.preintegrate_running_resume_stj(d_seg[:, :1].repeat(1, 2, 1).contiguous(), d_lin, d_q, prm, count=zero, carry_in=carry)
        rows, carry = eng.preintegrate_running_resume_stj(d_seg, d_lin, d_q, prm, carry_in=carry)
        want = _np(eng.query_open(d_seg, d_lin, rows, torch.zeros(len(times), dtype=torch.int32, device=eng.device), _dev(times, eng), base, q_k_lin=d_q,
                                  params=prm, want=("mean", "jac", "cov")))
        for k in fields:
            assert _bits(np.stack([g[k] for g in got]), want[k]), (a, k)
        # (a time before the chunk gives the state at the previous read: the reference is taken at the chunk's first stamp)
        ref = _cut_reference(model, kn, lin, q, np.maximum(times, kn[a, 0]))
        check_pre({k: np.stack([g[k] for g in got]) for k in fields}, {k: ref[k] for k in fields}, what=("mean", "jac", "cov"), v2=model == 2,
                  label="at() model %d read at %d" % (model, a))
        # the members then stand at the chunk's end
        assert _bits(np.asarray(cpi.alpha_tau), got[-1]["alpha"]) and _bits(cpi.P_meas.T.reshape(-1), got[-1]["P"])
        a = b
    # nothing pending: every time gives the current state
    again = cpi.at([kn[0, 0], kn[N, 0] + 1.0])
    for k in fields:
        assert _bits(again[0][k], got[-1][k]) and _bits(again[1][k], got[-1][k]), k


def test_cpp_at(eng):
    """tests/cpp/test_open_at.cpp: CpiBase::at over reads of 3, 5, 4 ... intervals; the program checks the states before and after each
    chunk against its members bit for bit, the lines it prints are compared with the oracle on the cut window."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    kn, lin, q = _window()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_open_at")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_open_at.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        path = os.path.join(tmp, "win.bin")
        np.concatenate([[float(N + 1)], kn.reshape(-1), lin, q]).astype(np.float64).tofile(path)
        for model in (1, 2):
            p = subprocess.run([exe, path, str(model)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
            assert p.returncode == 0, (p.returncode, p.stderr)
            lines = p.stdout.splitlines()
            assert lines[-1] == "test_open_at ok"
            vals = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("AT ")])
            assert len(vals) == sum(s + 3 for s in READS)
            fields = MEAN + (JAC7 if model == 2 else JAC7[:5]) + ("P",)
            sizes = dict(op.OUT_FIELDS)
            got, at = {}, 1
            for k in fields:
                got[k] = vals[:, at:at + sizes[k]] if sizes[k] > 1 else vals[:, at]
                at += sizes[k]
            assert at == vals.shape[1]
            # a time before its chunk gives the state at the previous read: the reference is taken at the chunk's first stamp
            starts = np.concatenate([np.full(size + 3, kn[a, 0]) for a, size in zip(np.cumsum((0,) + READS[:-1]), READS)])
            ref = _cut_reference(model, kn, lin, q, np.maximum(vals[:, 0], starts))
            check_pre(got, {k: ref[k] for k in fields}, what=("mean", "jac", "cov"), v2=model == 2, label="CpiBase::at model %d" % model)
