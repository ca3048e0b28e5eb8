"""CPU: host emulation of model 2's running and query-time bias Jacobians (tests/hostsim/hostsim_stj.cpp: the nine Discrete_J_b
transition columns of cov_body, from cpi_math.hpp).

Two claims are checked without a GPU.  The per-interval read-out: every row of all seven fields against the C restatement's trace
(oracle_py.oracle().trace with state_transition_jacobians = 1, which returns O_a / O_b after every feed_IMU) at TOL_JAC, and
against the pinned trace of the compiled reference (tests/golden/trace_v2.npz) at REG_JAC for the fields it holds.  The
reconstruction cpi_query_stj_kernel relies on: the nine columns REBUILT from one row of Jacobians (theta rows of the b_a /
theta_klin columns zero, unit / zero bias rows, the clone rows equal to the theta rows), advanced by one partial interval with the
reading held, against the oracle on the cut window [knot 0 .. knot i, {t_q, w_i, a_i}] at TOL_JAC."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as op
from tests.tol import REG_JAC, TOL_JAC, check_pre

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_stj.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_stj.so")
_HDR = os.path.join(os.path.dirname(_HERE), "cpi_amd", "csrc", "cpi_math.hpp")
GRAV = np.array([0.0, 0.0, 9.8])
JAC7 = ("J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b")
NS = (1, 2, 22, 23, 24, 47)        # on and beside the pass length of cov_body<2> (23)


@pytest.fixture(scope="module")
def lib():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-o", _LIB, _SRC])
    return C.CDLL(_LIB)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def stj_rows(lib, avg, kn, lin, q, N=None, n=None):
    kn = np.ascontiguousarray(kn, dtype=np.float64)
    n = kn.shape[0] - 1 if n is None else n
    N = n if N is None else N
    rows = np.full((N, 308), np.nan)
    lin, q = np.ascontiguousarray(lin), np.ascontiguousarray(q)
    assert lib.hss_rows(int(avg), N, n, _dp(kn), _dp(lin), _dp(q), _dp(GRAV), _dp(rows)) == 0
    return rows


def stj_query(lib, avg, row, knot, tq, lin, q):
    out = np.full(308, np.nan)
    row = None if row is None else np.ascontiguousarray(row)
    knot, lin, q = np.ascontiguousarray(knot), np.ascontiguousarray(lin), np.ascontiguousarray(q)
    lib.hss_query.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double] + [C.POINTER(C.c_double)] * 4
    assert lib.hss_query(int(avg), _dp(row), _dp(knot), float(tq), _dp(lin), _dp(q), _dp(GRAV), _dp(out)) == 0
    return op.split_out(out[None])


def _worst(worst, got, ref):
    for k in JAC7:
        worst[k] = max(worst.get(k, 0.0), float(np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max()))


def test_hostsim_stj_rows_match_the_golden_trace(lib, golden_dir):
    d = np.load(os.path.join(golden_dir, "trace_v2.npz"))
    got = op.split_out(stj_rows(lib, 0, d["knots"], d["lin"], d["q_k_lin"]))
    held = tuple(k for k in JAC7 if k in d.files)
    assert held, "the fixture holds no Jacobian field"
    for k in held:
        e = float(np.abs(got[k] - d[k]).max())
        print("golden trace_v2 %s err %.2e" % (k, e))
        assert e <= REG_JAC, (k, e)


@pytest.mark.parametrize("N", NS)
def test_hostsim_stj_rows_match_the_oracle_trace(lib, N):
    """The read-out after every interval, all seven fields, every row (seeded windows, edge cases included)."""
    from cpi_amd import synth
    W = 6
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=300 + N))
    worst = {}
    for avg in (0, 1):
        prm = op.make_params(2, avg, 1)
        for w in range(W):
            ref = op.oracle().trace(prm, kn[w], lin[w], q[w])
            assert all(np.isfinite(ref[k]).all() for k in JAC7)
            got = op.split_out(stj_rows(lib, avg, kn[w], lin[w], q[w]))
            check_pre(got, ref, what=("jac",), v2=True, label="stj rows avg%d N%d w%d" % (avg, N, w))
            _worst(worst, got, ref)
    print("hostsim stj rows vs oracle.trace, N = %d: %s" % (N, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


def test_hostsim_stj_rows_past_the_count_and_skipped_intervals_repeat(lib):
    from cpi_amd import synth
    N = 24
    kn, lin, q = (t.numpy()[0] for t in synth.make_windows(1, N, seed=11, edge_cases=False))
    for avg in (0, 1):
        for n in (0, 1, 23, 24):
            got = op.split_out(stj_rows(lib, avg, kn, lin, q, N=N, n=n))
            for k in JAC7:
                if n == 0:
                    assert not got[k][0].any(), (n, k)
                for i in range(max(n, 1), N):
                    assert np.array_equal(got[k][i], got[k][i - 1]), (n, i, k)
        k2 = kn.copy()
        i = N // 2
        k2[i + 1:, 0] -= k2[i + 1, 0] - k2[i, 0]          # dt == 0 at interval i
        got = op.split_out(stj_rows(lib, avg, k2, lin, q))
        for k in JAC7:
            assert np.array_equal(got[k][i], got[k][i - 1]), k


@pytest.mark.parametrize("N", (1, 23, 30))
def test_hostsim_stj_query_step_matches_the_oracle_on_the_cut_window(lib, N):
    """The reconstruction claim: nine columns rebuilt from a row of the ORACLE's trace (so that only the rebuild and the one
    partial interval are under test), one step with the reading held, against the oracle on [knot 0 .. knot i, {t_q, w_i, a_i}]."""
    from cpi_amd import synth
    W = 4
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=500 + N, edge_cases=False))
    worst = {}
    for avg in (0, 1):
        prm = op.make_params(2, avg, 1)
        for w in range(W):
            trace = op.oracle().trace(prm, kn[w], lin[w], q[w])
            for i in sorted({0, N // 2, N - 1}):
                for frac in (0.25, 0.9):
                    t_i, t_n = kn[w, i, 0], kn[w, i + 1, 0]
                    tq = t_i + frac * (t_n - t_i)
                    cut = np.concatenate([kn[w, :i + 1], kn[w, i:i + 1]], axis=0).copy()
                    cut[-1, 0] = tq
                    ref = op.oracle().trace(prm, cut, lin[w], q[w])
                    ref = {k: ref[k][-1:] for k in JAC7}
                    row = None
                    if i > 0:
                        row = np.zeros(308)
                        row[7:11] = trace["q"][i - 1]
                        for k, off in zip(JAC7, (20, 29, 38, 47, 56, 65, 74)):
                            row[off:off + 9] = trace[k][i - 1]
                    got = stj_query(lib, avg, row, kn[w, i], tq, lin[w], q[w])
                    check_pre(got, ref, what=("jac",), v2=True, label="stj query avg%d N%d w%d i%d" % (avg, N, w, i))
                    _worst(worst, got, ref)
    print("hostsim stj query vs oracle on the cut window, N = %d: %s" % (N, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
