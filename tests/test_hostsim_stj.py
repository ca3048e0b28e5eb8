"""CPU: host emulation of model 2's running and query-time bias Jacobians (tests/hostsim/hostsim_stj.cpp: the nine Discrete_J_b
transition columns of cov_body, from cpi_math.hpp).

Two claims are checked without a GPU.  The per-interval read-out: every row of all seven fields against the C restatement's trace
(oracle_py.oracle().trace with state_transition_jacobians = 1, which returns O_a / O_b after every feed_IMU) at TOL_JAC, and
against the pinned trace of the compiled reference (tests/golden/trace_v2.npz) at REG_JAC for the fields it holds.  The
reconstruction cpi_query_stj_kernel relies on: the nine columns REBUILT from one row of Jacobians (theta rows of the b_a /
theta_klin columns zero, unit / zero bias rows, the clone rows equal to the theta rows), advanced by one partial interval with the
reading held, against the oracle on the cut window [knot 0 .. knot i, {t_q, w_i, a_i}] at TOL_JAC."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as op
from tests import running_cases as rc
from tests.tol import REG_JAC, TOL_JAC, FieldTable, check_pre, field_gates

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_stj.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_stj.so")
_HDR = os.path.join(os.path.dirname(_HERE), "cpi_amd", "csrc", "cpi_math.hpp")
GRAV = np.array([0.0, 0.0, 9.8])
JAC7 = ("J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b")
NS = (1, 2, 22, 23, 24, 47)        # on and beside the pass length of cov_body<2> (23)


def _gxx(src, out):
    """The emulation's build line."""
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src])


@pytest.fixture(scope="module")
def lib():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        _gxx(_SRC, _LIB)
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


# ------------------------------------------------------------------------------------------------ large rotations, per-field gates
# The tumbling windows of tests/running_cases.py (|w| dt up to ~1.16 rad per interval: the long polynomial and the Cody-Waite
# reduction of sincos_fast, every branch of rot_2_quat / quat_2_Rot, rotations carried past 90 degrees), every row and every
# query, one gate per field: 100 x the floor below, never looser than TOL_JAC.  A floor is the largest error of this emulation
# against the oracle measured on the CPU (x86-64, g++ -O2 -ffp-contract=off; both imu_avg settings; pytest -s prints the tables,
# profiles/stj_edges.md keeps them), never below 2^-53 x max |ref| of the field.
#   rows:    hss_rows on stj_edge_windows(N), N of STJ_EDGE_N, 32 windows each; every floor is set at N = 46 or 47 (J_q, J_b, H_a, H_b
#            and O_b by N = 47, J_a and O_a by N = 46), in one of the last seven rows of the window
#   queries: hss_query on tumbling_windows(32, 47) from the EMULATION's own row i - 1, i of {0, 1, CH - 1, CH, CH + 1, N - 1},
#            0.37 and 0.999 into the interval; every floor is set at i = N - 1
HOST_FLOOR_ROWS = {"J_q": 2.50e-16, "J_a": 1.91e-17, "J_b": 2.22e-16, "H_a": 4.16e-17, "H_b": 3.05e-16, "O_a": 3.33e-16, "O_b": 4.00e-15}
HOST_FLOOR_QUERY = {"J_q": 2.50e-16, "J_a": 1.39e-17, "J_b": 1.94e-16, "H_a": 3.82e-17, "H_b": 2.78e-16, "O_a": 2.78e-16, "O_b": 4.44e-15}
CH = rc.PASS[2]
_ref_cache = {}


def _ref_trace(key, avg, kn, lin, q):
    """oracle().trace of one window, kept for the mutation checks that run the same comparison again."""
    if (key, avg) not in _ref_cache:
        tr = op.oracle().trace(op.make_params(2, avg, 1), kn, lin, q)
        assert all(np.isfinite(tr[k]).all() for k in JAC7), key
        _ref_cache[(key, avg)] = {k: tr[k] for k in JAC7}
    return _ref_cache[(key, avg)]


def _rows_table(lib, cases, label):
    """FieldTable of hss_rows against the oracle's trace over every row of every window of the cases {name: (kn, lin, q)}."""
    t = FieldTable(JAC7)
    for name, (kn, lin, q) in cases.items():
        for avg in (0, 1):
            for w in range(kn.shape[0]):
                ref = _ref_trace((label, name, w), avg, kn[w], lin[w], q[w])
                got = op.split_out(stj_rows(lib, avg, kn[w], lin[w], q[w]))
                t.add(got, ref, "%s avg%d w%d" % (name, avg, w))
    return t


def _tumbling_cases():
    return {"N%d" % N: rc.stj_edge_windows(N) for N in rc.STJ_EDGE_N}


def _gentle_cases():
    """The windows of test_hostsim_stj_rows_match_the_oracle_trace at the two longest lengths."""
    from cpi_amd import synth
    return {"N%d" % N: tuple(t.numpy() for t in synth.make_windows(6, N, seed=300 + N)) for N in (24, 47)}


def _query_table(lib):
    """FieldTable of hss_query, the base row taken from hss_rows (so the rebuild from a COMPUTED row is under test), against the
    oracle on the cut window."""
    kn, lin, q = rc.tumbling_windows(32, 47)
    W, N = kn.shape[0], kn.shape[1] - 1
    t = FieldTable(JAC7)
    for avg in (0, 1):
        for w in range(W):
            rows = stj_rows(lib, avg, kn[w], lin[w], q[w])
            for i in (0, 1, CH - 1, CH, CH + 1, N - 1):
                for frac in (0.37, 0.999):
                    tq = kn[w, i, 0] + frac * (kn[w, i + 1, 0] - kn[w, i, 0])
                    cut = np.concatenate([kn[w, :i + 1], kn[w, i:i + 1]], axis=0).copy()
                    cut[-1, 0] = tq
                    ref = _ref_trace(("query", w, i, frac), avg, cut, lin[w], q[w])
                    got = stj_query(lib, avg, rows[i - 1] if i > 0 else None, kn[w, i], tq, lin[w], q[w])
                    t.add(got, {k: ref[k][-1:] for k in JAC7}, "avg%d w%d i%d +%g" % (avg, w, i, frac))
    return t


def test_hostsim_stj_rows_under_large_rotations(lib):
    t = _rows_table(lib, _tumbling_cases(), "tumbling")
    gates = field_gates(HOST_FLOOR_ROWS)
    t.report("hostsim stj rows vs oracle.trace, tumbling windows, N of %s, imu_avg 0 and 1" % rc.STJ_EDGE_N, gates)
    t.check(gates, "hostsim stj rows, tumbling")


def test_hostsim_stj_query_step_from_its_own_rows_under_large_rotations(lib):
    t = _query_table(lib)
    gates = field_gates(HOST_FLOOR_QUERY)
    t.report("hostsim stj query step from the emulation's own rows vs the oracle on the cut window, tumbling_windows(32, 47)", gates)
    t.check(gates, "hostsim stj query, tumbling")


# ---- mutation checks: the comparisons above must see a slip the old gate cannot see.  Nothing mutated leaves tmp_path.
_CSRC = os.path.dirname(_HDR)
MUTATIONS = {
    # (a) the x^15 term of the long sine polynomial
    "sin_x15_zero": ("cpi_amd/csrc/cpi_math.hpp", "CPI_HORNER(ps, z, -1.0 / 1307674368000.0);", "CPI_HORNER(ps, z, 0.0);"),
    # (b) the second part of pi/2 in the Cody-Waite reduction of sincos_wide
    "pio2_second_part_zero": ("cpi_amd/csrc/cpi_math.hpp", "r = fma(-k, 6.07710050650619224932e-11, r);", "r = fma(-k, 0.0, r);"),
    # (c) the query rebuild: the clone rows 15..17 not set from the theta rows
    "query_clone_rows_unset": ("tests/hostsim/hostsim_stj.cpp", "st3(P0 + 12, pp); st3(P0 + 15, th);", "st3(P0 + 12, pp);"),
}


def _mutant(tmp_path, name):
    rel, old, new = MUTATIONS[name]
    root = str(tmp_path / name)
    os.makedirs(os.path.join(root, "cpi_amd", "csrc"))
    os.makedirs(os.path.join(root, "tests", "hostsim"))
    for f in glob.glob(os.path.join(_CSRC, "*.hpp")) + glob.glob(os.path.join(_CSRC, "*.inc")):
        shutil.copy(f, os.path.join(root, "cpi_amd", "csrc"))
    shutil.copy(_SRC, os.path.join(root, "tests", "hostsim"))
    path = os.path.join(root, *rel.split("/"))
    text = open(path).read()
    assert text.count(old) == 1, "mutation %s: its pattern matches %d times in %s" % (name, text.count(old), rel)
    open(path, "w").write(text.replace(old, new))
    out = os.path.join(root, "libhostsim_stj_mutant.so")
    _gxx(os.path.join(root, "tests", "hostsim", "hostsim_stj.cpp"), out)
    return C.CDLL(out)


def _failing(t, gates):
    return [k for k in JAC7 if not t.err[k] <= gates[k]]


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutations_pass_the_old_gate_and_fail_the_per_field_gates(tmp_path, name):
    """(a) and (b) slip the wide path of sincos_fast: the gentle windows do not run it, and on the tumbling ones every field stays
    below TOL_JAC -- the old gate cannot see either -- while the per-field gates of the row comparison fail.  (c) breaks the query
    rebuild only: the rows pass their gates, the query step fails its own."""
    mut = _mutant(tmp_path, name)
    old = {k: TOL_JAC for k in JAC7}
    gentle = _rows_table(mut, _gentle_cases(), "gentle")
    rows = _rows_table(mut, _tumbling_cases(), "tumbling")
    query = _query_table(mut)
    g_rows, g_query = field_gates(HOST_FLOOR_ROWS), field_gates(HOST_FLOOR_QUERY)
    gentle.report("mutation %s: rows, gentle windows" % name, old)
    rows.report("mutation %s: rows, tumbling windows" % name, g_rows)
    query.report("mutation %s: query step, tumbling windows" % name, g_query)
    print("mutation %s: fields failing the per-field gates: rows %s, query step %s" % (name, _failing(rows, g_rows), _failing(query, g_query)))
    gentle.check(old, "mutation %s on the gentle windows at TOL_JAC" % name)
    if name == "query_clone_rows_unset":
        rows.check(g_rows, "mutation %s leaves the rows alone" % name)
        assert _failing(query, g_query), "the query-step gates do not see mutation %s" % name
    else:
        rows.check(old, "mutation %s on the tumbling windows at TOL_JAC" % name)
        assert _failing(rows, g_rows), "the per-field row gates do not see mutation %s" % name
