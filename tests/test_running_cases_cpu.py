"""CPU: the inputs of tests/running_cases.py still are what tests/test_gpu_running_edges.py needs them to be -- a change to
cpi_amd.synth or to the covariance kernel's pass length must not quietly empty those tests of their purpose.  If a seed stops
meeting a condition, choose another one; the conditions stay."""
import os
import re

import numpy as np
import pytest

from cpi_amd import stream as st
from oracle import oracle_py as op
from tests import running_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]
NAMES = ("DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a", "H_b", "P")


def test_cov_running_pass_lengths():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_cov_kernels.hpp")).read()
    m = re.search(r"constexpr int CH = \(MODEL == 1\) \? (\d+) : (\d+);", src)
    assert m and {1: int(m.group(1)), 2: int(m.group(2))} == rc.PASS, \
        "the pass lengths of cov_body changed: derive EDGE_N, the cut tables and STREAM_CASES of tests/running_cases.py again"
    m = re.search(r"#define CPI_RUN_T (\d+)", open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_running_kernels.hpp")).read()
                  + open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_running_body.inc")).read())
    assert m and int(m.group(1)) == rc.ROW_GROUP, "the row group of the running mean kernel changed: derive EDGE_N again"
    for C in rc.PASS.values():
        assert {C - 1, C, C + 1, 2 * C, 2 * C + 1} <= set(rc.EDGE_N)
    assert {rc.ROW_GROUP - 1, rc.ROW_GROUP, rc.ROW_GROUP + 1} <= set(rc.EDGE_N) and 70 in rc.EDGE_N


def test_tumbling_windows_reach_what_they_are_for():
    kn, lin, q = rc.tumbling_windows()
    W, N = kn.shape[0], kn.shape[1] - 1
    a = rc.wdt(kn, lin)
    print("tumbling windows: max |w| dt %.4f, %d of %d intervals above 0.25, %d above 1.0; windows reaching those bands: %d, %d"
          % (a.max(), (a > 0.25).sum(), a.size, (a > 1.0).sum(), (a > 0.25).any(axis=1).sum(), (a > 1.0).any(axis=1).sum()))
    assert a.max() < 1.3                                    # the stability region of the covariance's RK4
    assert (a > 0.25).mean() >= 0.40 and (a > 1.0).sum() >= 10
    # one wavefront holds lanes on the short polynomial, the wide one and the reduced path at once
    assert 0 < (a > 0.25).any(axis=1).sum() < W and 0 < (a > 1.0).any(axis=1).sum() < W
    for model, avg in MODES:
        prm = op.make_params(model, avg, 1)
        qs = []
        for w in range(W):
            tr = op.oracle().trace(prm, kn[w], lin[w], q[w])
            assert all(np.isfinite(tr[k]).all() for k in NAMES), (model, avg, w)
            qs.append(tr["q"])
        largest = np.bincount(np.abs(np.concatenate(qs)).argmax(axis=1), minlength=4)
        print("model %d imu_avg %d: largest quaternion component x / y / z / w in %s rows" % (model, avg, " / ".join(map(str, largest))))
        assert largest.sum() == W * N and largest.min() >= 0.05 * W * N, (model, avg, largest)     # every branch of rot_2_quat


@pytest.mark.parametrize("n,phase", rc.STREAM_CASES)
def test_tumbling_streams_put_the_tail_where_they_should(n, phase):
    s, u, lin, q = rc.tumbling_stream(n, phase)
    knots, first, count = st.assemble_windows(s, u)
    U = len(u)
    # n whole intervals, + the tail with a phase: the tail is interval n, slot 0 of a pass where n is a multiple of its length
    assert U == 20 and np.array_equal(count, np.full(U, n + (1 if phase > 0 else 0))), count
    wins = [knots[first[w]:first[w] + count[w] + 1] for w in range(U)]
    worst = max(float(rc.wdt(k[None], lin[w:w + 1]).max()) for w, k in enumerate(wins))
    print("tumbling stream n %d phase %g: max |w| dt %.4f" % (n, phase, worst))
    assert worst < 1.3
    for model, avg in MODES:
        prm = op.make_params(model, avg, 1)
        for w in range(U):
            tr = op.oracle().trace(prm, wins[w], lin[w], q[w])
            assert all(np.isfinite(tr[k]).all() for k in NAMES), (model, avg, w)


# ---- the inputs of tests/test_gpu_stj_edges.py and of the tumbling cases of tests/test_hostsim_stj.py
JAC7 = ("J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b")


def _stj_inputs():
    """name -> dense windows (kn, lin, q) and the counts the GPU tests cut them at (None: whole windows)."""
    from tests.test_gpu_query import _case, _layout
    from tests.test_gpu_running import _ragged_layout
    out = {}
    for N in rc.STJ_EDGE_N:
        kn, lin, q = rc.stj_edge_windows(N)
        out["edge N%d" % N] = (kn, lin, q, None if N == 47 else _ragged_layout(kn, rc.STJ_LAYOUT_SEED, garbage=True)[2])
    out["dense N47 cut as the ragged layout"] = rc.stj_edge_windows(47) + (_ragged_layout(rc.stj_edge_windows(47)[0], rc.STJ_LAYOUT_SEED, garbage=True)[2],)
    out["chains"] = rc.stj_chain_windows() + (None,)
    for model in (1, 2):
        out["open m%d" % model] = rc.stj_open_windows(model) + (None,)
    for case in ("tumbling", "reduced"):
        kn, lin, q, _ = _case(case)
        out["query %s dense" % case] = (kn, lin, q, None)
        out["query %s ragged" % case] = (kn, lin, q, _layout(case, "ragged")[3])
    return out


@pytest.mark.parametrize("avg", [0, 1])
def test_stj_tumbling_inputs_reach_what_they_are_for(avg):
    """Every tumbling input of the model-2 Jacobian tests: |w| dt inside the stability region of the covariance's RK4, intervals on
    the short polynomial, the long one and the reduced path of sincos_fast, a finite oracle trace in all seven Jacobian fields (and
    the means and P) over every interval the tests integrate -- so that no row and no query has to be left out -- and every branch of
    rot_2_quat among the oracle's q rows (per input from one pass length on; a window of one or two intervals cannot turn far
    enough, there the branches are reached by the set of edge lengths as a whole)."""
    prm = op.make_params(2, avg, 1)
    union = np.zeros(4, dtype=np.int64)
    for name, (kn, lin, q, count) in _stj_inputs().items():
        W, N = kn.shape[0], kn.shape[1] - 1
        a = rc.wdt(kn, lin)
        if count is not None:                                   # the intervals past a window's count are not integrated
            a = np.where(np.arange(N)[None, :] < np.asarray(count)[:, None], a, 0.0)
        reg = rc.sincos_regimes(a)
        assert a.max() < 1.3, (name, a.max())
        # case "tumbling" of tests/test_gpu_query.py stays on the two polynomials; the reduced path of the queries is case "reduced"
        assert min(reg[:2] if name.startswith("query tumbling") else reg) > 0 and sum(reg) == a.size, (name, reg)
        # a wavefront mixes the regimes: windows that never leave the short polynomial beside windows on the wide path
        assert 0 < (a > 0.25).any(axis=1).sum() < W, name
        qs = []
        for w in range(W):
            n = N if count is None else int(count[w])
            if n == 0:
                continue
            tr = op.oracle().trace(prm, kn[w, :n + 1], lin[w], q[w])
            assert all(np.isfinite(tr[k]).all() for k in NAMES + JAC7[5:]), (name, avg, w)
            qs.append(tr["q"])
        largest = np.bincount(np.abs(np.concatenate(qs)).argmax(axis=1), minlength=4)
        print("%s imu_avg %d: max |w| dt %.4f, intervals short / long / reduced %s, largest quaternion component x / y / z / w in %s rows"
              % (name, avg, a.max(), reg, " / ".join(map(str, largest))))
        if name.startswith("edge"):
            union += largest
        if N >= rc.PASS[2]:
            assert largest.min() >= 1, (name, avg, largest)
    assert union.min() >= 1, union


@pytest.mark.parametrize("avg", [0, 1])
@pytest.mark.parametrize("n,phase", [(23, 0.37), (46, 0.37)])
def test_stj_tumbling_streams_have_finite_jacobian_traces(n, phase, avg):
    """The stream cases of the model-2 Jacobian rows: a finite trace in all seven fields and |w| dt inside the stability region.  The
    streams are there for the tail interval that opens a pass; the wide path of sincos_fast is the windows' part (the rates of
    tumbling_stream stay on the short polynomial once the bias is taken off)."""
    s, u, lin, q = rc.tumbling_stream(n, phase)
    knots, first, count = st.assemble_windows(s, u)
    prm = op.make_params(2, avg, 1)
    reg = np.zeros(3, dtype=np.int64)
    for w in range(len(u)):
        k = knots[first[w]:first[w] + count[w] + 1]
        a = rc.wdt(k[None], lin[w:w + 1])
        assert a.max() < 1.3
        reg += rc.sincos_regimes(a)
        tr = op.oracle().trace(prm, k, lin[w], q[w])
        assert all(np.isfinite(tr[f]).all() for f in NAMES + JAC7[5:]), (n, avg, w)
    print("tumbling stream n %d phase %g: intervals short / long / reduced %s" % (n, phase, tuple(int(r) for r in reg)))
    assert reg.sum() == int(count.sum()) and np.all(count == n + 1)
