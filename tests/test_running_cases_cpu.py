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
