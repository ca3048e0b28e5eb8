"""CPU: the inputs of tests/mean_cases.py still are what tests/test_gpu_mean_edges.py needs them to be, and the lane algorithm of
the mean kernels (tests/hostsim_py.mean: cpi_math.hpp compiled for the host, driven lane by lane) holds the oracle at per-field
gates on those inputs at every lane count.  If a seed stops meeting a condition, choose another one; the conditions stay."""
import os
import re

import numpy as np
import pytest

from oracle import oracle_py as op
from tests import hostsim_py as hs
from tests import mean_cases as mc
from tests import running_cases as rc
from tests.test_gpu_running import _ragged_layout
from tests.tol import FieldTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpi_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_mean_kernel_constants_behind_the_edge_lengths():
    again = ": derive MEAN_EDGE_N and the table above it in tests/mean_cases.py again"
    m = re.search(r"static const int kMeanLanes\[\] = \{([0-9, ]+)\};", _src("cpi_mean.hip"))
    assert m and [int(v) for v in m.group(1).split(",")] == mc.MEAN_LANES, "kMeanLanes changed" + again
    hdr = _src("cpi_mean_kernels.hpp")
    m, b = re.search(r"#define CPI_MEAN_C (\d+)", hdr), re.search(r"#define CPI_MEAN_BIG_C (\d+)", hdr)
    assert m and int(m.group(1)) == mc.CHUNK, "CPI_MEAN_C changed" + again
    assert b and int(b.group(1)) == mc.CHUNK_BIG, "CPI_MEAN_BIG_C changed: derive the BIG shapes of tests/test_gpu_mean_edges.py again"
    m = re.search(r"constexpr int C = BIG \? CPI_MEAN_BIG_C : \(\(L <= (\d+) && !JAC\) \? CPI_MEAN_C : 1\);", _src("cpi_mean_body.inc"))
    assert m and int(m.group(1)) == mc.CHUNK_LANES, "the rule that picks the knots per chunk changed" + again
    # what the table of MEAN_EDGE_N says of each length, from the constants
    per = lambda N, L: -(-N // L)
    used = lambda N, L: -(-N // per(N, L))
    assert mc.MEAN_EDGE_N == [1, 5, 13, 47, 65] and mc.CHUNK == 2
    assert per(5, 1) % mc.CHUNK == 1 and per(5, 5) == 1 and used(5, 6) == 5
    assert per(13, 2) == 7 and used(13, 12) == 7 and used(13, 16) == 13
    assert 47 < 64 and used(47, 32) == 24
    assert per(65, 64) == 2 and used(65, 64) == 33
    assert any(L <= mc.CHUNK_LANES for L in mc.MEAN_LANES) and any(L > mc.CHUNK_LANES for L in mc.MEAN_LANES)
    assert 17 >= int(re.search(r"#define CPI_MEAN_BIG_NMIN (\d+)", _src("cpi_mean.hip")).group(1)) and 17 % mc.CHUNK_BIG != 0


def test_dense_sets_reach_what_they_are_for():
    """Every dense set holds intervals on the short polynomial, the long one and the reduced path and stays below |w| dt = 1.3; a
    wavefront mixes windows on the short polynomial with windows off it; the ragged counts hold 0, 1, N - 1, N and a value above
    N; over the sets, the oracle's final quaternions reach every branch of rot_2_quat, for both models."""
    largest = {m: np.zeros(4, dtype=np.int64) for m in mc.MODES}
    for N in mc.MEAN_EDGE_N:
        kn, lin, q = mc.mean_edge_windows(N)
        assert kn.shape == (32, N + 1, 7)
        a = rc.wdt(kn, lin)
        reg = rc.sincos_regimes(a)
        assert a.max() < 1.3 and min(reg) > 0 and sum(reg) == a.size, (N, a.max(), reg)
        assert 0 < (a > 0.25).any(axis=1).sum() and (N == 1 or (a <= 0.25).any(axis=1).sum() > 0), N
        _, _, count, given = _ragged_layout(kn, mc.MEAN_LAYOUT_SEED, garbage=True)
        assert {0, 1, N - 1, N} <= set(int(c) for c in count) and (given > N).any() and np.array_equal(np.clip(given, 0, N), count), (N, given)
        print("dense N %d: max |w| dt %.4f, intervals short / long / reduced %s; ragged counts given: %s" % (N, a.max(), reg, given.tolist()))
        for model, avg in mc.MODES:
            for cnt, key in ((None, ("dense", N)), (count, ("ragged", N))):
                ref = mc.oracle_windows(model, avg, kn, lin, q, cnt, key=key)
                largest[(model, avg)] += np.bincount(np.abs(ref["q"]).argmax(axis=1), minlength=4)
    for mode, c in largest.items():
        print("model %d imu_avg %d: largest quaternion component x / y / z / w in %s final rotations" % (mode + (" / ".join(map(str, c)),)))
        assert c.min() >= 1, (mode, c)


@pytest.mark.parametrize("n,phase", mc.STREAM_CASES)
def test_stream_cases_reach_what_they_are_for(n, phase):
    """Both runs of every stream case: 20 windows of n whole intervals (+ the tail with a phase), all three regimes, below 1.3,
    a finite oracle in every mode; with a phase, tail intervals on the short polynomial and on the wide path."""
    for run in (0, 1):
        s, u, lin, q = mc.mean_stream(n, phase, run)
        knots, first, count, dense, N = mc.stream_windows(s, u)
        assert len(u) == mc.STREAM_WINDOWS and N == n + (1 if phase > 0 else 0) and np.all(count == N), count
        a = mc.masked_wdt(dense, lin, count)
        reg = rc.sincos_regimes(a)
        assert a.max() < 1.3 and min(reg) > 0, (n, phase, run, a.max(), reg)
        tails = a[:, N - 1] if phase > 0 else np.zeros(0)
        print("stream n %d phase %g run %d: max |w| dt %.4f, intervals short / long / reduced %s, tails on the wide path %d of %d"
              % (n, phase, run, a.max(), reg, (tails > 0.25).sum(), len(tails)))
        if phase > 0:
            assert (tails > 0.25).sum() >= 2 and (tails <= 0.25).sum() >= 2, tails
        # neighbouring windows in different regimes: the windows that reach the reduced path are neither none nor all
        assert 0 < (a > 1.0).any(axis=1).sum() < len(u) and 0 < (a > 0.25).any(axis=1).sum()
        for model, avg in mc.MODES:
            mc.oracle_windows(model, avg, dense, lin, q, count, key=("stream", n, phase, run))
    # the option keeps the existing callers' bits
    s0 = rc.tumbling_stream(n, phase)
    from cpi_amd import synth
    s1 = [t.numpy().copy() for t in synth.make_stream(20, n, seed=60 + n, phase=phase)]
    s1[0][:, 1:4] *= 25.0
    s1[2][:, 0:3] *= 25.0
    assert all(np.array_equal(x, y) for x, y in zip(s0, s1))


def test_big_cases_reach_what_they_are_for():
    """The shapes that the launcher admits to the three-knot kernel, and inputs on all three paths of sincos_fast."""
    src = _src("cpi_mean.hip")
    lim = {k: int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("CPI_MEAN_BIG_W", "CPI_MEAN_BIG_W_DENSE", "CPI_MEAN_BIG_W_M2", "CPI_MEAN_BIG_NMIN")}
    W, N, B = mc.BIG_DENSE
    U, n, phase = mc.BIG_STREAM
    assert W >= max(lim["CPI_MEAN_BIG_W_DENSE"], lim["CPI_MEAN_BIG_W_M2"]) and N >= lim["CPI_MEAN_BIG_NMIN"] and N % mc.CHUNK_BIG != 0, lim
    assert lim["CPI_MEAN_BIG_W"] <= U < lim["CPI_MEAN_BIG_W_M2"] and n + 1 >= lim["CPI_MEAN_BIG_NMIN"], lim
    assert all(B % p for p in range(2, B)) and W % B and W % 64
    kn, lin, q = mc.big_dense_base()
    a = rc.wdt(kn, lin)
    assert kn.shape == (B, N + 1, 7) and a.max() < 1.3 and min(rc.sincos_regimes(a)) > 0, (a.max(), rc.sincos_regimes(a))
    s, u, lin, q = mc.big_stream()
    assert len(u) == U and len(s) == U * n + 1
    a = np.linalg.norm(s[:-1, 1:4] - np.repeat(lin[:, 0:3], n, axis=0), axis=1) * np.diff(s[:, 0])
    reg = rc.sincos_regimes(a)
    print("big stream: max |w| dt %.4f, intervals short / long / reduced %s" % (a.max(), reg))
    assert a.max() < 1.3 and min(reg) > 0
    tails = a.reshape(U, n)[:, -1] * phase        # the tail holds the reading that closes the last whole interval; close enough to count
    assert (tails > 0.25).sum() > 64 and (tails <= 0.25).sum() > 64


@pytest.mark.parametrize("mode", mc.MODES)
def test_host_twin_at_every_lane_count(mode):
    """hostsim_py.mean on every dense set at every L of kMeanLanes, mean-only and (model 1) with the analytic Jacobians, against
    the oracle: the order-preserving composition tree (mean_combine; model 2 mean-only: mean_step_v2seg / grav_combine /
    grav_apply) with segment rotations past 90 degrees, N < L and empty trailing segments, where no GPU exists."""
    model, avg = mode
    total = FieldTable(mc.MEAN + (mc.JAC5 if model == 1 else ()))
    for N in mc.MEAN_EDGE_N:
        kn, lin, q = mc.mean_edge_windows(N)
        ref = mc.oracle_windows(model, avg, kn, lin, q, key=("dense", N))
        t = FieldTable(total.fields)
        for L in mc.MEAN_LANES:
            for jac in ((0, 1) if model == 1 else (0,)):
                got = op.split_out(hs.mean(model, jac, avg, L, kn, lin, q))
                if not jac:                                     # the Jacobians of a mean-only run are not computed
                    got = dict(got, **{k: ref[k] for k in mc.JAC5})
                for tab in (t, total):
                    tab.add(got, ref, "N%d L%d%s" % (N, L, " jac" if jac else ""))
        t.report("host twin, mean_edge_windows(%d), model %d imu_avg %d, every L, vs the oracle" % (N, model, avg), mc.TWIN_GATE)
    total.report("host twin, all dense sets, model %d imu_avg %d" % (model, avg), mc.TWIN_GATE)
    total.check(mc.TWIN_GATE, "host twin model %d imu_avg %d" % (model, avg))
