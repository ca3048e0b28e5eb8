"""Inputs, references and gates for the tests of the mean kernels (cpi_mean_kernel, cpi_mean_carry_kernel, cpi_mean_runs_kernel,
cpi_mean_tiled_kernel) under large rotations: tests/test_mean_cases_cpu.py (the inputs stay honest, the host twin at every lane
count) and tests/test_gpu_mean_edges.py (every entry on an MI355X).  Stated once, here.

The dense sets are the tumbling windows of tests/running_cases.py (|w| dt up to ~1.16 rad per interval: every wavefront mixes
lanes on the short polynomial of sincos_fast, on the long one and on the Cody-Waite reduction, and the final rotations reach
every branch of rot_2_quat); the stream cases are tumbling_stream with a gyro scale that rises along the stream.

Floors and gates: a floor is the largest error of one field over one kind of comparison against the oracle
(oracle_py.oracle().run), never below 2^-53 x max |ref| of the field; the gate is 100 x the floor, never looser than TOL_MEAN /
TOL_JAC / TOL_COV (tests/tol.py: field_gates).  FLOOR holds the figures measured on an MI355X, TWIN_FLOOR those of the host
twin (tests/hostsim_py.mean) on the same dense sets; profiles/mean_edges.md holds the tables per case."""
import numpy as np

from cpi_amd import stream as st
from oracle import oracle_py as op
from tests import running_cases as rc
from tests.tol import field_gates

MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]
MEAN = ("DT", "alpha", "beta", "q")
JAC5 = ("J_q", "J_a", "J_b", "H_a", "H_b")
JAC7 = JAC5 + ("O_a", "O_b")

# cpi_mean.hip: kMeanLanes.  tests/test_mean_cases_cpu.py reads the list, CPI_MEAN_C, CPI_MEAN_BIG_C and the L <= 8 rule of
# cpi_mean_body.inc out of the sources: if one of them changes, the table below has to be derived again.
MEAN_LANES = [1, 2, 3, 4, 5, 6, 8, 12, 16, 32, 64]
CHUNK = 2                # CPI_MEAN_C: knots per chunk of the staged kernels with L <= 8, mean-only (1 otherwise)
CHUNK_BIG = 3            # CPI_MEAN_BIG_C
CHUNK_LANES = 8          # the largest L that stages CHUNK knots

# Window lengths, with per = ceil(N / L):
#    1   N < L for every L > 1
#    5   an odd per at L = 1 (the padded second step of a two-knot chunk is skipped); per = 1 at L = 5; one empty trailing
#        segment at L = 6
#   13   per = 7 at L = 2; seven segments and five empty lanes at L = 12; three empty lanes at L = 16
#   47   N < L at L = 64; 24 of 32 segments used at L = 32
#   65   33 segments of two intervals and 31 empty lanes at L = 64; staging of one knot per chunk (L >= 12, or any Jacobian
#        request) beside two knots per chunk
MEAN_EDGE_N = [1, 5, 13, 47, 65]
MEAN_EDGE_SEED = {1: rc.STJ_EDGE_SEED[1], 5: 944, 13: 961, 47: 901, 65: 978}
MEAN_LAYOUT_SEED = rc.STJ_LAYOUT_SEED


def mean_edge_windows(N):
    """32 tumbling windows of N intervals (N of MEAN_EDGE_N): kn [32, N + 1, 7], lin [32, 6], q [32, 4]."""
    return rc.tumbling_windows(32, N, seed=MEAN_EDGE_SEED[N])


# ---- streams: (n whole intervals, phase of the update grid); the scale of the gyro readings rises from RAMP[0] to RAMP[1] along
# the stream.  Two seeds per case: the first is the single stream, both together are the two runs of preintegrate_streams.  Chosen
# on the CPU (tests/test_mean_cases_cpu.py asserts it) so that every stream holds intervals on the short polynomial, on the long
# one and on the reduced path, stays below |w| dt = 1.3, and -- with a phase -- has tail intervals on the short polynomial in some
# windows and on the wide path in others.
STREAM_CASES = [(5, 0.37), (13, 0.0), (17, 0.37), (47, 0.37)]
STREAM_WINDOWS = 20
STREAM_RAMP = (4.0, 95.0)
STREAM_SEED = {(5, 0.37): (18, 22), (13, 0.0): (2, 10), (17, 0.37): (2, 10), (47, 0.37): (2, 10)}


def mean_stream(n, phase, run=0):
    """(stream [K, 7], update_times [20], lin [20, 6], q [20, 4]) of a stream case; run 1: the second run of the pair."""
    return rc.tumbling_stream(n, phase, seed=STREAM_SEED[(n, phase)][run], ramp=STREAM_RAMP, U=STREAM_WINDOWS)


# ---- the three-knot BIG instantiation: the launcher admits it from CPI_MEAN_BIG_W_DENSE = 700 000 dense windows (model 2:
# CPI_MEAN_BIG_W_M2 = 700 000 of either kind) or CPI_MEAN_BIG_W = 100 000 stream windows, from CPI_MEAN_BIG_NMIN = 16 intervals.
BIG_DENSE = (700_003, 17, 191)           # windows, intervals (five chunks of three knots and a padded one), base windows (a prime)
BIG_DENSE_SEED = 900
BIG_STREAM = (100_003, 16, 0.37)         # update times, whole intervals per window, phase
BIG_STREAM_SEED = 7


def big_dense_base():
    """The 191 tumbling windows of 17 intervals that the dense BIG batch repeats (window w of the batch is base window w % 191)."""
    return rc.tumbling_windows(BIG_DENSE[2], BIG_DENSE[1], seed=BIG_DENSE_SEED)


def big_stream():
    U, n, phase = BIG_STREAM
    return rc.tumbling_stream(n, phase, seed=BIG_STREAM_SEED, ramp=STREAM_RAMP, U=U)


def stream_windows(s, u):
    """The host-assembled windows of a stream (cpi_amd.stream.assemble_windows) and their dense copy for the oracle:
    (knots, first, count, dense [U, N + 1, 7], N)."""
    knots, first, count = st.assemble_windows(s, u)
    N = int(count.max())
    dense = np.zeros((len(u), N + 1, 7))
    for w in range(len(u)):
        c = int(count[w])
        dense[w, :c + 1] = knots[first[w]:first[w] + c + 1]
        dense[w, c + 1:] = dense[w, c]
    return knots, first, count, dense, N


def masked_wdt(kn, lin, count=None):
    """|w - b_w| dt of the intervals a window integrates (0 past its count)."""
    a = rc.wdt(kn, lin)
    if count is not None:
        a = np.where(np.arange(a.shape[1])[None, :] < np.asarray(count)[:, None], a, 0.0)
    return a


# ---- the reference: the oracle on every window, cut at its count
_ref_cache = {}


def oracle_windows(model, avg, kn, lin, q, count=None, key=None):
    """oracle_py.oracle().run on every window of kn [W, N + 1, 7], window w cut at count[w] (clamped into [0, N]; 0 intervals:
    the zero state).  key: cache the result under (key, model, avg) -- the tests share it and leave it unchanged."""
    if key is not None and (key, model, avg) in _ref_cache:
        return _ref_cache[(key, model, avg)]
    prm = op.make_params(model, avg, 1)
    W, N = kn.shape[0], kn.shape[1] - 1
    if count is None:
        ref = op.oracle().run(prm, kn, lin, q)
    else:
        c = np.clip(np.asarray(count), 0, N)
        raw = np.zeros((W, op.OUT_DOUBLES))
        for n in np.unique(c):
            sel = np.nonzero(c == n)[0]
            sub = np.zeros((len(sel), op.OUT_DOUBLES))
            op.oracle().run(prm, kn[sel, :n + 1], lin[sel], q[sel], raw=sub)
            raw[sel] = sub
        ref = op.split_out(raw)
    ref = {k: v for k, v in ref.items() if k != "R" and (model == 2 or k not in ("O_a", "O_b"))}
    assert all(np.isfinite(v).all() for v in ref.values()), (model, avg, key)
    for v in ref.values():
        v.flags.writeable = False
    if key is not None:
        _ref_cache[(key, model, avg)] = ref
    return ref


# ---- floors and gates
# The host twin (tests/hostsim_py.mean: cpi_math.hpp compiled for the host, driven lane by lane) against the oracle on the five
# dense sets, every mode and every L of MEAN_LANES; measured by tests/test_mean_cases_cpu.py, which prints the table.
# All of them on mean_edge_windows(65) but q: DT by its rounding, alpha model 2 L = 64, beta model 2 L = 6 and 8, J_q L = 6, J_a and
# J_b L = 12, H_a L = 64, H_b L = 32; q 8.88e-16 twice, model 1 imu_avg 0 on N = 65 at L = 12 and model 1 imu_avg 1 on
# mean_edge_windows(47) at L = 5 with Jacobians.
TWIN_FLOOR = {"DT": 3.61e-17, "alpha": 8.88e-16, "beta": 5.77e-15, "q": 8.88e-16,
              "J_q": 3.89e-16, "J_a": 6.25e-17, "J_b": 6.11e-16, "H_a": 4.16e-17, "H_b": 2.78e-16}
TWIN_GATE = field_gates(TWIN_FLOOR)

# Largest error against the oracle measured on an MI355X, never below 2^-53 x max |ref| of the field; P: cov_rel_err.  The case
# that sets each floor is named beside it.
FLOOR = {
    # Engine.preintegrate, every L and request, dense ("d") and ragged ("r") layouts of mean_edge_windows(N): all on d65 but P
    "batch": {"DT": 3.61e-17,                                   # its rounding
              "alpha": 8.88e-16, "beta": 7.99e-15,              # d65 model 2 imu_avg 0, mean-only, L = 64 and L = 6
              "q": 2.82e-15,                                    # d65 model 1 imu_avg 0, mean-only, L = 5
              "J_q": 3.47e-16, "J_b": 5.55e-16, "H_a": 5.55e-17, "H_b": 3.89e-16,      # d65 imu_avg 1, everything, L = 32, 64, 1, 2
              "J_a": 4.86e-17,                                  # d65 imu_avg 0, everything, L = 32
              "P": 2.68e-15},                                   # r47 model 1 imu_avg 0
    # Engine.preintegrate_resume, mean_edge_windows(N) cut once at c ("N/c"), first and second call
    "resume": {"DT": 3.61e-17,
               "alpha": 8.88e-16, "beta": 7.99e-15,             # 65/64 and 65/32, model 2 imu_avg 0, mean-only, second call, L = 0 and 3
               "q": 3.69e-15,                                   # 47/46 model 1 imu_avg 1, mean-only, first call, L = 0
               "J_q": 4.06e-16,                                 # 65/64 imu_avg 1, first call, L = 8
               "J_a": 5.55e-17, "J_b": 6.11e-16, "H_a": 5.55e-17,       # 65/1 imu_avg 0, second call, L = 64, 64, 0
               "H_b": 3.89e-16},                                # 65/64 imu_avg 1, second call, L = 1
    # preintegrate_stream / preintegrate_streams: all on mean_stream(47, 0.37), the two runs (P: the single stream)
    "stream": {"DT": 2.63e-17,
               "alpha": 5.00e-16, "beta": 5.11e-15,             # model 2, imu_avg 1 mean-only L = 1, imu_avg 0 means + Jacobians L = 64
               "q": 3.33e-15,                                   # model 1 imu_avg 1, means + Jacobians, L = 16
               "J_q": 1.94e-16, "J_a": 1.21e-17, "H_a": 2.43e-17, "H_b": 2.22e-16,     # imu_avg 1, L = 5, 64, 64, 1
               "J_b": 2.50e-16,                                 # imu_avg 0, L = 32
               "P": 2.46e-15},                                  # model 1 imu_avg 0
    # Engine.preintegrate_tiled, S wavefronts per tile, without counts
    "tiled": {"DT": 3.61e-17,
              "alpha": 8.88e-16,                                # N = 65 model 2 imu_avg 0, S = 2
              "beta": 7.55e-15,                                 # N = 47 model 2 imu_avg 0, S = 1
              "q": 2.84e-15},                                   # N = 65 model 1 imu_avg 0, S = 5
    # the three-knot instantiation: 700 003 dense windows of 17 intervals, 100 003 stream windows of 16 and a tail
    "big": {"DT": 9.44e-18,
            "alpha": 4.16e-17, "beta": 1.55e-15,                # dense, model 2, imu_avg 0 and 1
            "q": 2.16e-15},                                     # stream, model 1 imu_avg 1
}
GATE = {kind: field_gates(f) for kind, f in FLOOR.items()}
