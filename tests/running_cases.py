"""Inputs for the tests of the running family (cpi_preintegrate_running, _running_resume, _stream[s]_running) at the places
the seeded windows of cpi_amd.synth never reach: window lengths on and beside the pass boundaries of the covariance kernel
and the row groups of the mean kernel, and rotations large enough for every branch of rot_2_quat, the wide polynomial and
the Cody-Waite reduction of sincos_fast, and lane scans that compose rotations past 90 degrees.

tests/test_running_cases_cpu.py asserts, on the CPU, that these inputs still have the properties the GPU tests rely on."""
import numpy as np

from cpi_amd import synth

# Intervals the running covariance kernel stages per phase-A pass (cpi_cov_kernels.hpp, cov_body: CH); between passes the
# rotation is carried through GS_R / GS_R0 in LDS.  test_cov_running_pass_lengths reads the line out of the header: if it
# changes, EDGE_N, the cut tables of the chain test and the (n, phase) pairs of the stream test must be derived again.
PASS = {1: 14, 2: 23}
ROW_GROUP = 6                    # cpi_running_body.inc: CPI_RUN_T, rows a lane flushes through LDS at a time

# CH - 1, CH, CH + 1, 2 CH, 2 CH + 1 for both models, 70 = 5 * 14 = 3 * 23 + 1, and lengths around T = 6: with the lane
# counts in use per = ceil(N / L) comes out below T, at T and at T + 1 (N = 5, 6, 7 at L = 1; 13 at L = 2; 70 at L = 12 ...),
# and N < L for every L > 1.
EDGE_N = [1, 2, 3, 5, 6, 7, 13, 14, 15, 22, 23, 24, 28, 29, 46, 47, 70]

STREAM_CASES = [(14, 0.37), (23, 0.0), (23, 0.37), (28, 0.0), (46, 0.37)]


def tumbling_windows(W=32, N=47, seed=901, lo=4.0, hi=70.0):
    """make_windows without its edge cases, the gyro reading of window w scaled about its linearisation bias by
    linspace(lo, hi, W)[w]: |w| dt up to ~1.16 rad per interval (inside the 1.3 the RK4 of the covariance is stable for),
    wavefronts that mix lanes on the short polynomial, the wide polynomial and the reduced path, every branch of rot_2_quat."""
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=seed, edge_cases=False))
    kn = kn.copy()
    s = np.linspace(lo, hi, W)[:, None, None]
    b = lin[:, None, 0:3]
    kn[:, :, 1:4] = b + s * (kn[:, :, 1:4] - b)
    return kn, lin, q


def tumbling_stream(n, phase, seed=None, ramp=None, U=20):
    """make_stream(U, n, seed = 60 + n, phase) with the gyro columns and the gyro linearisation biases scaled by 25
    (|w| dt <= 0.38): U windows of n whole intervals, + the tail interval when phase > 0 (the first window excepted).
    ramp = (lo, hi): the scale rises along the stream instead, linspace(lo, hi) over the readings (the bias of a window with
    the scale of the reading that opens it) -- with the rate's own swing, neighbouring windows then sit on different paths of
    sincos_fast, and late tails leave the short polynomial."""
    s, u, lin, q = (t.numpy().copy() for t in synth.make_stream(U, n, seed=60 + n if seed is None else seed, phase=phase))
    if ramp is None:
        s[:, 1:4] *= 25.0
        lin[:, 0:3] *= 25.0
        return s, u, lin, q
    f = np.linspace(ramp[0], ramp[1], len(s))
    s[:, 1:4] *= f[:, None]
    lin[:, 0:3] *= f[np.arange(U) * n, None]
    return s, u, lin, q


def wdt(kn, lin):
    """|w - b_w| dt per interval of dense windows [W, N + 1, 7] (the opening reading of each interval)."""
    return np.linalg.norm(kn[:, :-1, 1:4] - lin[:, None, 0:3], axis=2) * np.diff(kn[:, :, 0], axis=1)


# ---- model 2's Jacobian rows and queries (tests/test_gpu_stj_edges.py, tests/test_hostsim_stj.py)
STJ_EDGE_N = [1, 2, 22, 23, 24, 46, 47]      # 1, 2 and CH - 1, CH, CH + 1, 2 CH, 2 CH + 1 of cov_body<2> (PASS[2])
STJ_CHAIN_N = 3 * PASS[2] + 1                # 70: the chains of tests/test_gpu_open_resume_stj.py


# seeds at which 32 (8) windows hold intervals on the short polynomial, on the long one and on the reduced path and stay below
# |w| dt = 1.3 (tests/test_running_cases_cpu.py asserts it; make_windows draws one rate profile per seed, whatever N)
STJ_LAYOUT_SEED = 950          # _ragged_layout(kn, STJ_LAYOUT_SEED): counts that keep the three regimes at every N of STJ_EDGE_N
STJ_EDGE_SEED = {1: 944, 2: 944, 22: 961, 23: 961, 24: 961, 46: 978, 47: 901}


def stj_edge_windows(N):
    """32 tumbling windows of N intervals (N of STJ_EDGE_N; N = 47 is tumbling_windows() itself)."""
    return tumbling_windows(32, N, seed=STJ_EDGE_SEED[N])


def stj_chain_windows():
    """8 tumbling windows of STJ_CHAIN_N intervals: the chains cut on and beside the passes."""
    return tumbling_windows(8, STJ_CHAIN_N, seed=988)


def stj_open_windows(model):
    """8 tumbling windows of 2 CH + 1 intervals of the model: the open views and the chains queried while open."""
    return tumbling_windows(8, 2 * PASS[model] + 1, seed=947)


def sincos_regimes(a):
    """Intervals of |w| dt on the short polynomial of sincos_fast, on the long one and on the reduced path."""
    return int((a <= 0.25).sum()), int(((a > 0.25) & (a <= 1.0)).sum()), int((a > 1.0).sum())
