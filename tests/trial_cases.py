"""Inputs and references of the trial-step tests (tests/test_trial_cpu.py, tests/test_gpu_trial.py): states and steps for
cpi_retract_batch / cpi_local_batch, the oracle's results for them, the margins of the oracle's own sign decisions, and the documented
summations of cpi_factor_cost_batch restated in NumPy.

Steps: |dtheta| is dealt out state by state from MAGS, so that every wavefront mixes the magnitudes: exact zero, 1e-300 (its square
underflows), 1e-9, 0.2, either side of the 0.25 rad switch of sincos_fast on the half angle (0.49 / 0.51), either side of the range
reduction of sincos_wide (1.99 / 2.01), either side of pi where dq.w changes sign and is flipped, 4.5 and 2 pi - 1e-3.  Axes are
random, every fifth one 1e-3 beside a coordinate axis.  Quaternions are random unit ones, every second one negated, every third one
rounded to float32 (unit to 1e-8 only).  The additive parts are O(1) biases, velocities of tens and positions of up to 5e6 with steps
of every size from 1e-9 up to the size of the entry."""
import functools
import math

import numpy as np

LD = np.longdouble
SEED = 20261018
MARGIN_MIN = 1e-9          # tests/factor_cases.MARGIN_MIN: a sign decision with |w| below this is a genuine discontinuity
MAGS = [0.0, 1e-300, 1e-9, 0.2, 0.49, 0.51, 1.99, 2.01, math.pi - 1e-3, math.pi + 1e-3, 4.5, 2 * math.pi - 1e-3]
S_ALL = 4099               # the largest batch of the GPU test; smaller ones are its head
SIZES = [1, 63, 64, 65, 257, 4099]


def _unit(rng, n, k):
    u = rng.standard_normal((n, k))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def states_and_steps(S=S_ALL, seed=SEED):
    """states [S,16], delta [S,15], other [S,16] (for localCoordinates: unrelated second states), mag index [S]; read-only."""
    g = lambda tag: np.random.default_rng([seed, tag])
    k = np.arange(S)

    def quats(tag):
        q = _unit(g(tag), S, 4)
        q[k % 3 == 2] = q[k % 3 == 2].astype(np.float32).astype(np.float64)
        q[k % 2 == 1] *= -1.0
        return q

    def rest(tag):
        r = g(tag).standard_normal((S, 12)) * np.array([0.05] * 3 + [30.0] * 3 + [0.5] * 3 + [1.0] * 3)
        r[:, 9:12] *= np.array([1.0, 1e2, 1e4, 5e6])[k % 4][:, None]
        return r

    states = np.concatenate([quats(1), rest(2)], axis=1)
    other = np.concatenate([quats(3), rest(4)], axis=1)
    axis = _unit(g(5), S, 3)
    near = (k % 5 == 4)
    e = np.eye(3)[(k // 5) % 3]
    beside = e + 1e-3 * _unit(g(6), S, 3)
    axis[near] = (beside / np.linalg.norm(beside, axis=1, keepdims=True))[near]
    mag = (k * 7 + k // len(MAGS)) % len(MAGS)          # a different magnitude in every lane, another deal in every wavefront
    dth = np.array(MAGS)[mag][:, None] * axis
    step = g(7).standard_normal((S, 12)) * np.abs(states[:, 4:]) * (10.0 ** -(k % 10))[:, None]
    delta = np.concatenate([dth, step], axis=1)
    for a in (states, delta, other, mag):
        a.setflags(write=False)
    return states, delta, other, mag


def _qmul_raw_w(q, p):
    """w of quat_multiply(q, p) before its flip and normalisation (quat_ops.h:115-128), longdouble."""
    q, p = np.asarray(q, dtype=LD), np.asarray(p, dtype=LD)
    return q[:, 3] * p[:, 3] - (q[:, :3] * p[:, :3]).sum(axis=1)


def retract_margins(states, delta):
    """|w| of the oracle's two sign decisions per state: dq.w = cos(n / 2) and the w of quat_multiply(dq, q) before its flip."""
    d = np.asarray(delta[:, :3], dtype=LD)
    n = np.sqrt((d * d).sum(axis=1))
    safe = np.where(n > 0, n, 1)
    dq = np.concatenate([np.where(n[:, None] > 0, np.sin(n / 2)[:, None] / safe[:, None] * d, 0), np.cos(n / 2)[:, None]], axis=1)
    dq = dq * np.where(dq[:, 3:4] < 0, -1, 1)
    return np.asarray(np.minimum(np.abs(dq[:, 3]), np.abs(_qmul_raw_w(dq, states[:, :4]))), dtype=np.float64)


def local_margins(x, other):
    xinv = np.asarray(x[:, :4], dtype=LD) * np.array([-1, -1, -1, 1], dtype=LD)
    return np.asarray(np.abs(_qmul_raw_w(other[:, :4], xinv)), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def oracle_results(S=S_ALL, seed=SEED):
    """(retract [S,16], local [S,15], retract of a zero step [S,16]) by oracle/cpi_oracle.c, state by state; read-only."""
    from oracle import oracle_py as op
    orc = op.oracle()
    states, delta, other, _ = states_and_steps(S, seed)
    r = np.stack([orc.retract(states[s], delta[s]) for s in range(S)])
    l = np.stack([orc.local(states[s], other[s]) for s in range(S)])
    z = np.stack([orc.retract(states[s], np.zeros(15)) for s in range(S)])
    for a in (r, l, z):
        a.setflags(write=False)
    return r, l, z


def quat_dev(got, ref):
    """Largest |difference| of the quaternion entries per state."""
    return np.abs(np.asarray(got)[:, :4] - np.asarray(ref)[:, :4]).max(axis=1)


def local_rot_dev(got, ref):
    """Rotation part of localCoordinates: |difference| / max(1, |ref|), per state."""
    return (np.abs(got[:, :3] - ref[:, :3]) / np.maximum(1.0, np.abs(ref[:, :3]))).max(axis=1)


def per_mag(e, mag):
    return {("%.4g" % MAGS[m]): float(e[mag == m].max()) for m in range(len(MAGS)) if (mag == m).any()}


# ------------------------------------------------------------------------------------------ cost
def chi2_documented(werr):
    """include/cpi_amd.h, cpi_factor_cost_batch: every square rounded by itself, added in ascending order, left to right."""
    w = np.asarray(werr, dtype=np.float64)
    acc = w[:, 0] * w[:, 0]
    for i in range(1, 15):
        acc = acc + w[:, i] * w[:, i]
    return acc


def chi2_gate(g, werr_ref):
    """32 g m^2 with m = max(1, max |werr_ref|) of the factor: each component is off by at most g m, so the sum of squares is off
    by at most 15 (2 m g m + g^2 m^2)."""
    m = np.maximum(1.0, np.abs(np.asarray(werr_ref, dtype=np.float64)).max(axis=1))
    return 32.0 * g * m * m


def total_bound(F, total):
    """|total - 0.5 fsum(chi2)| <= F 2^-53 total: the any-order summation bound for non-negative terms."""
    return F * 2.0 ** -53 * total
