"""Inputs, reference and metrics of the chain-marginalisation tests (cpi_chain_marginalize_batch).  TEST INFRASTRUCTURE ONLY.

Inputs: the chains of tests/chain_cases.py (imported, not edited): every layout of cc.LAYOUTS at seed 1 with the prior on the first
state or on every state, and cc.LONG / cc.EMPTY_WAVE as chain_cases builds them.  A DROP PLAN gives every chain its m: `scalar1` is
M = 1 with drop = NULL (chains of fewer than two states are refused), `mixed0` .. `mixed3` give chain c the entry (c + k) mod 4 of
[0, 1, n - 1, n // 2], so that one wavefront mixes all four and every chain meets each of them.

Reference: the UNDAMPED system of the factors < m and the priors <= m of a chain, assembled by the definition in numpy longdouble
(cc.dense_system on the m factor rows and m + 1 prior rows), its leading block A_EE factorised by a longdouble Cholesky, and
    [Lam eta] = [A_mm g_m] - Y^T Y',  Y = L^-1 [A_Em g_E]
in longdouble: a dense Schur complement that knows nothing of the block recursion.

Metrics (printed by the tests before anything is asserted), d = sqrt(diag(Lam_ref)):
    (c)  max_ij |Lam - ref|_ij / (d_i d_j)                           in units of cond_2(A_EE) 2^-53
    (d)  max_i  |eta - ref|_i  / (d_i sqrt(g_E^T A_EE^-1 g_E))       in the same units
    (e)  equivalence: chain_marginalize -> chain_solve(lambda = NULL) on the reduced chain; the delta rows of the kept states go
         through metric (b) of cc.Reference built on the FULL chain (the rows of the eliminated states, which the reduced solve does
         not produce, are recovered from the kept ones in longdouble: x_E = A_EE^-1 (g_E - A_Em x_m)), against the unchanged
         cc.GATE_FORWARD_*.  Metric (a) of the same vector is printed and not gated: in row m of the full system it sees the
         FORWARD error of the carried Lam and eta, which is bounded by cond_2(A_EE) 2^-53 -- what (c) and (d) gate -- and not by
         2^-53 as the residual of a solve is (measured: up to 9.9e-15 on the host twin, 2.2e-14 on the device).
m = 0 has no A_EE: there the output is compared bit for bit with the prior row, not through a metric.

Gates = 100 x the floor (the rule of tests/tol.py); a floor is the largest metric over every layout, both priors and every drop plan,
measured against the longdouble reference (profiles/chain_marginalize.md):
    float64 numpy (Cholesky plus Schur; the issue's figure, x86-64)                    (c) 1.5       (d) 0.015
    host twin (tests/hostsim/hostsim_marginalize.cpp, x86-64, -ffp-contract=off)       (c) 0.75      (d) 0.017
    device (MI355X)                                                                    (c) 0.44      (d) 0.015
((c): dense_9x17 with the prior on the first state (host) and the ragged chains with it (device); (d): the prior on every state.)
The largest cond_2(A_EE) of these inputs is 3.8e7.  The equivalence (e) measures 0.052 (host) and 0.059 (device) of cond_2(A) 2^-53.
A wrong term shows as a metric of 1e13 and more (the mutation checks of tests/test_marginalize_cpu.py).

The edges of the contract (the second half of this file) add cases, not gates: frozen chains beside failing ones, NaN at status 0, a
zero block, ffirst, clamps, call sizes and powers of two, on chains of 1 to 4 states with 4 to 8 chains per call, cc.RAGGED for the
clamps and cc.LONG once (profiles/chain_marginalize_edges.md).
"""
import functools

import numpy as np

from tests import chain_cases as cc
from tests import marginals_cases as mc

SEED = 1
FLOOR_LAM_NUMPY, FLOOR_ETA_NUMPY = 1.5, 0.015
FLOOR_LAM_HOST, FLOOR_ETA_HOST = 0.75, 0.017
FLOOR_LAM_DEVICE, FLOOR_ETA_DEVICE = 0.44, 0.015
GATE_LAM_HOST, GATE_ETA_HOST = 100 * FLOOR_LAM_HOST, 100 * FLOOR_ETA_HOST
GATE_LAM_DEVICE, GATE_ETA_DEVICE = 100 * FLOOR_LAM_DEVICE, 100 * FLOOR_ETA_DEVICE

LAYOUTS = dict(cc.LAYOUTS)
LAYOUTS["long"] = (cc.LONG, "tile")
LAYOUTS["empty_wave"] = (cc.EMPTY_WAVE, "tile")
PLANS = ("scalar1", "mixed0", "mixed1", "mixed2", "mixed3")


def plan_drop(batch, plan):
    """m of every chain under a plan, int32 [C].  A chain without states gets 0 (it is refused whatever m is)."""
    n = batch.count.astype(np.int64)
    if plan == "scalar1":
        return np.ones(batch.C, dtype=np.int32)
    k = int(plan[-1])
    pick = (np.arange(batch.C) + k) % 4
    m = np.select([pick == 0, pick == 1, pick == 2], [np.zeros_like(n), np.ones_like(n), n - 1], n // 2)
    return np.clip(m, 0, np.maximum(n - 1, 0)).astype(np.int32)


def expected_status(batch, drop):
    """0 where 0 <= m < n, -1 elsewhere (no chain of these batches has its factor rows outside hess)."""
    return np.where((drop >= 0) & (drop < batch.count), 0, -1).astype(np.int32)


def unpack_out(row):
    """[136] -> (Lam [15, 15] symmetric, eta [15]) float64."""
    P = cc.unpack_sym(np.asarray(row), 16, dtype=np.float64)
    return P[:15, :15], P[:15, 15]


def schur_longdouble(hess, prior, m):
    """hess [B, >= m, 496], prior [B, >= m + 1, 136] or None, m >= 1 -> (Lam [B, 15, 15], eta [B, 15], q [B], A_EE [B, 15 m, 15 m]) in longdouble."""
    A, g = cc.dense_system(hess[:, :m], None if prior is None else prior[:, :m + 1], np.zeros(hess.shape[0]), False)
    N = 15 * m
    L = mc.cholesky_longdouble(A[:, :N, :N])
    rhs = np.concatenate([A[:, :N, N:], g[:, :N, None]], axis=2)               # [A_Em | g_E]
    Y = np.zeros_like(rhs)
    for j in range(N):
        Y[:, j] = (rhs[:, j] - (L[:, j, :j, None] * Y[:, :j]).sum(axis=1)) / L[:, j, j][:, None]
    T = np.matmul(Y[:, :, :15].transpose(0, 2, 1), Y)                         # [B, 15, 16]
    Lam = A[:, N:, N:] - T[:, :, :15]
    eta = g[:, N:] - T[:, :, 15]
    q = np.sqrt((Y[:, :, 15] ** 2).sum(axis=1))
    return Lam, eta, q, A[:, :N, :N]


class Reference:
    """The longdouble Schur complements of a batch under drop [C]; cond [C] is cond_2 of the float64 A_EE (1 where m = 0)."""

    def __init__(self, batch, drop, with_prior=True):
        self.batch, self.drop = batch, np.asarray(drop, dtype=np.int32)
        self.status = expected_status(batch, self.drop)
        self.lam, self.eta, self.q, self.cond = {}, {}, {}, np.ones(batch.C)
        groups = {}
        for c in range(batch.C):
            if self.status[c] == 0 and self.drop[c] > 0:
                groups.setdefault(int(self.drop[c]), []).append(c)
        for m, cs in groups.items():
            hs = np.stack([batch.chain(c)[0][:m] for c in cs])
            ps = np.stack([batch.chain(c)[1][:m + 1] for c in cs]) if with_prior else None
            Lam, eta, q, AEE = schur_longdouble(hs, ps, m)
            for k, c in enumerate(cs):
                self.lam[c], self.eta[c], self.q[c] = Lam[k], eta[k], q[k]
                self.cond[c] = np.linalg.cond(np.asarray(AEE[k], dtype=np.float64))

    def check_inputs(self):
        """A condition on the INPUTS, checked before anything is compared: cond_2(A_EE) <= 1e11, a finite reference with a positive diagonal."""
        for c in self.lam:
            assert self.cond[c] <= cc.COND_MAX, (c, self.cond[c])
            assert np.isfinite(np.asarray(self.lam[c], dtype=np.float64)).all() and (np.diagonal(self.lam[c]) > 0).all() and self.q[c] > 0, c

    def metrics(self, out, chains=None):
        """(largest (c), largest (d)) of out [C, 136] over the chains with m >= 1 (all of them by default)."""
        mc_, md_ = 0.0, 0.0
        for c in (self.lam if chains is None else chains):
            if c not in self.lam:
                continue
            Lam, eta = unpack_out(out[c])
            if not (np.isfinite(Lam).all() and np.isfinite(eta).all()):
                return np.inf, np.inf
            d = np.sqrt(np.diagonal(self.lam[c]))
            unit = self.cond[c] * cc.EPS_HALF
            mc_ = max(mc_, float((np.abs(Lam - self.lam[c]) / (d[:, None] * d[None, :])).max() / unit))
            md_ = max(md_, float((np.abs(eta - self.eta[c]) / (d * self.q[c])).max() / unit))
        return mc_, md_


@functools.lru_cache(maxsize=None)
def case(layout, prior_all=False):
    """(batch, the reference of the FULL chains' solve) of a layout, computed once and shared: nobody changes them."""
    if layout == "long":
        return cc.long_case()
    if layout == "empty_wave":
        return cc.empty_wave_case()
    counts, how = LAYOUTS[layout]
    b = cc.Batch(counts, seed=SEED, prior_all=prior_all, layout=how)
    full = cc.Reference(b)
    full.check_inputs()
    return b, full


@functools.lru_cache(maxsize=None)
def reference(layout, prior_all, plan):
    """(batch, drop [C], the Schur reference, the full chains' reference) of a layout under a drop plan."""
    b, full = case(layout, prior_all)
    drop = plan_drop(b, plan)
    ref = Reference(b, drop)
    ref.check_inputs()
    return b, drop, ref, full


def cases():
    """(layout, prior_all) of every batch: LONG and EMPTY_WAVE exist with the prior on the first state only."""
    return [(name, p) for name in LAYOUTS for p in ((False,) if name in ("long", "empty_wave") else (False, True))]


def reduced(batch, drop, out, status):
    """The arguments of the reduced chains' solve: (first, count, ffirst, prior) with out[c] at state first_c + m_c of a copy of prior.
    A chain that was refused or failed keeps no states."""
    good = np.asarray(status) == 0
    m = np.where(good, drop, 0).astype(np.int64)
    first, ffirst = batch.first + m, batch.ffirst + m
    count = np.where(good, batch.count - m, 0).astype(np.int32)
    prior = batch.prior.copy()
    for c in np.nonzero(good)[0]:
        prior[first[c]] = out[c]
    return first, count, ffirst, prior


def equivalence(full, drop, status, delta):
    """Metrics (a), (b) of cc.Reference, built on the FULL chains, for delta [S, 15] of the REDUCED chains.  The rows of the eliminated
    states, which that solve does not write, are recovered from the kept ones in longdouble, x_E = A_EE^-1 (g_E - A_Em x_m): they
    satisfy their own equations exactly, so every residual and every error the metrics see is the reduced solve's."""
    b = full.batch
    d = np.full((b.S, 15), np.nan, dtype=np.longdouble)
    chains = []
    for c in full.A:
        if status[c] != 0:
            continue
        rows, N = b.rows(c), 15 * int(drop[c])
        kept = np.asarray(delta[rows.start + int(drop[c]):rows.stop], dtype=np.longdouble)
        d[rows.start + int(drop[c]):rows.stop] = kept
        if N and np.isfinite(np.asarray(kept, dtype=np.float64)).all():
            A, g = full.A[c], full.g[c]
            rhs = g[:N] - A[:N, N:N + 15] @ kept[0]
            d[rows.start:rows.start + int(drop[c])] = cc.solve_longdouble(A[None, :N, :N], rhs[None])[0].reshape(-1, 15)
        chains.append(c)
    return full.metrics(d, chains)


# ---------------------------------------------------------------------------------------------------------------------------------
# The edges of the contract (tests/test_gpu_marginalize_edges.py and the twin tests of tests/test_marginalize_cpu.py).  The chains are
# those of tests/chain_cases.py; what a case must give is asserted by tests/marginalize_edge_checks.py, for twin and device alike.
# No gate is added: the reference-gated cases below (LONG, the odd power of two) use GATE_LAM_* / GATE_ETA_* above as they are.
#
# (a) the bad batch of cc.failure_plan() with an m of its own per chain: in both plans every wavefront holds chains that are FROZEN
# (m below the wavefront's largest) while a mate fails, and chains whose broken block sits exactly at state m -- in Pr_m, which a
# frozen chain goes on adding to its carried block in every later trip without it counting as a failure.
FREEZE_DROPS = ([1, 3, 0, 2, 3, 1, 2, 0], [3, 1, 2, 3, 0, 3, 1, 2])
FREEZE_STATUS = ([1, 1, 0, 0, 0, 0, 2, 0], [1, 1, 0, 3, 0, 0, 0, 0])
# (b) the good batch: wavefront 0 and wavefront 1 each freeze chains at trip 0 (m = 0) and at trip 1 beside an m of 3
POISON_DROP = [1, 3, 0, 2, 1, 3, 0, 2]
POISON_CHAINS = (0, 2, 4, 6)
POISON_ENTRY = 7                                   # packed (1, 3)
LONG_DROP = [63, 0, 0, 1]                          # the chain without states is refused whatever its m is
NAN_STATUS = {1: [0, 0, 0, 0], 2: [2, 0, 0, 0], 3: [2, 3, 3, 0]}
SCALE_EXPONENTS = (2, -2, 300, -300, 301)
FFIRST_NULL_DROPS = (((5, 3, 5, 1, 2), [2, 1, 4, 0, 1]), ((5,) * 5, 3))


def failure_status(drop):
    """What cc.failure_plan()'s bad batch must report under drop [8]: s + 1 of cc.FAILURES[c] if s < m_c, else 0."""
    return [cc.FAILURES[c][0] + 1 if c in cc.FAILURES and cc.FAILURES[c][0] < int(drop[c]) else 0 for c in range(8)]


def freeze_failure_case(k):
    """(the clean batch, the bad batch, drop [8], the status the bad batch must give) of plan k of (a)."""
    good, bad, _ = cc.failure_plan()
    drop = np.asarray(FREEZE_DROPS[k], dtype=np.int32)
    assert failure_status(drop) == FREEZE_STATUS[k]
    return good.b, bad.b, drop, FREEZE_STATUS[k]


def prior_row_m(b, drop, c):
    """The row of b.prior that is Pr_m of chain c."""
    return int(b.first[c]) + int(drop[c])


def without_prior_m(b, drop):
    """b.prior with Pr_m of every chain zeroed: out is then (N + 0.0) + 0.0 = N, the carried block itself, to the bit."""
    prior = b.prior.copy()
    for c in range(b.C):
        if 0 <= drop[c] < b.count[c]:
            prior[prior_row_m(b, drop, c)] = 0.0
    return prior


def poison_case(what):
    """(the good batch of cc.failure_plan(), its prior with Pr_m of POISON_CHAINS poisoned, drop [8]).  what = "negative": -1e12 on
    all 15 diagonal entries (every pivot of every frozen trip fails); "nan": a NaN at packed entry POISON_ENTRY."""
    b = cc.failure_plan()[0].b
    drop = np.asarray(POISON_DROP, dtype=np.int32)
    prior = b.prior.copy()
    for c in POISON_CHAINS:
        row = prior_row_m(b, drop, c)
        if what == "negative":
            prior[row, cc.tri(np.arange(15)) + np.arange(15)] = -1e12
        else:
            prior[row, POISON_ENTRY] = np.nan
    return b, prior, drop


def long_freeze_case():
    """(the batch of cc.LONG, its prior with a NaN at POISON_ENTRY of state 1 of the chain of two states, drop [4]).  That row is the
    chain's Pr_m: the chain is frozen from trip 1 on and re-reads it in each of the 62 trips the chain of 64 states still makes."""
    b = cc.long_case()[0]
    drop = np.asarray(LONG_DROP, dtype=np.int32)
    assert b.count.tolist() == cc.LONG == [64, 1, 0, 2]
    prior = b.prior.copy()
    prior[prior_row_m(b, drop, 3), POISON_ENTRY] = np.nan
    return b, prior, drop


def nan_sets(M):
    """chain -> the packed entries of its out row that cc.nan_plan() under M must make NaN at status 0 (the rows of chains whose
    status is not 0 are all NaN; every other entry has the bits of the clean call):
        M = 2, chain 1   the NaN sits at (5, 5) of the TRAILING block of factor 1, which state 2 receives as it is
        M = 2, chain 2   at (3, 5) of U of factor 1: column 5 of W = L^-1 U, hence row and column 5 of W^T W and entry 5 of W^T y
        M = 3, chain 3   in g of the trailing part of factor 2: eta[14]"""
    col5 = {cc.tri(5) + i for i in range(6)} | {cc.tri(j) + 5 for j in range(6, 15)} | {cc.tri(15) + 5}
    return {1: {}, 2: {1: {cc.tri(5) + 5}, 2: col5}, 3: {3: {cc.tri(15) + 14}}}[M]


def rhs_nan_case():
    """(the clean batch of cc.nan_plan(), its prior with a NaN in eta[3] of state 0 of chain 0): a right-hand side further back than
    what state m receives directly, for M = 2."""
    b = cc.nan_plan()[0].b
    prior = b.prior.copy()
    prior[b.first[0], cc.tri(15) + 3] = np.nan
    return b, prior


def zero_block_case(negative):
    """(batch, hess with chain 0's one factor row all 0.0 or all -0.0): two chains of 2 and 3 states, to be run without a prior."""
    b = cc.Batch([2, 3], seed=7)
    hess = b.hess.copy()
    hess[b.ffirst[0]] = -0.0 if negative else 0.0
    return b, hess


def ffirst_drops(count):
    """The m of the ffirst boundary cases: n - 1 (every factor row is read), 0 (none is) and 1 where the chain has two states (fewer
    rows are read than the refusal looks at)."""
    n = np.asarray(count, dtype=np.int32)
    return [np.maximum(n - 1, 0), np.zeros_like(n), np.minimum(1, np.maximum(n - 1, 0))]


@functools.lru_cache(maxsize=None)
def scaled_case():
    """(the unscaled batch of cc.scaled_batch, drop [C] of plan mixed2, the longdouble Schur reference): computed once, not changed."""
    b = cc.scaled_reference()[0]
    drop = plan_drop(b, "mixed2")
    ref = Reference(b, drop)
    ref.check_inputs()
    return b, drop, ref
