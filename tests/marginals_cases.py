"""Inputs, reference and metric of the chain-marginals tests (cpi_chain_marginals_batch).  TEST INFRASTRUCTURE ONLY.

Inputs: the chains of tests/chain_cases.py (imported, not edited): every layout of cc.LAYOUTS, the prior on the first state or on every
state, seed 1.

Reference: the dense system cc.dense_system(...) of a chain in numpy longdouble (lam = 0, or the damped matrix where a test says so),
its longdouble Cholesky A = L L^T, X = L^-1 by forward substitution in longdouble, and Sigma = X^T X = L^-T L^-1 -- a dense inverse
that knows nothing of the block recursion.  Only the blocks the entry returns are formed.

Metric (printed by the tests before anything is asserted):
    e      = max over every cov block and every cross block of a chain of |out - ref|_ij / sqrt(ref_ii ref_jj), the diagonals of ref
             being those of the two states involved (an error relative to the standard deviations: a correlation error)
    metric = e / (cond_2(A) 2^-53)

Gates = 100 x the floor (the rule of tests/tol.py); a floor is the largest metric over every layout with the prior on the first state
and on every state, undamped.  Measured (profiles/chain_marginals.md):
    float64 numpy restatement of the recursion (the issue's figure, x86-64)     0.058
    host twin (tests/hostsim/hostsim_marginals.cpp, x86-64, -ffp-contract=off)   0.057
    device (MI355X)                                                              0.046
The largest cond_2(A) of these inputs is 5.1e9 (the input condition cond <= 1e11 of tests/chain_cases.py holds), the smallest
eigenvalue of the resulting correlation matrices 1.1e-3.  A wrong term shows as a metric of 1e5 and more (the mutation checks of
tests/test_marginals_cpu.py).
"""
import functools

import numpy as np

from tests import chain_cases as cc

SEED = 1
FLOOR_NUMPY = 0.058
FLOOR_HOST = 0.057
FLOOR_DEVICE = 0.046
GATE_HOST = 100 * FLOOR_HOST
GATE_DEVICE = 100 * FLOOR_DEVICE

R15, C15 = cc._tri_rc(15)


def unpack_cov(rows):
    """[..., 120] packed upper triangles -> [..., 15, 15] symmetric float64."""
    return cc.unpack_sym(np.asarray(rows), 15, dtype=np.float64)


def unpack_cross(rows):
    """[..., 225] column-major -> [..., 15, 15] with [i, c] = entry (row i of state s, column c of state s + 1)."""
    rows = np.asarray(rows)
    return rows.reshape(rows.shape[:-1] + (15, 15)).swapaxes(-1, -2)


def cholesky_longdouble(A):
    A = np.array(A, dtype=np.longdouble)
    N = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(N):
        d = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        L[:, j, j] = np.sqrt(d)
        if j + 1 < N:
            L[:, j + 1:, j] = (A[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, j, None, :j]).sum(axis=2)) / L[:, j, j][:, None]
    return L


def inverse_blocks_longdouble(A):
    """A [B, 15 n, 15 n] -> (diag [B, n, 15, 15], cross [B, n - 1, 15, 15]) of A^-1 in longdouble: Cholesky, X = L^-1, Sigma = X^T X."""
    L = cholesky_longdouble(A)
    B, N = L.shape[0], L.shape[1]
    n = N // 15
    X = np.zeros_like(L)
    for j in range(N):                                   # row j of L^-1 (lower triangular)
        X[:, j, :j] = -(L[:, j, :j, None] * X[:, :j, :j]).sum(axis=1) / L[:, j, j][:, None]
        X[:, j, j] = 1.0 / L[:, j, j]
    diag = np.zeros((B, n, 15, 15), dtype=np.longdouble)
    cross = np.zeros((B, max(n - 1, 0), 15, 15), dtype=np.longdouble)
    for s in range(n):
        a = X[:, :, 15 * s:15 * s + 15]
        diag[:, s] = np.matmul(a.transpose(0, 2, 1), a)
        if s + 1 < n:
            cross[:, s] = np.matmul(a.transpose(0, 2, 1), X[:, :, 15 * s + 15:15 * s + 30])
    return diag, cross


class Reference:
    """The dense systems of a batch and the blocks of their longdouble inverses; cond [C] is cond_2 of the float64 matrix."""

    def __init__(self, batch, lam=None, diagonal=False, with_prior=True):
        self.batch = batch
        lam = np.zeros(batch.C) if lam is None else np.broadcast_to(np.asarray(lam, dtype=np.float64), (batch.C,))
        self.diag, self.cross, self.A, self.cond = {}, {}, {}, np.zeros(batch.C)
        for n in sorted(set(int(v) for v in batch.count if v > 0)):
            cs = [c for c in range(batch.C) if batch.count[c] == n]
            hs = np.stack([batch.chain(c)[0] for c in cs]).reshape(len(cs), n - 1, 496)
            ps = np.stack([batch.chain(c)[1] for c in cs]) if with_prior else None
            A, _ = cc.dense_system(hs, ps, lam[cs], diagonal)
            d, x = inverse_blocks_longdouble(A)
            for k, c in enumerate(cs):
                self.A[c], self.diag[c], self.cross[c] = A[k], d[k], x[k]
                self.cond[c] = np.linalg.cond(np.asarray(A[k], dtype=np.float64))

    def check_inputs(self):
        """A condition on the INPUTS, checked before anything is compared: finite float64 Cholesky, cond <= 1e11, a finite reference."""
        for c in self.A:
            assert np.isfinite(np.linalg.cholesky(np.asarray(self.A[c], dtype=np.float64))).all(), c
            assert np.isfinite(np.asarray(self.diag[c], dtype=np.float64)).all() and self.cond[c] <= cc.COND_MAX, (c, self.cond[c])

    def min_correlation_eigenvalue(self):
        """Smallest eigenvalue over the chains of the correlation matrix of a state's reference block."""
        worst = np.inf
        for c in self.diag:
            D = np.asarray(self.diag[c], dtype=np.float64)
            sd = np.sqrt(np.einsum("sii->si", D))
            worst = min(worst, float(np.linalg.eigvalsh(D / (sd[:, :, None] * sd[:, None, :])).min()))
        return worst

    def chain_error(self, c, cov, cross):
        """e of chain c: cov [S, 120], cross [S, 225] or None, as the entry wrote them."""
        rows = self.batch.rows(c)
        n = int(self.batch.count[c])
        D = self.diag[c]
        sd = np.sqrt(np.einsum("sii->si", D))
        got = unpack_cov(cov[rows]).astype(np.longdouble)
        if not np.isfinite(np.asarray(got, dtype=np.float64)).all():
            return np.inf
        e = float((np.abs(got - D) / (sd[:, :, None] * sd[:, None, :])).max())
        if cross is not None and n > 1:
            gx = unpack_cross(cross[rows][:n - 1]).astype(np.longdouble)
            if not np.isfinite(np.asarray(gx, dtype=np.float64)).all():
                return np.inf
            e = max(e, float((np.abs(gx - self.cross[c]) / (sd[:-1, :, None] * sd[1:, None, :])).max()))
        return e

    def metric(self, cov, cross, chains=None):
        """The largest e / (cond_2(A) 2^-53) over the chains (all with states by default)."""
        return max([self.chain_error(c, cov, cross) / (self.cond[c] * cc.EPS_HALF) for c in (self.A if chains is None else chains)] or [0.0])


@functools.lru_cache(maxsize=None)
def case(layout, prior_all, lam_v=None):
    """(batch, lam [C] or None, reference) of a layout, computed once and shared: nobody changes them.  lam_v: identity damping."""
    counts, how = cc.LAYOUTS[layout]
    b = cc.Batch(counts, seed=SEED, prior_all=prior_all, layout=how)
    lam = cc.lam_of(b, lam_v)
    ref = Reference(b, lam, False)
    ref.check_inputs()
    return b, lam, ref


def untouched_rows(b, chains=None):
    m = np.ones(b.S, dtype=bool)
    for c in (range(b.C) if chains is None else chains):
        m[b.rows(c)] = False
    return m


def last_rows(b, chains=None):
    """The last state of every chain with states: its cross row is not written."""
    return np.array([int(b.first[c]) + int(b.count[c]) - 1 for c in (range(b.C) if chains is None else chains) if b.count[c] > 0], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# The edge cases of tests/chain_cases.py that have a reference: the same batches, the blocks of their dense inverses.
@functools.lru_cache(maxsize=None)
def long_case():
    """(batch, reference) of cc.LONG."""
    b, _ = cc.long_case()
    ref = Reference(b)
    ref.check_inputs()
    return b, ref


@functools.lru_cache(maxsize=None)
def scaled_reference():
    """(the unscaled batch, its reference): with hess and prior times 2^e the inverse is 2^-e times this one, exactly, so
    metric(cov * 2^e, cross * 2^e) against this reference is the metric of the scaled call."""
    b, _ = cc.scaled_reference()
    ref = Reference(b)
    ref.check_inputs()
    return b, ref


@functools.lru_cache(maxsize=None)
def diagonal_case():
    """(batch, lam, reference): the ragged chains under diagonal damping 0.25, against the damped matrix's own inverse."""
    b = cc.Batch(cc.RAGGED, seed=SEED)
    lam = cc.lam_of(b, 0.25)
    ref = Reference(b, lam, True)
    ref.check_inputs()
    return b, lam, ref
