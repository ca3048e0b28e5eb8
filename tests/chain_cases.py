"""Inputs, reference and metrics of the chain-solve tests (cpi_chain_solve_batch).  TEST INFRASTRUCTURE ONLY.

Generator: IMU-like chains.  Factor k of a chain is the whitened Jacobian row block [A1 A2 b] = R [-Phi, I + E, r] over the tangent
vectors [theta bg v ba p] of states k and k + 1:
    R    upper triangular, row scales [1e3, 1e4, 1e2, 1e3, 1e2] per tangent block (a square-root information of realistic spread)
    Phi  = I + 0.05 N, plus 0.1 I in the (p, v) block (position integrates velocity);  E = 0.05 N;  r = N
and its hess row is the packed upper triangle of [A1 A2 b]^T [A1 A2 b] (the packing of cpi_factor_hessian_*).  A prior of
information 0.1 diag(scales)^2 sits on each chain's first state, or on every state.  Unstructured random Jacobians are NOT used:
their chains lose positive definiteness in float64 within a few dozen states (cond 2.5e27 at 17 states).

Reference: the dense system assembled by the definition of include/cpi_amd.h in numpy longdouble, Cholesky and the two substitutions
in longdouble, vectorised over the chains of equal length (modelled on tests/tol.py: sqrt_info_longdouble).

Metrics (printed by the tests before anything is asserted):
    (a) componentwise backward error in longdouble    max_i |A delta - g|_i / (|A| |delta| + |g|)_i
    (b) forward error over its bound                  (|delta - ref|_inf / |ref|_inf) / (cond_2(A) 2^-53)

Gates = 100 x the floor (the rule of tests/tol.py); a floor is the largest value measured over every layout of the tests and never
below the rounding of the format (2^-53 for (a); for (b) the unit is already cond 2^-53).  Measured (profiles/chain_solve.md):
    host twin (tests/hostsim/hostsim_chain.cpp, x86-64)               (a) 6.6e-16   (b) 3.8e-01
    device (MI355X)                                                   (a) 5.9e-16   (b) 2.2e-01
    float64 LAPACK (numpy.linalg.solve) on the same systems           (a) 2.7e-14   (b) 3.2e-01
((a): the 1000 chains of 5 states; (b): the ragged chains without a prior, identity damping; LAPACK's row is over the layouts of the
table in the profile).
"""
import functools

import numpy as np

EPS_HALF = 2.0 ** -53
SCALES = np.repeat(np.array([1e3, 1e4, 1e2, 1e3, 1e2]), 3)
COND_MAX = 1e11

FLOOR_BACKWARD_HOST, FLOOR_FORWARD_HOST = 6.6e-16, 3.8e-1
FLOOR_BACKWARD_DEVICE, FLOOR_FORWARD_DEVICE = 5.9e-16, 2.2e-1
GATE_BACKWARD_HOST, GATE_FORWARD_HOST = 100 * max(FLOOR_BACKWARD_HOST, EPS_HALF), 100 * FLOOR_FORWARD_HOST
GATE_BACKWARD_DEVICE, GATE_FORWARD_DEVICE = 100 * max(FLOOR_BACKWARD_DEVICE, EPS_HALF), 100 * FLOOR_FORWARD_DEVICE

RAGGED = [0, 1, 2, 3, 17, 40, 5, 16, 15, 1, 2]


def _tri_rc(n):
    """(rows, cols) of the packed upper triangle of an n x n matrix in storage order: (i, d) at i + d (d + 1) / 2."""
    cols = np.repeat(np.arange(n), np.arange(1, n + 1))
    rows = np.arange(n * (n + 1) // 2) - cols * (cols + 1) // 2
    return rows, cols


R31, C31 = _tri_rc(31)
R16, C16 = _tri_rc(16)


def pack_upper(M):
    n = M.shape[-1]
    r, c = _tri_rc(n)
    return np.ascontiguousarray(M[..., r, c])


def unpack_sym(p, n, dtype=np.longdouble):
    r, c = _tri_rc(n)
    M = np.zeros(p.shape[:-1] + (n, n), dtype=dtype)
    M[..., r, c] = p
    M[..., c, r] = p
    return M


class Batch:
    """C chains with their arrays in the layout of the entry.  hess / prior rows that belong to nothing hold NaN: a kernel that reads
    one shows it."""

    def __init__(self, counts, seed=0, prior_all=False, layout="tile", gap=2):
        rng = np.random.default_rng(seed)
        self.count = np.asarray(counts, dtype=np.int32)
        self.C = len(counts)
        self.G = max(1, int(self.count.max()) if self.C else 1)
        n = self.count.astype(np.int64)
        nf = np.maximum(n - 1, 0)
        if layout == "tile":                      # what NULL first / ffirst mean: chain c in the slots c * G and c * (G - 1)
            self.first = np.arange(self.C, dtype=np.int64) * self.G
            self.ffirst = np.arange(self.C, dtype=np.int64) * (self.G - 1)
            self.S, self.F = self.C * self.G, self.C * (self.G - 1)
        else:                                     # "gaps": gap rows between chains; "reverse": chains stored last to first, with gaps
            order = np.arange(self.C) if layout == "gaps" else np.arange(self.C)[::-1]
            self.first, self.ffirst = np.zeros(self.C, np.int64), np.zeros(self.C, np.int64)
            s = f = gap
            for c in order:
                self.first[c], self.ffirst[c] = s, f
                s += int(n[c]) + gap
                f += int(nf[c]) + gap
            self.S, self.F = s, f
        self.explicit = layout != "tile"
        self.hess = np.full((max(self.F, 1), 496), np.nan)
        self.prior = np.full((max(self.S, 1), 136), np.nan)
        lam0 = 0.1 * SCALES ** 2
        for c in range(self.C):
            for k in range(int(nf[c])):
                self.hess[self.ffirst[c] + k] = pack_upper(_factor(rng))
            for s in range(int(n[c])):
                P = np.zeros((16, 16))
                if s == 0 or prior_all:
                    P[:15, :15] = np.diag(lam0)
                    P[:15, 15] = P[15, :15] = lam0 * 0.01 * rng.standard_normal(15)
                P[15, 15] = np.nan                 # entry 135 is never read
                self.prior[self.first[c] + s] = pack_upper(P)
        self.hess = self.hess[:self.F] if self.F else self.hess[:0]
        self.prior = self.prior[:self.S] if self.S else self.prior[:0]

    @classmethod
    def from_arrays(cls, count, first, ffirst, hess, prior):
        """A batch over arrays that something else produced (the device's own hess)."""
        b = cls.__new__(cls)
        b.count, b.first, b.ffirst = np.asarray(count, dtype=np.int32), np.asarray(first, dtype=np.int64), np.asarray(ffirst, dtype=np.int64)
        b.C, b.G, b.hess, b.prior = len(b.count), max(1, int(b.count.max())), np.asarray(hess), np.asarray(prior)
        b.S, b.F, b.explicit = b.prior.shape[0], b.hess.shape[0], True
        return b

    def chain(self, c):
        n = int(self.count[c])
        return (self.hess[self.ffirst[c]:self.ffirst[c] + max(n - 1, 0)], self.prior[self.first[c]:self.first[c] + n])

    def rows(self, c):
        return slice(int(self.first[c]), int(self.first[c]) + int(self.count[c]))


def _factor(rng):
    N = rng.standard_normal
    U = np.triu(np.eye(15) + 0.1 * N((15, 15)))
    R = SCALES[:, None] * U
    Phi = np.eye(15) + 0.05 * N((15, 15))
    Phi[12:15, 6:9] += 0.1 * np.eye(3)
    M = np.concatenate([-Phi, np.eye(15) + 0.05 * N((15, 15)), N((15, 1))], axis=1)
    A = R @ M
    return A.T @ A


def dense_system(hess, prior, lam, diagonal):
    """hess [B, n - 1, 496], prior [B, n, 136] or None, lam [B] -> (A [B, 15 n, 15 n], g [B, 15 n]) in longdouble, by the definition."""
    B, n = hess.shape[0], hess.shape[1] + 1
    A = np.zeros((B, 15 * n, 15 * n), dtype=np.longdouble)
    g = np.zeros((B, 15 * n), dtype=np.longdouble)
    for k in range(n - 1):
        H = unpack_sym(hess[:, k], 31)
        o = 15 * k
        A[:, o:o + 30, o:o + 30] += H[:, :30, :30]
        g[:, o:o + 30] += H[:, :30, 30]
    if prior is not None:
        for s in range(n):
            P = unpack_sym(np.where(np.arange(136) == 135, 0.0, prior[:, s]), 16)
            o = 15 * s
            A[:, o:o + 15, o:o + 15] += P[:, :15, :15]
            g[:, o:o + 15] += P[:, :15, 15]
    i = np.arange(15 * n)
    lam = np.asarray(lam, dtype=np.longdouble)[:, None]
    A[:, i, i] += lam * A[:, i, i] if diagonal else lam
    return A, g


def solve_longdouble(A, g):
    """Cholesky A = L L^T and the two substitutions in longdouble, vectorised over the batch."""
    A = np.array(A, dtype=np.longdouble)
    B, N = g.shape
    L = np.zeros_like(A)
    for j in range(N):
        d = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        L[:, j, j] = np.sqrt(d)
        if j + 1 < N:
            L[:, j + 1:, j] = (A[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, j, None, :j]).sum(axis=2)) / L[:, j, j][:, None]
    y = np.zeros_like(g)
    for j in range(N):
        y[:, j] = (g[:, j] - (L[:, j, :j] * y[:, :j]).sum(axis=1)) / L[:, j, j]
    x = np.zeros_like(g)
    for j in range(N - 1, -1, -1):
        x[:, j] = (y[:, j] - (L[:, j + 1:, j] * x[:, j + 1:]).sum(axis=1)) / L[:, j, j]
    return x


class Reference:
    """The dense systems of a batch and their longdouble solutions.  delta [S, 15] float64 (NaN in rows of no chain)."""

    def __init__(self, batch, lam=None, diagonal=False, with_prior=True):
        self.batch = batch
        lam = np.zeros(batch.C) if lam is None else np.broadcast_to(np.asarray(lam, dtype=np.float64), (batch.C,))
        self.A, self.g, self.x, self.cond = {}, {}, {}, np.zeros(batch.C)
        self.delta = np.full((batch.S, 15), np.nan)
        for n in sorted(set(int(v) for v in batch.count if v > 0)):
            cs = [c for c in range(batch.C) if batch.count[c] == n]
            hs = np.stack([batch.chain(c)[0] for c in cs]).reshape(len(cs), n - 1, 496)
            ps = np.stack([batch.chain(c)[1] for c in cs]) if with_prior else None
            A, g = dense_system(hs, ps, lam[cs], diagonal)
            x = solve_longdouble(A, g)
            for k, c in enumerate(cs):
                self.A[c], self.g[c], self.x[c] = A[k], g[k], x[k]
                self.cond[c] = np.linalg.cond(np.asarray(A[k], dtype=np.float64))
                self.delta[batch.rows(c)] = np.asarray(x[k], dtype=np.float64).reshape(n, 15)

    def check_inputs(self):
        """A condition on the INPUTS, checked before anything is compared: every system has a finite float64 Cholesky and cond <= 1e11."""
        for c in self.A:
            L = np.linalg.cholesky(np.asarray(self.A[c], dtype=np.float64))
            assert np.isfinite(L).all() and np.isfinite(self.x[c]).all(), c
            assert self.cond[c] <= COND_MAX, (c, self.cond[c])

    def metrics(self, delta, chains=None):
        """(largest (a), largest (b)) of delta [S, 15] over the chains (all with states by default)."""
        a = b = 0.0
        for c in (self.A if chains is None else chains):
            d = np.asarray(delta[self.batch.rows(c)], dtype=np.longdouble).reshape(-1)
            if not np.isfinite(np.asarray(d, dtype=np.float64)).all():
                return np.inf, np.inf
            A, g, x = self.A[c], self.g[c], self.x[c]
            if not np.any(x):                                   # a zero right-hand side: the exact solution is zero, and so must delta be
                if np.any(d):
                    return np.inf, np.inf
                continue
            a = max(a, float((np.abs(A @ d - g) / (np.abs(A) @ np.abs(d) + np.abs(g))).max()))
            b = max(b, float(np.abs(d - x).max() / np.abs(x).max()) / (self.cond[c] * EPS_HALF))
        return a, b

    def lapack_metrics(self):
        out = np.full((self.batch.S, 15), np.nan)
        for c in self.A:
            n = int(self.batch.count[c])
            out[self.batch.rows(c)] = np.linalg.solve(np.asarray(self.A[c], dtype=np.float64), np.asarray(self.g[c], dtype=np.float64)).reshape(n, 15)
        return self.metrics(out)


# every layout of the tests: name -> (counts, layout)
LAYOUTS = {
    "dense_9x17": ([17] * 9, "tile"),
    "ragged": (RAGGED, "tile"),
    "one_1": ([1], "tile"),
    "one_2": ([2], "tile"),
    "one_3": ([3], "tile"),
    "gaps": (RAGGED, "gaps"),
    "reverse": (RAGGED, "reverse"),
}
DAMPINGS = (("none", None, False), ("identity", 3.0, False), ("diagonal", 0.25, True))


def lam_of(batch, value):
    """per-chain lambda: the value scaled a little differently per chain, or None."""
    return None if value is None else value * (1.0 + 0.125 * (np.arange(batch.C) % 4))


# ---------------------------------------------------------------------------------------------------------------------------------
# The edges of the contract (tests/test_gpu_chain_edges.py and the twin tests of tests/test_chain_cpu.py / test_marginals_cpu.py):
# one call of an entry with any subset of first / count / ffirst, a G and an S of its own, and the builders of the cases.  What a
# case must give is asserted by tests/chain_edge_checks.py, for the twins and for the device alike.
class Call:
    """One call of cpi_chain_solve_batch (and of cpi_chain_marginals_batch after it) on the arrays of batch b.  first / count / ffirst:
    arrays [C], or None for NULL; G and S default to the batch's; S < b.S passes the leading S rows of delta / prior / cov / cross."""

    def __init__(self, b, first=None, count=None, ffirst=None, G=None, S=None, lam=None, diagonal=False, with_prior=True, C=None):
        arr = lambda v, dt: None if v is None else np.ascontiguousarray(v, dtype=dt)
        self.b, self.first, self.count, self.ffirst = b, arr(first, np.int64), arr(count, np.int32), arr(ffirst, np.int64)
        given = [v for v in (self.first, self.count, self.ffirst) if v is not None]
        self.C = (len(given[0]) if given else b.C) if C is None else C
        self.G, self.S = int(b.G if G is None else G), int(b.S if S is None else S)
        self.lam, self.diagonal, self.with_prior = arr(lam, np.float64), bool(diagonal), with_prior

    @classmethod
    def explicit(cls, b, chains=None, lam=None, **kw):
        """first, count and ffirst of the batch, all three given; chains: only these, in this order."""
        idx = np.arange(b.C) if chains is None else np.asarray(chains)
        lam = None if lam is None else np.asarray(lam, dtype=np.float64)[idx]
        return cls(b, first=b.first[idx], count=b.count[idx], ffirst=b.ffirst[idx], lam=lam, **kw)

    def states(self, c):
        """(first state, number of states) of chain c as include/cpi_amd.h clamps them: count into [0, G], first into [0, S], the
        chain clipped at S."""
        f = int(self.first[c]) if self.first is not None else c * self.G
        n = int(self.count[c]) if self.count is not None else self.G
        n = min(max(n, 0), self.G)
        f = min(max(f, 0), self.S)
        return f, min(n, self.S - f)

    def rows(self, c):
        f, n = self.states(c)
        return slice(f, f + n)

    def owned(self):
        """(rows [b.S] that belong to a chain, rows that are a chain's last state: their cross row is not written)."""
        own, last = np.zeros(self.b.S, dtype=bool), np.zeros(self.b.S, dtype=bool)
        for c in range(self.C):
            f, n = self.states(c)
            own[f:f + n] = True
            if n > 0:
                last[f + n - 1] = True
        return own, last


def clone(b):
    """The batch with arrays of its own."""
    n = Batch.__new__(Batch)
    n.__dict__.update(b.__dict__)
    n.count, n.first, n.ffirst, n.hess, n.prior = b.count.copy(), b.first.copy(), b.ffirst.copy(), b.hess.copy(), b.prior.copy()
    return n


# chain -> (state s, pivot k) of a non-positive pivot: all four chains of wavefront 0 at different states, the chain in lanes 48 .. 63,
# pivots 0, 7 and 14, a chain's first and last state; chains 4 and 7 stay as they are
FAILURES = {0: (0, 0), 1: (0, 14), 2: (3, 14), 3: (2, 7), 5: (3, 0), 6: (1, 14)}
FAILURE_STATUS = [1, 1, 4, 3, 0, 4, 2, 0]


def failure_plan():
    """(the clean call, the call with the pivots of FAILURES made negative, the status it must give).  -1e12 on the diagonal of the
    state's prior block, where the factors and the prior add a few times SCALES^2 <= 1e8."""
    good = Batch([4] * 8, seed=7, prior_all=True)
    bad = clone(good)
    for c, (s, k) in FAILURES.items():
        bad.prior[bad.first[c] + s, k + k * (k + 1) // 2] = -1e12
    return Call(good), Call(bad), FAILURE_STATUS


def tri(d):
    return d * (d + 1) // 2


# chain -> (factor, entry of its hess row, status): a NaN in a D block (twice: from the factor's leading and from its trailing block),
# in a U block, and in g of the chain's last state alone -- every pivot is fine then, and every delta row of the chain is NaN
NANS = {0: (1, tri(3) + 3, 2), 1: (1, tri(20) + 20, 3), 2: (1, tri(20) + 3, 3), 3: (2, tri(30) + 29, 0)}


def nan_plan():
    """(the clean call, the call with the NaN entries of NANS, the status it must give)."""
    good = Batch([4] * 4, seed=7, prior_all=True)
    bad = clone(good)
    for c, (k, e, _) in NANS.items():
        bad.hess[bad.ffirst[c] + k, e] = np.nan
    return Call(good), Call(bad), [NANS[c][2] for c in range(4)]


def ffirst_boundary_cases():
    """(the unmoved call, [(chain, ffirst, call, status)]): the last valid and the first invalid factor row of a chain of three and of
    two states, and a chain of one state with an ffirst far outside.  F = 16, rows 14 and 15 are gap rows; where the new ffirst is
    valid the chain's own factor rows are copied there first, so status 0 comes with the bits of the unmoved call."""
    base = Batch([3, 2, 1, 4], seed=3, layout="gaps")
    assert base.F == 16 and int(base.ffirst[3]) + 3 == 14
    cases = []
    for c, ff, status in ((0, 14, 0), (0, 15, -1), (0, -1, -1), (1, 15, 0), (1, 16, -1), (2, -100, 0), (2, base.F + 100, 0)):
        b = clone(base)
        n = int(b.count[c])
        if status == 0 and n > 1:
            b.hess[ff:ff + n - 1] = base.hess[base.ffirst[c]:base.ffirst[c] + n - 1]
        b.ffirst[c] = ff
        cases.append((c, ff, Call.explicit(b), status))
    return Call.explicit(base), cases


def ffirst_null_case(counts=(5, 3, 5, 1, 2)):
    """(the tile call, the call with first = c (G + 1) given and ffirst NULL): G = 5, so the factor rows of chain c start at
    first[c] - c = c G, which is neither the tile rule c (G - 1) nor first[c]; every row that is not used holds NaN."""
    G, Cn = 5, len(counts)
    src = Batch(list(counts), seed=3, prior_all=True)
    assert src.G == G
    first = np.arange(Cn, dtype=np.int64) * (G + 1)
    hess, prior = np.full((Cn * G, 496), np.nan), np.full((Cn * (G + 1), 136), np.nan)
    for c, n in enumerate(counts):
        prior[first[c]:first[c] + n] = src.prior[src.rows(c)]
        hess[first[c] - c:first[c] - c + max(n - 1, 0)] = src.chain(c)[0]
    b = Batch.from_arrays(list(counts), first, first - np.arange(Cn), hess, prior)
    return Call(src, count=src.count), Call(b, first=b.first, count=b.count)


def clamp_cases():
    """[(name, the call as given, the call with the values already clamped)] on the ragged chains with gaps: a negative first and
    count, a first beyond S, a G below the longest counts, an S that cuts the last chain in two.  The two calls of a case must agree
    in status and bit for bit, and rows of no clamped chain keep the sentinel."""
    b = Batch(RAGGED, seed=3, layout="gaps")
    cases = []
    raw, cl = clone(b), clone(b)
    raw.first[0], raw.count[0] = -5, -3
    cl.first[0], cl.count[0] = 0, 0
    cases.append(("negative first and count", Call.explicit(raw), Call.explicit(cl)))
    raw, cl = clone(b), clone(b)
    raw.first[9] = b.S + 7
    cl.first[9], cl.count[9] = b.S, 0
    cases.append(("first beyond S", Call.explicit(raw), Call.explicit(cl)))
    cl = clone(b)
    cl.count = np.minimum(b.count, 17).astype(np.int32)
    cases.append(("G = 17", Call.explicit(b, G=17), Call.explicit(cl)))
    cut = int(b.first[10]) + 1                                               # the last chain has two states: one is left
    assert b.count[10] == 2 and b.first[10] == b.first.max()
    cl = clone(b)
    cl.count[10] = 1
    cases.append(("S cuts the last chain", Call.explicit(b, S=cut), Call.explicit(cl)))
    return cases


LONG = [64, 1, 0, 2]                 # a trip count of 64 beside 1, 0 and 2: the carried registers of the short chains idle for 62 trips
EMPTY_WAVE = [0, 0, 0, 0, 3, 0, 2]   # a wavefront whose four chains have no states, next to one that has some
SCALED_EXPONENTS = (0, 300, -300, 301)


@functools.lru_cache(maxsize=None)
def long_case():
    """(batch, reference) of LONG: tile layout, the prior on the first state only (cond 1.6e10)."""
    b = Batch(LONG, seed=5)
    ref = Reference(b)
    ref.check_inputs()
    return b, ref


@functools.lru_cache(maxsize=None)
def scaled_reference():
    """(the unscaled batch, its reference).  scaled_batch(e) multiplies hess and prior by 2^e: A and g are scaled by a power of two,
    exactly, so delta is the unscaled one and this reference serves every exponent (cond 2.9e5)."""
    b = Batch(RAGGED, seed=3, prior_all=True)
    ref = Reference(b)
    ref.check_inputs()
    return b, ref


def scaled_batch(e):
    b = clone(scaled_reference()[0])
    b.hess *= 2.0 ** e
    b.prior *= 2.0 ** e
    return b


@functools.lru_cache(maxsize=None)
def empty_wave_case():
    b = Batch(EMPTY_WAVE, seed=3)
    ref = Reference(b)
    ref.check_inputs()
    return b, ref


def zero_pivot_case(diagonal):
    """(call, status): no prior, lambda = [0, 2, 2] on chains of 1, 1 and 2 states.  The block of a chain of one state is exactly
    zero: with lambda = 0 its first pivot is 0, and so it is under diagonal damping whatever lambda is (lambda * 0)."""
    b = Batch([1, 1, 2], seed=7)
    return Call(b, count=b.count, lam=[0.0, 2.0, 2.0], diagonal=diagonal, with_prior=False), ([1, 1, 0] if diagonal else [1, 0, 0])


@functools.lru_cache(maxsize=None)
def no_prior_diagonal_case():
    """(batch, lam, reference): no prior, diagonal damping 0.25 on chains of two states and more (cond 4.3e3)."""
    b = Batch([2, 3, 17, 40, 5, 16], seed=3)
    lam = lam_of(b, 0.25)
    ref = Reference(b, lam, True, with_prior=False)
    ref.check_inputs()
    return b, lam, ref
