"""Inputs, reference and metrics of the segment-condensation tests (cpi_chain_condense_batch / cpi_chain_expand_batch).  TEST
INFRASTRUCTURE ONLY.

Inputs: the chains of tests/chain_cases.py (imported, not edited).  Per segment length K in KS the counts
[0, 1, 2, 3, K, K + 1, K + 2, 2K, 2K + 1, 2K + 2] -- no interior and one interior, a tail segment of one factor, exact multiples, a chain
that is a single segment -- in the layouts "tile", "gaps" and "reverse"; MANY (chains of 5 and 6 segments at K = 2, so that segments of
different chains share a wavefront); LONG (one chain of 100 states at K = 12 beside short ones, the prior on every state and diagonal
lambda 1e-3: a prior on the first state alone gives cond 1.5e12 at 100 states, beyond the reference's own input condition).  Every
case runs the three dampings of cc.DAMPINGS with a lambda per chain and, without priors, identity damping 3.0 (a chain of one
state without a prior is exactly zero under diagonal damping).

Reference.  (1) The full chains' dense systems and their longdouble solutions: cc.Reference, unchanged.  (2) The definition of
include/cpi_amd.h restated in numpy longdouble, segment by segment (condense_longdouble): M = H_a, and per interior t
    D = M_tt + H_t[0:15, 0:15] + Pr_t + damping_t,   X = D^-1 [M_at^T  U_t  g]   (a longdouble Cholesky of D)
    M_aa -= M_at X_a;  M_a,t+1 = -M_at X_n;  M_t+1,t+1 = H_t[15:30, 15:30] - U_t^T X_n;  m_a -= M_at x_g;  m_t+1 = H_t[15:30, 30] - U_t^T x_g;
    c += H_t[30, 30] - g^T x_g
with damping_t = lambda or lambda diag(H_{t-1}[15:30, 15:30] + H_t[0:15, 0:15] + Pr_t), and the separators' prior rows.

Metrics (printed by the tests before anything is asserted):
    (a), (b)  of cc.Reference for the segmented delta, against the FULL chains' longdouble solution
    (r)  the reduced arrays alone: the reduced system they state is solved in LONGDOUBLE and its rows are compared with the full
         reference at the separators, |x_red - x_full|_inf / |x_full|_inf in units of cond_2(A) 2^-53 -- the error of rhess / rprior
         without that of the reduced solve
    (c)  a reduced factor row against (2): max_ij |M - ref|_ij / (d_i d_j), d_i = sqrt(ref_ii) for i < 30 and d_30 = sqrt(sum of the
         segment's H_t[30, 30]) (M is a Gram matrix: |M_ij| <= d_i d_j), in units of cond_2(D-system of the segment's interiors) 2^-53.
         A segment of one factor has no metric: it is compared bit for bit.
The separators' prior rows are one rounding from (2): off the diagonal the input's bits, on it within 2^-52 of the sum of magnitudes.

Gates = 100 x the floor (the rule of tests/tol.py); a floor is the largest value over every case, never below the rounding of the
format (2^-53 for (a); the other units already are cond 2^-53).  Measured against the longdouble reference
(profiles/chain_condense.md):
    host twin (tests/hostsim/hostsim_condense.cpp, x86-64, -ffp-contract=off)   (a) 7.5e-16  (b) 0.37  (r) 0.19  (c) 0.37
    device (MI355X)                                                            (a) 5.9e-16  (b) 0.40  (r) 0.24  (c) 0.86
((a): K = 7 without priors (host, device); (b), (r): K = 2 and K = 4 without priors, identity damping; (c): K = 4, identity damping.)
The largest cond_2(A) of these inputs is 1.9e8.  A reduced row with one entry off by 1e-6 shows (c) = 4.6e5.
"""
import functools

import numpy as np

from tests import chain_cases as cc

KS = (1, 2, 4, 7)
KINDS = ("tile", "gaps", "reverse")
SEED = 11

FLOOR_A_HOST, FLOOR_B_HOST, FLOOR_R_HOST, FLOOR_C_HOST = 7.5e-16, 0.37, 0.19, 0.37
FLOOR_A_DEVICE, FLOOR_B_DEVICE, FLOOR_R_DEVICE, FLOOR_C_DEVICE = 5.9e-16, 0.40, 0.24, 0.86
GATES_HOST = tuple(100 * v for v in (max(FLOOR_A_HOST, cc.EPS_HALF), FLOOR_B_HOST, FLOOR_R_HOST, FLOOR_C_HOST))
GATES_DEVICE = tuple(100 * v for v in (max(FLOOR_A_DEVICE, cc.EPS_HALF), FLOOR_B_DEVICE, FLOOR_R_DEVICE, FLOOR_C_DEVICE))


def counts_for(K):
    return [0, 1, 2, 3, K, K + 1, K + 2, 2 * K, 2 * K + 1, 2 * K + 2]


# name -> (counts, layout, K, prior on every state, the dampings it runs: (name, lambda or None, diagonal, with_prior))
_STD = tuple(cc.DAMPINGS) + (("identity_no_prior", 3.0, False),)
CASES = {}
for _K in KS:
    for _kind in KINDS:
        CASES["k%d_%s" % (_K, _kind)] = (counts_for(_K), _kind, _K, False, _STD)
CASES["many"] = ([12, 11, 13, 2, 12], "tile", 2, False, _STD)
CASES["long"] = ([3, 100, 1, 14], "tile", 12, True, (("diagonal_1e-3", 1e-3, True),))


def reduced_states(n, K):
    return (n - 2) // K + 2 if n >= 2 else n


def separators(n, K):
    """Chain-local indices of the states that stay."""
    return [min(j * K, n - 1) for j in range(reduced_states(n, K))] if n >= 2 else list(range(n))


def _chol_solve(D, B):
    """D [15, 15] symmetric positive definite, B [15, k] -> D^-1 B, in longdouble."""
    n = D.shape[0]
    L = np.zeros_like(D)
    for j in range(n):
        L[j, j] = np.sqrt(D[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (D[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.zeros_like(B)
    for j in range(n):
        Y[j] = (B[j] - L[j, :j] @ Y[:j]) / L[j, j]
    X = np.zeros_like(B)
    for j in range(n - 1, -1, -1):
        X[j] = (Y[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def _damp(D, raw, lam, diagonal):
    i = np.arange(15)
    D = D.copy()
    D[i, i] += lam * raw if diagonal else lam
    return D


def condense_longdouble(hess, prior, lam, diagonal, K):
    """One chain by the definition: hess [n - 1, 496], prior [n, 136] or None -> (rows: the m - 1 reduced factors [31, 31], priors: the m
    reduced prior rows [136], d30: per segment the square root of the summed constants) in longdouble."""
    n = hess.shape[0] + 1
    H = cc.unpack_sym(hess, 31)
    lam = np.longdouble(lam)
    if prior is not None:
        P = cc.unpack_sym(np.where(np.arange(136) == 135, 0.0, prior), 16)
    else:
        P = np.zeros((n, 16, 16), dtype=np.longdouble)
    seps = separators(n, K)
    rows, priors, d30 = [], [], []
    for s in seps:
        raw = (np.diagonal(H[s - 1][15:30, 15:30]) if s > 0 else 0) + (np.diagonal(H[s][:15, :15]) if s < n - 1 else 0) + np.diagonal(P[s][:15, :15])
        R = P[s].copy()
        R[:15, :15] = _damp(R[:15, :15], raw, lam, diagonal)
        priors.append(cc.pack_upper(R))
    for j in range(len(seps) - 1):
        a, b = seps[j], seps[j + 1]
        M = H[a].copy()
        const = H[a][30, 30]
        for t in range(a + 1, b):
            raw = np.diagonal(H[t - 1][15:30, 15:30]) + np.diagonal(H[t][:15, :15]) + np.diagonal(P[t][:15, :15])
            D = _damp(M[15:30, 15:30] + H[t][:15, :15] + P[t][:15, :15], raw, lam, diagonal)
            g = M[15:30, 30] + H[t][:15, 30] + P[t][:15, 15]
            Mat, U = M[:15, 15:30], H[t][:15, 15:30]
            X = _chol_solve(D, np.concatenate([Mat.T, U, g[:, None]], axis=1))
            Xa, Xn, xg = X[:, :15], X[:, 15:30], X[:, 30]
            N = np.zeros((31, 31), dtype=np.longdouble)
            N[:15, :15] = M[:15, :15] - Mat @ Xa
            N[:15, 15:30] = -Mat @ Xn
            N[15:30, :15] = N[:15, 15:30].T
            N[15:30, 15:30] = H[t][15:30, 15:30] - U.T @ Xn
            N[:15, 30] = N[30, :15] = M[:15, 30] - Mat @ xg
            N[15:30, 30] = N[30, 15:30] = H[t][15:30, 30] - U.T @ xg
            N[30, 30] = M[30, 30] + H[t][30, 30] - g @ xg
            const = const + H[t][30, 30]
            M = N
        rows.append(M)
        d30.append(np.sqrt(const))
    return rows, priors, d30


class Case:
    """One case under one damping: the batch, lambda per chain, the full chains' reference and the condensed reference."""

    def __init__(self, name, damping):
        counts, kind, K, prior_all, _ = CASES[name]
        dname, value, diagonal = damping
        self.name, self.K, self.diagonal = "%s/%s" % (name, dname), K, bool(diagonal)
        self.with_prior = not dname.endswith("no_prior")
        self.batch = b = cc.Batch(counts, seed=SEED, prior_all=prior_all, layout=kind)
        self.lam = cc.lam_of(b, value)
        self.full = cc.Reference(b, self.lam, self.diagonal, with_prior=self.with_prior)
        self.full.check_inputs()
        self.Gr = reduced_states(b.G, K)
        lam = np.zeros(b.C) if self.lam is None else self.lam
        self.rows, self.priors, self.d30, self.cond = {}, {}, {}, {}
        for c in range(b.C):
            n = int(b.count[c])
            if n == 0:
                continue
            hs, ps = b.chain(c)
            rows, priors, d30 = (condense_longdouble(hs, ps if self.with_prior else None, lam[c], self.diagonal, K) if n > 1 else
                                 ([], [None], []))
            if n == 1:                            # one state: its prior row, damped
                P = cc.unpack_sym(np.where(np.arange(136) == 135, 0.0, ps[0]), 16) if self.with_prior else np.zeros((16, 16), dtype=np.longdouble)
                P[:15, :15] = _damp(P[:15, :15], np.diagonal(P[:15, :15]).copy(), np.longdouble(lam[c]), self.diagonal)
                priors = [cc.pack_upper(P)]
            seps = separators(n, K)
            for j, M in enumerate(rows):
                self.rows[(c, j)], self.d30[(c, j)] = M, d30[j]
                lo, hi = 15 * (seps[j] + 1), 15 * seps[j + 1]
                self.cond[(c, j)] = np.linalg.cond(np.asarray(self.full.A[c][lo:hi, lo:hi], dtype=np.float64)) if hi > lo else 1.0
            for j, p in enumerate(priors):
                self.priors[(c, j)] = p

    def expected_rcount(self):
        return np.array([reduced_states(int(n), self.K) for n in self.batch.count], dtype=np.int32)

    def reduced_metric(self, rhess, rprior):
        """(r): the reduced system of the arrays solved in longdouble against the full reference at the separators."""
        b, worst = self.batch, 0.0
        for c in self.full.A:
            n = int(b.count[c])
            m = reduced_states(n, self.K)
            hs = rhess[c * (self.Gr - 1):c * (self.Gr - 1) + m - 1].reshape(1, m - 1, 496)
            ps = rprior[c * self.Gr:c * self.Gr + m].reshape(1, m, 136)
            if not (np.isfinite(hs).all() and np.isfinite(ps[..., :135]).all()):
                return np.inf
            A, g = cc.dense_system(hs, ps, np.zeros(1), False)
            x = cc.solve_longdouble(A, g)[0].reshape(m, 15)
            want = self.full.x[c].reshape(n, 15)[separators(n, self.K)]
            if not np.any(want):
                continue
            worst = max(worst, float(np.abs(x - want).max() / np.abs(self.full.x[c]).max()) / (self.full.cond[c] * cc.EPS_HALF))
        return worst

    def rows_metric(self, rhess):
        """(c) over every segment with an interior; a segment of one factor must be its hess row bit for bit (asserted here)."""
        b, worst = self.batch, 0.0
        for (c, j), ref in self.rows.items():
            got = rhess[c * (self.Gr - 1) + j]
            a = separators(int(b.count[c]), self.K)[j]
            if separators(int(b.count[c]), self.K)[j + 1] == a + 1:
                src = b.hess[b.ffirst[c] + a]
                assert np.array_equal(got.view(np.int64), src.view(np.int64)), (self.name, c, j)
                continue
            if not np.isfinite(got).all():
                return np.inf
            M = cc.unpack_sym(got, 31)
            d = np.sqrt(np.append(np.diagonal(ref)[:30], self.d30[(c, j)] ** 2))
            worst = max(worst, float((np.abs(M - ref) / (d[:, None] * d[None, :])).max()) / (self.cond[(c, j)] * cc.EPS_HALF))
        return worst

    def check_priors(self, rprior):
        """The separators' rows: entry 135 is 0.0, off the diagonal the input's bits, the diagonal one rounding from the definition."""
        b = self.batch
        diag = cc.tri(np.arange(15)) + np.arange(15)
        for (c, j), ref in self.priors.items():
            got = rprior[c * self.Gr + j]
            s = separators(int(b.count[c]), self.K)[j]
            src = b.prior[b.first[c] + s] if self.with_prior else np.zeros(136)
            off = np.ones(136, dtype=bool)
            off[diag] = False
            off[135] = False
            assert got[135] == 0.0 and np.array_equal(got[off], src[off]), (self.name, c, j)
            if self.lam is None:
                assert np.array_equal(got[diag], src[diag]), (self.name, c, j)
            else:
                refd = np.asarray(ref[diag], dtype=np.float64)
                assert (np.abs(got[diag] - ref[diag]) <= 2.0 ** -52 * (np.abs(src[diag]) + np.abs(refd))).all(), (self.name, c, j)

    def check(self, res, gates):
        """res: rhess, rprior, rcount, seg_status, status, delta of a run (numpy).  Prints, then asserts; returns the four metrics."""
        b = self.batch
        a_, b_ = self.full.metrics(res["delta"])
        r_ = self.reduced_metric(res["rhess"], res["rprior"])
        c_ = self.rows_metric(res["rhess"])
        print("%s: cond(A) max %.1e, (a) %.3e (b) %.3e (r) %.3e (c) %.3e" % (self.name, self.full.cond.max(), a_, b_, r_, c_))
        assert np.array_equal(res["rcount"], self.expected_rcount()), res["rcount"]
        assert (res["seg_status"] == 0).all() and (res["status"] == 0).all(), (res["seg_status"], res["status"])
        self.check_priors(res["rprior"])
        own = np.zeros(b.S, dtype=bool)
        for c in range(b.C):
            own[b.rows(c)] = True
        assert np.isfinite(res["delta"][own]).all() and (res["delta"][~own] == SENTINEL).all()
        assert a_ <= gates[0] and b_ <= gates[1] and r_ <= gates[2] and c_ <= gates[3], (a_, b_, r_, c_, gates)
        return a_, b_, r_, c_


SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def case(name, k):
    """Damping k of a case, computed once and shared: nobody changes it."""
    return Case(name, CASES[name][4][k])


def all_cases():
    return [(name, k) for name in CASES for k in range(len(CASES[name][4]))]


def failure_plan(K=4):
    """(batch, the batch with the block of interior state 5 of chain 1 made indefinite, K, chain, segment slot, the status it must give):
    chains of 10, 11 and 3 states with the prior on every state; state 5 lies inside the second segment (states 4 .. 8)."""
    good = cc.Batch([10, 11, 3, 6], seed=7, prior_all=True)
    bad = cc.clone(good)
    bad.prior[bad.first[1] + 5, cc.tri(7) + 7] = -1e12
    return good, bad, K, 1, 1, 6
