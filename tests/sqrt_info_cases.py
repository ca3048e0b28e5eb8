"""The square-root information at the edges of its contract: the cases and their references (CPU only).

cpi_sqrt_information_batch / _packed_batch compute R = chol_upper(P^-1) with cpi_sqrt_info_kernel<PACKED>
(cpi_amd/csrc/cpi_factor_kernels.hpp).  tests/test_sqrt_info_cpu.py checks the cases and the references below on their own;
tests/test_gpu_sqrt_info_edges.py asks the same of the device.

Every matrix is [row][col] and EXACTLY symmetric (the upper triangle mirrored): the dense kernel reads both triangles.

Families (families() -> {name: Family}):
  realistic  the oracle's P of synth.make_windows(16, N, seed=91, edge_cases=True), N = 1 and 50, models 1 and 2
  scaled     D C D, C = A A^T + 15 I, D = 10^uniform(-2 s / 3, s / 3), s = 0, 6, 12, 18: rows of R that differ by up to 1e12
  graded     Q diag(lambda) Q^T, lambda log-spaced over 10^0, 10^4, 10^8, 10^10: conditioning that no diagonal scaling removes
  exact      the identity, diag(4^k), and P beside 4^+-200 P for eight realistic factors: results known bit for bit
  not_pd     for every pivot k = 0 .. 14 and every kind of failing pivot (-1, 0.0, -0.0, NaN, +inf) a matrix whose reverse-Cholesky
             pivot k IS P[k][k], beside its healthy twin (not_pd() -> NotPd)

References: tests.tol.sqrt_info_longdouble (unchanged), restatement() -- float64 numpy in the kernel's own formulation, for the CPU
floors and the NaN pattern --, and lapack() = chol(inv(P)) as a second float64 baseline.
Metrics: e_row (row-wise relative error) and e_id (max |R P R^T - I| in long double on the float64 R)."""
import functools

import numpy as np

from tests.tol import sqrt_info_longdouble

N = 15
SEED = 20260
KINDS = (("-1", -1.0), ("0.0", 0.0), ("-0.0", -0.0), ("nan", float("nan")), ("+inf", float("inf")))
SCALES = (0, 6, 12, 18)
GRADES = (0, 4, 8, 10)
PER_SCALE = 12
PER_GRADE = 8
SCALED_S6 = slice(PER_SCALE, 2 * PER_SCALE)          # the s = 6 block of `scaled`: the bases of not_pd
EXACT_SHIFT = 200
GATE_OF = {"realistic": "realistic", "scaled": "scaled", "exact": "realistic"}   # family -> the gate of tests/tol.py it is held to
RATIO_FLOOR = 2.0 ** -52     # no float64 result is judged more finely than an ulp of its row's largest entry (graded: cond 1)

# column-major dense [225] <-> packed upper triangle [120] (CPI_TRI_INDEX: entry (r, c), r <= c, at r + c (c + 1) / 2)
TRI = np.array([c * N + r for c in range(N) for r in range(c + 1)])


def mirror(P):
    """Exactly symmetric: the upper triangle of [.., 15, 15], mirrored."""
    P = np.asarray(P, dtype=np.float64)
    return np.triu(P) + np.swapaxes(np.triu(P, 1), -1, -2)


def dense_of(P):
    """[F, 15, 15] -> [F, 225] column-major (what cpi_sqrt_information_batch reads)."""
    return np.ascontiguousarray(np.swapaxes(P, -1, -2).reshape(-1, N * N))


def packed_of(P):
    """[F, 15, 15] -> [F, 120], the packed upper triangle (what cpi_sqrt_information_packed_batch reads)."""
    return np.ascontiguousarray(dense_of(P)[:, TRI])


def from_dense(R):
    """[F, 225] column-major -> [F, 15, 15] [row][col]."""
    return np.swapaxes(np.asarray(R).reshape(-1, N, N), -1, -2)


def from_packed(Rt, below=0.0):
    """[F, 120] -> [F, 15, 15] [row][col], `below` under the diagonal."""
    Rt = np.asarray(Rt)
    flat = np.full((Rt.shape[0], N * N), below, dtype=np.float64)
    flat[:, TRI] = Rt
    return from_dense(flat)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


class Family:
    """P [n, 15, 15]; label [n] says where a case comes from; cond [n] for `graded` (the condition number it was built with)."""

    def __init__(self, P, label, cond=None):
        self.P, self.label, self.cond = P, list(label), cond
        self.P.setflags(write=False)
        assert self.P.shape == (len(self.label), N, N)


# ------------------------------------------------------------------------------------------------ references
def pivot_rsqrt(a):
    """1 / sqrt(a) by the kernel's route (inv_sqrt_unclamped of cpi_math.hpp): a reciprocal-square-root seed -- NaN for a < 0, +inf
    for +0, -inf for -0, 0 for +inf -- and its Newton sequence, in which 0 x inf = NaN carries every one of those to the result.
    float64 without fused multiply-adds: within an ulp or two for a normal a > 0, and exact under a -> 4^k a."""
    with np.errstate(all="ignore"):
        y = 1.0 / np.sqrt(a)
        g, h = a * y, 0.5 * y
        r = 0.5 - h * g
        g, h = g + g * r, h + h * r
        d = a - g * g
        g = g + d * h
        r = 0.5 - h * g
        h = h + h * r
        return 2.0 * h


def restatement(P):
    """The kernel's factorisation in float64 numpy, vectorised over the batch: reverse Cholesky with the inverse folded in, "lane" j
    holding column j of the working matrix, running sums started at -[i == j], u[k] = -acc[k] * inv, the trailing updates taking
    column k of lane k as they do on the device (chol_inv_step).  Products and sums are rounded separately where the device fuses
    them.  Returns R [F, 15, 15] [row][col] with +0.0 below the diagonal, NaNs where a pivot failed."""
    A = np.array(P, dtype=np.float64)                    # A[f, i, j]: register a[i] of lane j
    F = A.shape[0]
    acc = np.tile(-np.eye(N), (F, 1, 1))
    u = np.zeros((F, N, N))
    with np.errstate(all="ignore"):
        for k in range(N - 1, -1, -1):
            inv = pivot_rsqrt(A[:, k, k])[:, None]
            u[:, k, :] = -acc[:, k, :] * inv
            ca, cu = -inv * (A[:, k, :] * inv), inv * u[:, k, :]
            col = A[:, :k, k].copy()                     # lane k's column, as every lane reads it
            acc[:, :k, :] += col[:, :, None] * cu[:, None, :]
            A[:, :k, :] += col[:, :, None] * ca[:, None, :]
    return np.where(np.triu(np.ones((N, N), dtype=bool)), u, 0.0)


def lapack(P):
    """chol(inv(P)) through LAPACK, transposed to the upper factor: the second float64 baseline.  Where the float64 inverse is no
    longer positive definite (condition numbers from about 1e9 up) LAPACK refuses it and the factor's R is all NaN: this baseline
    does not exist there."""
    out = []
    for p in np.asarray(P):
        try:
            out.append(np.linalg.cholesky(np.linalg.inv(p)).T)
        except np.linalg.LinAlgError:
            out.append(np.full((N, N), np.nan))
    return np.stack(out)


def baseline_errors(name):
    """{"e_row": [n], "e_id": [n]}: per case the larger of the two float64 baselines' errors (restatement, LAPACK where it exists)
    against the long-double reference -- what a float64 algorithm achieves on that matrix."""
    P, Rl = families()[name].P, reference(name)
    Rr, Rn = restatement(P), lapack(P)
    have = np.isfinite(Rn).all(axis=(1, 2))
    Rn = np.where(have[:, None, None], Rn, Rr)
    return {"e_row": np.maximum(e_row(Rr, Rl), e_row(Rn, Rl)), "e_id": np.maximum(e_id(Rr, P), e_id(Rn, P)), "lapack_exists": have}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The long-double R of a family, rounded to float64 -- computed once, shared, read-only."""
    R = sqrt_info_longdouble(families()[name].P)
    R.setflags(write=False)
    return R


def e_row(R, Rref):
    """[F]: max over rows k of max_j |R - Rref|[k][j] / max_j |Rref[k][j]|.  A NaN in R counts as inf."""
    d = np.abs(np.asarray(R) - Rref)
    d = np.where(np.isnan(d), np.inf, d)
    return (d.max(axis=2) / np.abs(Rref).max(axis=2)).max(axis=1)


def e_max(R, Rref):
    """[F]: max |R - Rref| / max |Rref| of the factor -- the norm the older tests use."""
    d = np.abs(np.asarray(R) - Rref)
    d = np.where(np.isnan(d), np.inf, d)
    return d.max(axis=(1, 2)) / np.abs(Rref).max(axis=(1, 2))


def e_id(R, P):
    """[F]: max |R P R^T - I|, evaluated in long double on the float64 R."""
    Rl, Pl = np.array(R, dtype=np.longdouble), np.array(P, dtype=np.longdouble)
    d = np.abs(Rl @ Pl @ np.swapaxes(Rl, -1, -2) - np.eye(N))
    d = np.where(np.isnan(d), np.inf, d)
    return np.asarray(d.max(axis=(1, 2)), dtype=np.float64)


# ------------------------------------------------------------------------------------------------ families
def _realistic():
    from cpi_amd import synth
    from oracle import oracle_py as op
    Ps, label = [], []
    for n in (1, 50):
        kn, lin, q = (t.numpy() for t in synth.make_windows(16, n, seed=91, edge_cases=True))
        for model in (1, 2):
            out = op.oracle().run(op.make_params(model), kn, lin, q if model == 2 else None)
            Ps.append(mirror(from_dense(out["P"])))
            label += ["N %d model %d window %d" % (n, model, w) for w in range(16)]
    return Family(np.concatenate(Ps), label)


def _scaled():
    rng = np.random.default_rng(SEED + 1)
    Ps, label = [], []
    for s in SCALES:
        A = rng.standard_normal((PER_SCALE, N, N))
        C = A @ np.swapaxes(A, -1, -2) + 15.0 * np.eye(N)
        D = 10.0 ** rng.uniform(-2.0 * s / 3.0, s / 3.0, (PER_SCALE, N))
        Ps.append(mirror(D[:, :, None] * C * D[:, None, :]))
        label += ["s %d #%d" % (s, i) for i in range(PER_SCALE)]
    return Family(np.concatenate(Ps), label)


def _graded():
    rng = np.random.default_rng(SEED + 2)
    Ps, label, cond = [], [], []
    for c in GRADES:
        Q = np.linalg.qr(rng.standard_normal((PER_GRADE, N, N)))[0]
        lam = 10.0 ** np.linspace(0.0, float(c), N)
        Ps.append(mirror((Q * lam) @ np.swapaxes(Q, -1, -2)))
        label += ["cond 1e%d #%d" % (c, i) for i in range(PER_GRADE)]
        cond += [10.0 ** c] * PER_GRADE
    return Family(np.concatenate(Ps), label, np.array(cond))


EXACT_REAL = (0, 5, 17, 22, 33, 40, 51, 63)          # rows of `realistic`: both N, both models


@functools.lru_cache(maxsize=None)
def _exact_parts():
    """P [n, 15, 15], labels, and what is known of R: `want` [n, 15, 15] (NaN where nothing is fixed), and `pair` [n]: the row whose R,
    times `factor` [n] (a power of two), this row's R must equal bit for bit (-1: none)."""
    rng = np.random.default_rng(SEED + 3)
    Ps, label, want, pair, factor = [np.eye(N)], ["identity"], [diag_expectation(np.zeros(N, dtype=int))], [-1], [1.0]
    ks = [np.full(N, k) for k in (-200, -37, -1, 1, 64, 200)] + [rng.integers(-200, 201, N) for _ in range(5)]
    ks.append(np.array([200, -200] * 7 + [200]))
    for k in ks:
        Ps.append(np.diag(4.0 ** k.astype(np.float64)))
        label.append("diag(4^k), k = %d .. %d" % (k.min(), k.max()))
        want.append(diag_expectation(k)); pair.append(-1); factor.append(1.0)
    real = families_cached("realistic").P[list(EXACT_REAL)]
    base = len(Ps)
    for i, p in enumerate(real):
        Ps.append(p); label.append("realistic %d" % EXACT_REAL[i])
        want.append(np.full((N, N), np.nan)); pair.append(-1); factor.append(1.0)
    for sign in (+1, -1):
        for i, p in enumerate(real):
            Ps.append(p * 4.0 ** (sign * EXACT_SHIFT)); label.append("realistic %d x 4^%+d" % (EXACT_REAL[i], sign * EXACT_SHIFT))
            want.append(np.full((N, N), np.nan)); pair.append(base + i); factor.append(2.0 ** (-sign * EXACT_SHIFT))
    return np.stack(Ps), label, np.stack(want), np.array(pair), np.array(factor)


def diag_expectation(k):
    """R of diag(4^k): diag(2^-k) -- and, bit for bit, -0.0 above the diagonal (u[k] = -acc[k] * inv with a running sum that is still
    +0.0) and +0.0 below it."""
    R = np.where(np.triu(np.ones((N, N), dtype=bool), 1), -0.0, 0.0)
    R[np.arange(N), np.arange(N)] = 2.0 ** (-np.asarray(k, dtype=np.float64))
    return R


def exact_problems(R, below_is_zero=True):
    """What of the `exact` family's expectations a result R [n, 15, 15] misses (a list of texts; empty: all hold bit for bit).
    below_is_zero=False: R comes from the packed form, whose entries under the diagonal do not exist."""
    P, label, want, pair, factor = _exact_parts()
    up = np.triu(np.ones((N, N), dtype=bool))
    sel = up if not below_is_zero else np.ones((N, N), dtype=bool)
    bad = []
    for i in range(P.shape[0]):
        if not np.isnan(want[i]).any() and not bits_equal(R[i][sel], want[i][sel]):
            bad.append("%s: not diag(2^-k) bit for bit" % label[i])
        if pair[i] >= 0:
            if not (np.isfinite(R[i]).all() and bits_equal(R[i][up], (R[pair[i]] * factor[i])[up])):
                bad.append("%s: not its base's R x 2^%d bit for bit" % (label[i], int(np.log2(factor[i]))))
    return bad


def _exact():
    P, label = _exact_parts()[:2]
    return Family(mirror(P), label)


class NotPd:
    """bad [75, 15, 15] (pivot[i] = k fails, kind[i] names how), twin_of[i] indexes twin [15, 15, 15]: the same matrix with its
    positive pivot."""

    def __init__(self):
        base = families_cached("scaled").P[SCALED_S6]
        twin, bad, self.pivot, self.kind, self.twin_of = [], [], [], [], []
        for k in range(N):
            t = np.array(base[k % base.shape[0]])
            t[k, k + 1:] = 0.0                           # pivot k of the reverse Cholesky is now P[k][k] itself; rows < k stay coupled
            t[k + 1:, k] = 0.0
            twin.append(t)
            for name, v in KINDS:
                b = t.copy()
                b[k, k] = v
                bad.append(b); self.pivot.append(k); self.kind.append(name); self.twin_of.append(k)
        self.twin, self.bad = np.stack(twin), np.stack(bad)
        self.pivot, self.twin_of = np.array(self.pivot), np.array(self.twin_of)
        self.twin.setflags(write=False); self.bad.setflags(write=False)

    def of(self, k, kind):
        return int(np.nonzero((self.pivot == k) & (np.array(self.kind) == kind))[0][0])


@functools.lru_cache(maxsize=None)
def families_cached(name):
    return {"realistic": _realistic, "scaled": _scaled, "graded": _graded, "exact": _exact}[name]()


def families():
    return {n: families_cached(n) for n in ("realistic", "scaled", "graded", "exact")}


@functools.lru_cache(maxsize=None)
def not_pd():
    return NotPd()


# ------------------------------------------------------------------------------------------------ the failing-pivot rule
def expected_nan_pattern(k):
    """[15, 15] bool, [row][col]: the entries of R that are NaN when pivot k fails -- rows 0 .. k of the upper triangle.  (Pivot k
    failing makes 1 / b_kk NaN; row k of U is -acc[k] x NaN in every lane; ca / cu carry the NaN into every row above.  Rows k + 1
    .. 14 were finished before and depend on the trailing block alone: they are the healthy twin's.  Under the diagonal the dense
    form stores +0.0.)"""
    up = np.triu(np.ones((N, N), dtype=bool))
    up[k + 1:] = False
    return up


def nan_pattern_problems(R, twin, k, dense=True):
    """What R [15, 15] of a matrix whose pivot k fails misses of the rule, given the healthy twin's R (a list of texts)."""
    up = np.triu(np.ones((N, N), dtype=bool))
    want = expected_nan_pattern(k)
    bad = []
    if not np.array_equal(np.isnan(R)[up], want[up]):
        bad.append("NaN in %d entries of the triangle, expected rows 0 .. %d = %d" % (np.isnan(R)[up].sum(), k, want.sum()))
    if not bits_equal(R[k + 1:][up[k + 1:]], twin[k + 1:][up[k + 1:]]):
        bad.append("rows %d .. 14 are not the healthy twin's bit for bit" % (k + 1))
    if dense and not bits_equal(R[~up], np.zeros((~up).sum())):
        bad.append("not +0.0 below the diagonal")
    return bad
