"""Parity gates (BASELINE.json north_star; SURVEY.md section 8(d) 'Parity gates')."""
import numpy as np

TOL_MEAN = 1e-9      # alpha, beta, q, R, DT : max-abs
TOL_COV = 1e-6       # |dP_ij| <= TOL_COV * sqrt(P_ii P_jj)
TOL_JAC = 1e-8       # bias / orientation Jacobians: max-abs (our choice; north_star is silent)
TOL_FACTOR = 1e-9    # evaluateError residual and H1/H2 : max-abs

# Regression gates = 100 x the floor measured on MI355X against the COMPILED REFERENCE (means
# 2e-15, covariance 2e-15 relative, Jacobians 3e-13 -- the last is the reference's own cancellation noise in f2 / df
# just above its 0.008726646 rad/s threshold).  The contractual gates above say "parity"; these say "nothing moved":
# a kernel change that shifts a result by 1e-10 passes the former and must not pass silently.  They apply wherever the
# expected values come from the compiled reference (golden fixtures, oracle/_ref on the GPU box) on realistic inputs;
# stress tests with scaled inputs keep the contractual gates relative to the magnitude of the quantity.
REG_MEAN = 2e-13
REG_COV = 2e-13
REG_JAC = 3e-11
REG_FACTOR = 1e-12   # evaluateError on the golden cases vs the restatement (measured floor 2e-14 on O(10) entries in round 2; 2.7e-15 on the
                     # 256 golden cases with round 6's reciprocal quaternion normalisation: tests/tools/measure_factor_floor.py)
# SURVEY 8(f) rows (round 3; floors measured on MI355X with tests/tools/measure_floors.py, gates = ~100 x):
#   f4 Forster comparator, HIP (sparse, permuted, one exchange) vs the dense restatement oracle/forster_oracle.c on the
#      golden + seeded inputs: means <= 8.9e-15, bias Jacobians <= 2.9e-15, covariance <= 9.7e-15 relative
#   f1 square-root information on the realistic covariances (cond ~1e8), HIP vs the longdouble restatement
#      (sqrt_info_longdouble below), relative to max |R| of the factor: 3.5e-16 (LAPACK's own f64 result: 2.3e-16)
REG_FORSTER_MEAN = 1e-12
REG_FORSTER_JAC = 3e-13
REG_FORSTER_COV = 1e-12
REG_SQRT_INFO = 5e-14
# The same factorisation judged ROW BY ROW (tests/sqrt_info_cases.py: e_row = max_k max_j |R - R_ref|[k][j] / max_j |R_ref[k][j]|, and
# e_id = max |R P R^T - I| in long double) -- relative to max |R| of the factor, rows 0-2 of a realistic R (4e2 .. 8e2 against 5e5 in
# rows 3-5) could be wrong by 6e-11 of themselves under REG_SQRT_INFO.  Floors on MI355X against the long-double reference
# (profiles/sqrt_info_edges.md; the float64 restatement on the CPU beside them), gates = 100 x, never looser than 1e-12:
#   realistic (the oracle's P, N = 1 and 50, edge cases in)        e_row 6.409e-15 (CPU 3.22e-15)   e_id 4.122e-15 (CPU 2.15e-15)
#   scaled    (D C D, rows of R differing by up to 3.5e17)         e_row 9.524e-15 (CPU 4.19e-15)   e_id 3.401e-15 (CPU 5.57e-16)
# (the `exact` family -- realistic factors x 4^+-200 and diagonal matrices -- is held to the realistic gate: 3.3e-15, 2.0e-15)
REG_SQRT_INFO_EDGES = {"realistic": {"e_row": 6.409e-13, "e_id": 4.122e-13},
                       "scaled": {"e_row": 9.524e-13, "e_id": 3.401e-13}}
REG_SQRT_INFO_ROW = REG_SQRT_INFO_EDGES["realistic"]["e_row"]
# `graded` (condition numbers 1 .. 1e10: forward error grows with the condition number for any float64 algorithm): the gate is per
# case, a multiple of what float64 baselines achieve on that matrix against long double, each floored at 2^-52.  Two baselines, and
# the smaller gate holds:
#   max(restatement, LAPACK's chol(inv(P)))   worst device / baseline ratio on MI355X 1.98  -> multiple 10 x 1.98 = 20
#   the restatement alone                     worst ratio 10.15 (e_id, cond 1e4)           -> 10 x 10.15, capped at 100
# The second is there because chol(inv(P)) squares the condition number: from 1e8 up its own error is 1e-3 and more, and a multiple
# of it would hold nothing.
SQRT_INFO_GRADED_MULTIPLE = 20.0
SQRT_INFO_GRADED_MULTIPLE_RESTATEMENT = 100.0


def cov_rel_err(P, Pref):
    """max_ij |P-Pref|_ij / sqrt(Pref_ii Pref_jj) over a batch of column-major 15x15."""
    P = np.asarray(P).reshape(-1, 15, 15)
    Pref = np.asarray(Pref).reshape(-1, 15, 15)
    d = np.sqrt(np.abs(np.diagonal(Pref, axis1=1, axis2=2)))
    den = d[:, :, None] * d[:, None, :]
    den = np.where(den > 0, den, np.inf)
    rel = np.abs(P - Pref) / den
    # entries whose scale is exactly zero must be exactly (abs 1e-30) zero
    zero_scale = ~np.isfinite(den)
    assert np.all(np.abs((P - Pref)[zero_scale]) < 1e-30)
    return float(rel.max())


def check_pre(out, ref, what=("mean", "jac", "cov"), v2=False, label="", regression=False):
    """regression=True: the expected values come from the compiled reference on realistic inputs -- apply the
    regression gates (100 x the measured floor) instead of the contractual ones.  regression="forster": the Forster
    comparator against its restatement (its own measured floor)."""
    tol_mean, tol_jac, tol_cov = (REG_MEAN, REG_JAC, REG_COV) if regression else (TOL_MEAN, TOL_JAC, TOL_COV)
    if regression == "forster":
        tol_mean, tol_jac, tol_cov = REG_FORSTER_MEAN, REG_FORSTER_JAC, REG_FORSTER_COV
    msgs = []
    if "mean" in what:
        for k in ("DT", "alpha", "beta", "q"):
            e = float(np.abs(np.asarray(out[k]) - np.asarray(ref[k])).max())
            if not e <= tol_mean:
                msgs.append("%s %s err %.3e" % (label, k, e))
    if "jac" in what:
        for k in ("J_q", "J_a", "J_b", "H_a", "H_b") + (("O_a", "O_b") if v2 else ()):
            e = float(np.abs(np.asarray(out[k]) - np.asarray(ref[k])).max())
            if not e <= tol_jac:
                msgs.append("%s %s err %.3e" % (label, k, e))
    if "cov" in what:
        e = cov_rel_err(out["P"], ref["P"])
        if not e <= tol_cov:
            msgs.append("%s P rel err %.3e" % (label, e))
    assert not msgs, "; ".join(msgs)


def sqrt_info_longdouble(P):
    """R = chol_upper(P^-1) = B^-1 with P = B B^T, B upper triangular, in numpy longdouble (x87: 64-bit mantissa), vectorised
    over the batch: the best available reference for GTSAM's Gaussian::Covariance -> Information(P^-1) -> LLT::matrixU on
    the realistic covariances, whose condition numbers (~1e8) put LAPACK's own f64 result ~1e-9 away from the true R.
    P [F, 15, 15] -> R [F, 15, 15] (float64, [row][col])."""
    A = np.array(P, dtype=np.longdouble)
    F, n = A.shape[0], A.shape[1]
    B = np.zeros_like(A)
    for k in range(n - 1, -1, -1):                  # reverse Cholesky: P = B B^T, B upper triangular
        B[:, k, k] = np.sqrt(A[:, k, k])
        B[:, :k, k] = A[:, :k, k] / B[:, k, k][:, None]
        A[:, :k, :k] -= B[:, :k, k][:, :, None] * B[:, :k, k][:, None, :]
    U = np.zeros_like(B)                            # U = B^-1 (upper triangular), by back substitution
    for j in range(n):
        U[:, j, j] = 1 / B[:, j, j]
        for i in range(j - 1, -1, -1):
            U[:, i, j] = -(B[:, i, i + 1:j + 1] * U[:, i + 1:j + 1, j]).sum(axis=1) / B[:, i, i]
    return np.asarray(U, dtype=np.float64)


# ---- per-field regression gates (tests/test_gpu_stj_edges.py, tests/test_hostsim_stj.py; profiles/stj_edges.md)
# A floor is the largest error of one field measured against the oracle, never below the rounding of the field itself
# (2^-53 x max |ref|); the gate is 100 x the floor and never looser than the contractual gate of the field's group.
EPS_HALF = 2.0 ** -53
MEAN_FIELDS = ("DT", "alpha", "beta", "q")


def contract_gate(field):
    return TOL_MEAN if field in MEAN_FIELDS else (TOL_COV if field == "P" else TOL_JAC)


def field_gates(floors):
    """{field: floor} -> {field: gate}."""
    return {k: min(contract_gate(k), 100.0 * f) for k, f in floors.items()}


class FieldTable:
    """Largest error per field over the comparisons of a test, the rounding floor of the reference beside it, and where the largest
    error sits -- printed before anything is asserted, so that a failure shows the oracle's margin first."""

    def __init__(self, fields):
        self.fields = tuple(fields)
        self.err = {k: 0.0 for k in self.fields}
        self.ulp = {k: 0.0 for k in self.fields}
        self.where = {k: "" for k in self.fields}

    def add(self, got, ref, label=""):
        for k in self.fields:
            g, r = np.asarray(got[k]), np.asarray(ref[k])
            assert g.shape == r.shape, (label, k, g.shape, r.shape)
            assert np.isfinite(r).all(), (label, k, "the reference is not finite")
            if k == "P":
                e, at, u = (cov_rel_err(g, r) if np.isfinite(g).all() else np.inf), "", EPS_HALF
            else:
                d = np.abs(g - r)
                d = np.where(np.isnan(d), np.inf, d)               # a row that was not written fails
                e = float(d.max()) if d.size else 0.0
                at = " at %s (ref %.3g)" % (tuple(int(i) for i in np.unravel_index(int(d.argmax()), d.shape)), r.flat[int(d.argmax())]) if d.size else ""
                u = EPS_HALF * float(np.abs(r).max()) if r.size else 0.0
            self.ulp[k] = max(self.ulp[k], u)
            if e >= self.err[k]:
                self.err[k], self.where[k] = e, "%s%s" % (label, at)

    def floors(self):
        return {k: max(self.err[k], self.ulp[k]) for k in self.fields}

    def report(self, title, gates=None):
        print("%s" % title)
        print("| field | largest error | 2^-53 max abs ref | floor | gate | worst |")
        print("|---|---|---|---|---|---|")
        for k in self.fields:
            print("| `%s` | %.2e | %.2e | %.2e | %s | %s |" % (k, self.err[k], self.ulp[k], self.floors()[k],
                                                           "%.2e" % gates[k] if gates else "-", self.where[k]))

    def check(self, gates, title):
        bad = ["%s %.3e > %.2e (%s)" % (k, self.err[k], gates[k], self.where[k]) for k in self.fields if not self.err[k] <= gates[k]]
        assert not bad, title + ": " + "; ".join(bad)
