"""CPU: the cases and references of tests/sqrt_info_cases.py on their own, before tests/test_gpu_sqrt_info_edges.py asks the device.

The float64 restatement of cpi_sqrt_info_kernel's factorisation is what a float64 implementation of this formulation achieves: its
errors against the long-double reference are the CPU column of profiles/sqrt_info_edges.md (pytest -s prints them)."""
import numpy as np
import pytest

from tests import sqrt_info_cases as sc

FAMILIES = ("realistic", "scaled", "graded", "exact")


@pytest.fixture(scope="module")
def fam():
    return sc.families()


@pytest.fixture(scope="module")
def rest(fam):
    return {n: sc.restatement(f.P) for n, f in fam.items()}


def test_every_case_is_exactly_symmetric(fam):
    npd = sc.not_pd()
    for name, P in [(n, f.P) for n, f in fam.items()] + [("twin", npd.twin)]:
        assert sc.bits_equal(P, np.swapaxes(P, -1, -2)), name
    bad, nan = npd.bad, np.isnan(npd.bad)
    assert np.array_equal(nan, np.swapaxes(nan, -1, -2)) and sc.bits_equal(np.where(nan, 0.0, bad), np.swapaxes(np.where(nan, 0.0, bad), -1, -2))
    assert sc.bits_equal(sc.packed_of(fam["scaled"].P), sc.dense_of(fam["scaled"].P)[:, sc.TRI])
    assert fam["realistic"].P.shape[0] == 64 and bad.shape[0] == 75 and npd.twin.shape[0] == 15


def test_every_case_outside_not_pd_is_positive_definite_and_none_is_excluded(fam, rest):
    excluded = 0
    for name in FAMILIES:
        R = rest[name]
        ok = np.isfinite(R).all(axis=(1, 2)) & (np.diagonal(R, axis1=1, axis2=2) > 0).all(axis=1)
        ok &= np.isfinite(sc.reference(name)).all(axis=(1, 2))
        excluded += int((~ok).sum())
        assert np.all(np.tril(R, -1) == 0.0), name
    Rt = sc.restatement(sc.not_pd().twin)
    excluded += int((~(np.isfinite(Rt).all(axis=(1, 2)) & (np.diagonal(Rt, axis1=1, axis2=2) > 0).all(axis=1))).sum())
    assert excluded == 0


def test_the_not_pd_pivot_is_the_diagonal_entry():
    """Row k is cut from the trailing block (so the reverse Cholesky's pivot k is P[k][k] as given) and stays coupled to the rows
    above it, which is what lets a failing pivot k reach rows 0 .. k - 1."""
    npd = sc.not_pd()
    for i in range(npd.bad.shape[0]):
        k, b = int(npd.pivot[i]), npd.bad[i]
        assert np.all(b[k, k + 1:] == 0.0) and np.all(b[k + 1:, k] == 0.0)
        assert k == 0 or np.all(b[k, :k] != 0.0)
        t = npd.twin[npd.twin_of[i]]
        off = ~np.eye(sc.N, dtype=bool)
        assert sc.bits_equal(b[off], t[off]) and t[k, k] > 0
    kinds = [(npd.bad[npd.of(3, n), 3, 3]) for n, _ in sc.KINDS]
    assert kinds[0] == -1.0 and kinds[1] == 0.0 and not np.signbit(kinds[1]) and kinds[2] == 0.0 and np.signbit(kinds[2])
    assert np.isnan(kinds[3]) and kinds[4] == np.inf


def test_the_longdouble_reference_on_its_own(fam):
    """R_ref rounded to float64 satisfies R P R^T = I to 1e-15 on the families whose gates rest on it (measured: 3.0e-16 and
    2.2e-16)."""
    for name in ("realistic", "scaled"):
        e = float(sc.e_id(sc.reference(name), fam[name].P).max())
        print("reference %-9s e_id %.2e" % (name, e))
        assert e < 1e-15, name


def test_restatement_floors_are_printed_per_family(fam, rest):
    """The CPU column of profiles/sqrt_info_edges.md.  The restatement is a float64 algorithm of the kernel's shape: on the
    well-conditioned families it must stay within the gate the device is held to (tests/tol.py)."""
    from tests.tol import REG_SQRT_INFO_EDGES
    print("\n%-10s %5s %10s %10s %10s | LAPACK %10s %10s" % ("family", "n", "e_row", "e_max", "e_id", "e_row", "e_id"))
    for name in FAMILIES:
        P, Rl, R = fam[name].P, sc.reference(name), rest[name]
        Rn = sc.lapack(P)
        have = np.isfinite(Rn).all(axis=(1, 2))
        print("%-10s %5d %10.2e %10.2e %10.2e | %17.2e %10.2e (%d of %d exist)" % (
            name, P.shape[0], sc.e_row(R, Rl).max(), sc.e_max(R, Rl).max(), sc.e_id(R, P).max(),
            sc.e_row(Rn[have], Rl[have]).max(), sc.e_id(Rn[have], P[have]).max(), have.sum(), have.size))
        if name != "graded":
            gate = REG_SQRT_INFO_EDGES[sc.GATE_OF[name]]
            assert sc.e_row(R, Rl).max() < gate["e_row"] and sc.e_id(R, P).max() < gate["e_id"], name
    g = fam["graded"]
    for c in sc.GRADES:
        s = g.cond == 10.0 ** c
        print("graded cond 1e%-2d e_row %10.2e e_id %10.2e" % (c, sc.e_row(rest["graded"], sc.reference("graded"))[s].max(),
                                                             sc.e_id(rest["graded"], g.P)[s].max()))
    rm = np.abs(sc.reference("scaled")).max(axis=2)
    print("scaled: rows of R differ by up to %.1e" % (rm.max(axis=1) / rm.min(axis=1)).max())
    assert (rm.max(axis=1) / rm.min(axis=1)).max() > 1e11


def test_restatement_reproduces_the_exact_expectations_bit_for_bit(rest):
    assert sc.exact_problems(rest["exact"]) == []
    # and the checker is not blind: one ulp on one entry of a scaled factor, a +0.0 for a -0.0 above a diagonal
    R = rest["exact"].copy()
    R[-1, 0, 3] = np.nextafter(R[-1, 0, 3], np.inf)
    R[1, 2, 5] = 0.0
    assert len(sc.exact_problems(R)) == 2


def test_restatement_produces_the_nan_pattern_of_every_failing_pivot():
    npd = sc.not_pd()
    Rt, Rb = sc.restatement(npd.twin), sc.restatement(npd.bad)
    bad = []
    for i in range(npd.bad.shape[0]):
        k = int(npd.pivot[i])
        bad += ["pivot %d %s: %s" % (k, npd.kind[i], p) for p in sc.nan_pattern_problems(Rb[i], Rt[npd.twin_of[i]], k)]
        assert int(np.isnan(Rb[i]).sum()) == sum(sc.N - r for r in range(k + 1))
    assert bad == []
    assert sc.expected_nan_pattern(0).sum() == 15 and sc.expected_nan_pattern(14).sum() == 120
    # not blind: a NaN row too many, a finite entry in a row that must be NaN, a twin row off by an ulp
    i = npd.of(7, "0.0")
    for r, c, v in ((8, 9, np.nan), (7, 12, 1.0), (9, 9, np.nextafter(Rb[i][9, 9], np.inf))):
        R = Rb[i].copy()
        R[r, c] = v
        assert sc.nan_pattern_problems(R, Rt[7], 7), (r, c)
    R = Rb[i].copy()
    R[10, 2] = -0.0
    assert sc.nan_pattern_problems(R, Rt[7], 7) and not sc.nan_pattern_problems(R, Rt[7], 7, dense=False)


def test_no_row_norm_regression(fam, rest):
    """A sanity bound on the metric, not a gate on a kernel: on `realistic` the row-wise error of the restatement is within 20 x its
    error relative to max |R| (measured: 3.2e-15 against 3.0e-16) -- the rows of R differ by 1.2e3 there, so a metric that were off by
    the row scale would show as a factor of a thousand."""
    Rl = sc.reference("realistic")
    row, mx = float(sc.e_row(rest["realistic"], Rl).max()), float(sc.e_max(rest["realistic"], Rl).max())
    print("realistic: e_row %.2e, relative to max |R| %.2e" % (row, mx))
    assert mx <= row <= 20.0 * mx
