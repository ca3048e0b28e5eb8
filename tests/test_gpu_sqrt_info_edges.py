"""GPU: cpi_sqrt_information_batch / _packed_batch (cpi_sqrt_info_kernel<PACKED>) at the edges of their contract, on the cases of
tests/sqrt_info_cases.py: realistic covariances with the edge cases in, badly scaled and badly conditioned matrices, matrices whose
R is known bit for bit, and every failing pivot of every kind.

The reference is the long-double factorisation (tests.tol.sqrt_info_longdouble).  The error is judged ROW BY ROW (e_row) and through
the identity R P R^T = I (e_id): relative to max |R| of the factor, as the older tests judge it, three quarters of a realistic R are
invisible.  No case is left out of any comparison (tests/test_sqrt_info_cpu.py).

Gates (tests/tol.py, profiles/sqrt_info_edges.md): `realistic`, `scaled` and `exact` at 100 x the floor measured on an MI355X, never
looser than 1e-12; `graded` per case at SQRT_INFO_GRADED_MULTIPLE x max(restatement, LAPACK's chol(inv(P))) -- what float64 baselines
achieve on that matrix against long double -- and, because LAPACK's route squares the condition number and is off by 1e-3 and more
from 1e8 up, also at SQRT_INFO_GRADED_MULTIPLE_RESTATEMENT x the restatement alone: the smaller of the two holds.  pytest -s prints
every figure before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import cpi_amd
from tests import sqrt_info_cases as sc
from tests.tol import REG_SQRT_INFO_EDGES, SQRT_INFO_GRADED_MULTIPLE, SQRT_INFO_GRADED_MULTIPLE_RESTATEMENT

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 29, 32, 33)      # 4-factor wavefronts at -1 / 0 / +1; 8 groups (one per XCD of the grid) at -1 / 0 / +1
SENTINEL = -7.0
UP = np.triu(np.ones((sc.N, sc.N), dtype=bool))


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _device(eng, P, packed):
    """R of P [F, 15, 15] by one call into a buffer one factor longer, pre-filled, whose last row must stay as it was.
    Returns [F, 15, 15] [row][col]; the packed form's entries under the diagonal do not exist and come back as +0.0."""
    F = P.shape[0]
    flat = sc.packed_of(P) if packed else sc.dense_of(P)
    big = torch.full((F + 1, flat.shape[1]), SENTINEL, dtype=torch.float64, device=eng.device)
    eng.sqrt_information(torch.from_numpy(flat).to(eng.device), out=big[:F])
    torch.cuda.synchronize()
    assert bool(torch.all(big[F:] == SENTINEL)), "written past F = %d (%s)" % (F, "packed" if packed else "dense")
    got = big[:F].cpu().numpy()
    return sc.from_packed(got) if packed else sc.from_dense(got)


def _both(eng, P):
    """Dense and packed, bit-identical in the triangle; the dense form's lower triangle is +0.0.  Returns the dense result."""
    Rd, Rp = _device(eng, P, False), _device(eng, P, True)
    assert sc.bits_equal(Rd[:, UP], Rp[:, UP]), "dense and packed differ"
    assert sc.bits_equal(Rd[:, ~UP], np.zeros_like(Rd[:, ~UP])), "the dense form does not store +0.0 below the diagonal"
    return Rd


@functools.lru_cache(maxsize=None)
def _family(eng, name):
    """The device's R of a whole family: computed once, shared, read-only."""
    R = _both(eng, sc.families()[name].P)
    R.setflags(write=False)
    return R


@pytest.mark.parametrize("name", ["realistic", "scaled", "graded", "exact"])
def test_every_family_against_long_double(eng, name):
    f = sc.families()[name]
    n, Rl = f.P.shape[0], sc.reference(name)
    R = _family(eng, name)
    assert np.isfinite(R).all() and (np.diagonal(R, axis1=1, axis2=2) > 0).all()
    for F in SIZES:                                   # the same rows whatever the size of the call (families shorter than 33 wrap)
        rows = np.arange(F) % n
        assert sc.bits_equal(_both(eng, f.P[rows]), R[rows]), F
    row, ident = sc.e_row(R, Rl), sc.e_id(R, f.P)
    print("\n%-10s n %d: e_row %.3e (%s), e_id %.3e (%s)" % (name, n, row.max(), f.label[int(row.argmax())], ident.max(),
                                                          f.label[int(ident.argmax())]))
    if name == "scaled":
        for i, s in enumerate(sc.SCALES):
            sl = slice(i * sc.PER_SCALE, (i + 1) * sc.PER_SCALE)
            print("  s %-2d e_row %.3e e_id %.3e" % (s, row[sl].max(), ident[sl].max()))
    if name != "graded":
        gate = REG_SQRT_INFO_EDGES[sc.GATE_OF[name]]
        assert gate["e_row"] <= 1e-12 and gate["e_id"] <= 1e-12
        assert row.max() < gate["e_row"] and ident.max() < gate["e_id"]
        return
    Rr = sc.restatement(f.P)
    rest = {"e_row": np.maximum(sc.e_row(Rr, Rl), sc.RATIO_FLOOR), "e_id": np.maximum(sc.e_id(Rr, f.P), sc.RATIO_FLOOR)}
    both = sc.baseline_errors(name)                   # max(restatement, LAPACK where it exists)
    assert SQRT_INFO_GRADED_MULTIPLE <= 100.0 and SQRT_INFO_GRADED_MULTIPLE_RESTATEMENT <= 100.0
    bad = []
    for metric, got in (("e_row", row), ("e_id", ident)):
        base = np.maximum(both[metric], sc.RATIO_FLOOR)
        gate = np.minimum(SQRT_INFO_GRADED_MULTIPLE * base, SQRT_INFO_GRADED_MULTIPLE_RESTATEMENT * rest[metric])
        for c in sc.GRADES:
            s = f.cond == 10.0 ** c
            print("  cond 1e%-2d %-5s device %.3e | restatement %.3e, worst ratio %5.2f | max(restatement, LAPACK) %.3e, worst ratio %5.2f | "
                  "closest to its gate %.3f" % (c, metric, got[s].max(), rest[metric][s].max(), (got / rest[metric])[s].max(),
                                                base[s].max(), (got / base)[s].max(), (got / gate)[s].max()))
        bad += ["%s %s: %.3e > %.3e" % (f.label[i], metric, got[i], gate[i]) for i in np.nonzero(~(got < gate))[0]]
    assert not bad, "; ".join(bad)


def test_results_known_bit_for_bit(eng):
    """The identity, diag(4^k) -> diag(2^-k), and P x 4^+-200 -> R x 2^-+200: binary scaling is exact while nothing leaves the normal
    range, in both forms."""
    P = sc.families()["exact"].P
    assert sc.exact_problems(_device(eng, P, False)) == []
    assert sc.exact_problems(_device(eng, P, True), below_is_zero=False) == []


def test_a_permutation_of_the_factors_permutes_the_rows(eng):
    P = np.concatenate([sc.families()["realistic"].P, sc.families()["scaled"].P])
    R = np.concatenate([_family(eng, "realistic"), _family(eng, "scaled")])
    perm = np.random.default_rng(78).permutation(P.shape[0])
    assert len(set((perm % 4 - np.arange(P.shape[0]) % 4) % 4)) == 4        # factors change their slot within the wavefront
    assert sc.bits_equal(_both(eng, P[perm]), R[perm])


def test_every_failing_pivot_of_every_kind(eng):
    """Pivot k = 0 .. 14 zero, -0.0, negative, NaN or +inf: rows 0 .. k of the triangle are NaN, every entry of them; rows k + 1 ..
    14 are the healthy twin's bit for bit; the dense form still stores +0.0 below the diagonal."""
    npd = sc.not_pd()
    for packed in (False, True):
        Rt, Rb = _device(eng, npd.twin, packed), _device(eng, npd.bad, packed)
        assert np.isfinite(Rt).all()
        bad = []
        for i in range(npd.bad.shape[0]):
            k = int(npd.pivot[i])
            bad += ["%s pivot %d %s: %s" % ("packed" if packed else "dense", k, npd.kind[i], p)
                    for p in sc.nan_pattern_problems(Rb[i], Rt[npd.twin_of[i]], k, dense=not packed)]
        assert not bad, "; ".join(bad)


def test_a_failing_pivot_touches_no_other_factor(eng):
    """A batch of 7 -- one full wavefront and a tail of 3 --, each slot of the wavefront and the last factor of the tail poisoned in
    turn with the first pivot taken (14) and the last (0), every kind: every other factor's R keeps its bits."""
    npd = sc.not_pd()
    base = np.array(sc.families()["scaled"].P[sc.SCALED_S6][:7])
    for packed in (False, True):
        clean = _device(eng, base, packed)
        for slot in (0, 1, 2, 3, 6):
            for k in (0, 14):
                for kind, _ in sc.KINDS:
                    P = base.copy()
                    P[slot] = npd.bad[npd.of(k, kind)]
                    R = _device(eng, P, packed)
                    others = np.arange(7) != slot
                    assert sc.bits_equal(R[others], clean[others]), (packed, slot, k, kind)
                    assert np.array_equal(np.isnan(R[slot])[UP], sc.expected_nan_pattern(k)[UP]), (packed, slot, k, kind)


@pytest.mark.parametrize("model", [1, 2])
def test_a_failing_pivot_reaches_the_cost_and_the_hessian(eng, model):
    """What a caller sees of a failing pivot: a genuine output of the kernel for pivot 0 (ONE row of NaNs), 7 and 14 in place of one
    factor's R gives that factor, and it alone, a NaN chi2 and a NaN f (entry 495 of its Hessian block), and a NaN total."""
    from tests.test_gpu_factor_edges import Inputs
    F = 5
    x = Inputs(eng, model, F)
    npd = sc.not_pd()
    for packed in (False, True):
        flat = sc.packed_of(npd.bad) if packed else sc.dense_of(npd.bad)
        Rbad = eng.sqrt_information(torch.from_numpy(flat).to(eng.device))
        good = x.Rt if packed else x.R
        clean = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, good, x.ii, x.jj)
        clean_h = eng.factor_hessian(model, x.meas, x.lin, x.q, x.states, good, x.ii, x.jj)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(clean["chi2"]).all()) and bool(torch.isfinite(clean_h).all())
        for n, k in enumerate((0, 7, 14)):
            f = (2 * n + 1) % F                       # factors 1, 3 and 0
            R = good.clone()
            R[f] = Rbad[npd.of(k, "-1")]
            assert int(torch.isnan(R[f]).sum()) == int(sc.expected_nan_pattern(k).sum())
            cost = eng.factor_cost(model, x.meas, x.lin, x.q, x.states, R, x.ii, x.jj)
            hess = eng.factor_hessian(model, x.meas, x.lin, x.q, x.states, R, x.ii, x.jj)
            torch.cuda.synchronize()
            assert torch.isnan(cost["chi2"]).nonzero().flatten().tolist() == [f], (packed, k)
            assert bool(torch.isnan(cost["total"]).all()), (packed, k)
            assert torch.isnan(hess[:, 495]).nonzero().flatten().tolist() == [f], (packed, k)
            keep = torch.arange(F, device=eng.device) != f
            assert torch.equal(cost["chi2"][keep], clean["chi2"][keep]) and torch.equal(hess[keep], clean_h[keep]), (packed, k)


@pytest.mark.parametrize("F", [1, 3, 4, 5, 9])
def test_in_place_gives_the_same_bits(eng, F):
    """sqrt_information(P, out=P): the kernel stages a wavefront's factors before it stores any of them."""
    P = sc.families()["scaled"].P[:F]
    for flat in (sc.dense_of(P), sc.packed_of(P)):
        d = torch.from_numpy(flat).to(eng.device)
        want = eng.sqrt_information(d)
        buf = d.clone()
        got = eng.sqrt_information(buf, out=buf)
        torch.cuda.synchronize()
        assert got.data_ptr() == buf.data_ptr() and torch.equal(got, want) and not torch.equal(want, d)


def test_partial_overlap_is_refused(eng):
    P = sc.families()["scaled"].P[:9]
    for flat, who in ((sc.dense_of(P), "cpi_sqrt_information_batch"), (sc.packed_of(P), "cpi_sqrt_information_packed_batch")):
        buf = torch.from_numpy(flat).to(eng.device)
        keep = buf.clone()
        for src, dst in ((buf[:8], buf[1:9]), (buf[1:9], buf[:8])):
            with pytest.raises(cpi_amd.CpiError, match="%s: .* overlaps" % who):
                eng.sqrt_information(src, out=dst)
        torch.cuda.synchronize()
        assert torch.equal(buf, keep)                 # refused before anything ran
        eng.sqrt_information(buf[:4], out=buf[4:8])   # adjacent, not overlapping: allowed
        torch.cuda.synchronize()
        assert torch.equal(buf[4:8], eng.sqrt_information(keep[:4]))
