"""CPU-only checks of resumable preintegration (cpi_preintegrate_resume): the carry-record sizes, the argument checks that
run before any device work, the facades' incremental-mode rules and the carry kernels' place in the build report."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def test_carry_doubles(lib):
    assert lib.cpi_carry_doubles(1) == 288
    assert lib.cpi_carry_doubles(2) == 566
    assert lib.cpi_carry_doubles(3) == 0          # CPI_MODEL_FORSTER cannot be resumed
    assert lib.cpi_carry_doubles(0) == 0
    assert lib.cpi_carry_doubles(-1) == 0


def test_resume_rejects_invalid_calls_without_a_context(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, out = CpiParams(), CpiOutputs()
    assert lib.cpi_preintegrate_resume(None, C.byref(prm), 1, 1, None, None, None, None, None, None, None, C.byref(out)) == 1


def test_python_mirror_incremental_rules():
    import cpi_amd
    v1 = cpi_amd.CpiV1(0.005, 4e-6, 0.01, 2e-4)
    v1.set_incremental(True)
    v1.setLinearizationPoints(np.zeros(3), np.zeros(3))   # allowed until a segment was computed
    v1.feed_IMU(0.0, 0.005, np.zeros(3), np.zeros(3))
    with pytest.raises(RuntimeError):
        v1.set_incremental(False)                         # only before the first feed_IMU
    with pytest.raises(ValueError):
        cpi_amd.ForsterDiscrete(0.005, 4e-6, 0.01, 2e-4).set_incremental(True)


def test_carry_kernels_are_in_the_resource_report():
    """The batch kernels keep their rows; the carry path adds its own kernels (never a template argument of cpi_mean_kernel)."""
    from cpi_amd import build
    rows = [ln.split(">")[0] for ln in open(build.REPORT) if ln.startswith("cpi_mean_kernel<")]
    names = " ".join(open(build.REPORT).read().split("\n"))
    assert "cpi_mean_carry_kernel<1, true, false, 1>" in names and "cpi_mean_carry_kernel<2, false, true, 64>" in names
    assert "cpi_cov_carry_kernel<2, true>" in names and "cpi_cov_carry_kernel<1, false>" in names
    assert rows and all(r.count(",") == 5 for r in rows)   # <MODEL, JAC, AVG, L, CUT, BIG>: unchanged
