"""CPU-only checks of running preintegration (cpi_preintegrate_running): the symbols are declared and exported within ABI 3,
the Python layer knows them, the calls that can be refused without a context are refused, and the new kernels stand in the
build report beside the unchanged batch kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_preintegrate_running", "cpi_preintegrate_running_host")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def test_running_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "cpi_amd.h")).read()
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int
    assert lib.cpi_abi_version() == 3
    assert "cpi_preintegrate_running, cpi_preintegrate_running_host" in header.split("typedef struct cpi_ctx")[0]   # "additions within 3"


def test_running_rejects_a_null_context(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, out = CpiParams(), CpiOutputs()
    assert lib.cpi_preintegrate_running(None, C.byref(prm), 1, 1, None, None, None, None, None, C.byref(out)) == 1
    assert lib.cpi_preintegrate_running_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, C.byref(out)) == 1


def test_engine_has_the_running_entries():
    import cpi_amd
    assert callable(cpi_amd.Engine.preintegrate_running) and callable(cpi_amd.Engine.preintegrate_running_host)
    assert cpi_amd.Engine._running_want(("mean", "jac", "cov"), 2) == ("mean", "cov")      # model 2: no running Jacobians
    assert cpi_amd.Engine._running_want(("mean", "jac", "cov"), 1) == ("mean", "jac", "cov")
    assert cpi_amd.Engine._running_want(("mean", "jac"), 2) == ("mean", "jac")             # an explicit request reaches the library


def test_running_kernels_are_in_the_resource_report():
    """The new kernels have rows of their own and spill nothing; the batch kernels keep their template signature."""
    from cpi_amd import build
    lines = open(build.REPORT).read().splitlines()
    run = [ln.split() for ln in lines if ln.startswith(("cpi_mean_running_kernel<", "cpi_cov_running_kernel<"))]
    names = " ".join(lines)
    for m in ("cpi_mean_running_kernel<1, false, false, false>", "cpi_mean_running_kernel<1, true, true, true>",
              "cpi_mean_running_kernel<2, false, true, true>", "cpi_cov_running_kernel<1, false>", "cpi_cov_running_kernel<2, true>"):
        assert m in names, m
    assert "cpi_mean_running_kernel<2, true" not in names          # model 2 has no running Jacobian kernel
    assert len(run) == 16 and all(r[-3] == "0" for r in run)       # scratch column
    rows = [ln.split(">")[0] for ln in lines if ln.startswith("cpi_mean_kernel<")]
    assert rows and all(r.count(",") == 5 for r in rows)           # <MODEL, JAC, AVG, L, CUT, BIG>: unchanged
