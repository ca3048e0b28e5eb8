"""CPU-only checks of running preintegration from a carry record (cpi_preintegrate_running_resume): the symbols are declared with
the header's signatures and exported within ABI 3, the Python layer and the C++ facade know them, the calls that can be refused
without a context are refused, and the new kernels stand in the build report beside their unchanged twins."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_preintegrate_running_resume", "cpi_preintegrate_running_resume_host")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "cpi_amd.h")).read()
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int
    flat = re.sub(r"\s+", " ", header)
    dev = ("int cpi_preintegrate_running_resume(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, "
           "const int64_t *first, const int32_t *count, const double *lin, const double *q_k_lin, const double *carry_in, "
           "double *carry_out, const cpi_outputs *rows);")
    host = ("int cpi_preintegrate_running_resume_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, "
            "const int64_t *first, const int32_t *count, int64_t n_knots, const double *lin, const double *q_k_lin, "
            "const double *carry_in, double *carry_out, const cpi_outputs *rows);")
    assert dev in flat and host in flat
    assert len(lib.cpi_preintegrate_running_resume.argtypes) == 12 and len(lib.cpi_preintegrate_running_resume_host.argtypes) == 13
    assert lib.cpi_abi_version() == 3 and "#define CPI_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", header)
    additions = flat.split("typedef struct cpi_ctx")[0]
    assert "cpi_preintegrate_running_resume, cpi_preintegrate_running_resume_host" in additions       # "additions within 3"
    assert "Not provided: running rows from a carry record" not in header
    assert (lib.cpi_carry_doubles(1), lib.cpi_carry_doubles(2)) == (288, 566)                        # the record layout did not change


def test_rejects_a_null_context_without_touching_a_device(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, out = CpiParams(), CpiOutputs()
    assert lib.cpi_preintegrate_running_resume(None, C.byref(prm), 1, 1, None, None, None, None, None, None, None, C.byref(out)) == 1
    assert lib.cpi_preintegrate_running_resume_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, None, None, C.byref(out)) == 1


def test_engine_and_mirror_have_the_entries():
    import cpi_amd
    assert callable(cpi_amd.Engine.preintegrate_running_resume) and callable(cpi_amd.Engine.preintegrate_running_resume_host)
    assert callable(cpi_amd.CpiV1.read_rows) and callable(cpi_amd.CpiV2.read_rows)
    cpi = cpi_amd.CpiV1(0.005, 4e-6, 0.01, 2e-4)
    with pytest.raises(RuntimeError, match="set_incremental"):
        cpi.read_rows()                                     # refused before any engine is touched
    cpi.set_incremental(True)
    assert cpi.read_rows() == []                            # nothing fed: nothing runs
    v2 = cpi_amd.CpiV2(0.005, 4e-6, 0.01, 2e-4)
    v2.set_incremental(True)
    v2.state_transition_jacobians = False
    with pytest.raises(ValueError, match="no running form"):
        v2.read_rows()


def test_mirror_maps_fed_intervals_to_rows():
    """_knots(closing): per fed interval the index of its closing knot; separator knots (intervals that do not chain) and the
    carried tail knot own no entry."""
    import numpy as np
    import cpi_amd
    cpi = cpi_amd.CpiV1(0.005, 4e-6, 0.01, 2e-4, imu_avg_=True)
    w, a = np.ones(3), np.ones(3)
    cpi.feed_IMU(0.0, 0.1, w, a, 2 * w, 2 * a)
    cpi.feed_IMU(0.1, 0.2, 2 * w, 2 * a, 3 * w, 3 * a)      # chains
    cpi.feed_IMU(0.5, 0.6, w, a, w, a)                      # does not: NaN separator + a fresh opening knot
    closing = []
    kn = cpi._knots(closing)
    assert closing == [1, 2, 5] and kn.shape == (6, 7) and np.isnan(kn[3, 0])
    cpi._tail = kn[-1]
    cpi._iv = [(0.6, 0.7, w, a, w, a)]
    closing = []
    assert cpi._knots(closing).shape == (2, 7) and closing == [1]


def test_cpp_facade_has_read_rows():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "std::vector<CpiResult> read_rows(const Context &ctx)" in src and "cpi_preintegrate_running_resume_host(" in src
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_running_resume.cpp"))   # compiled by tests/test_abi.py's facade check


def test_new_kernels_are_in_the_resource_report():
    """Twelve mean and four covariance instantiations with rows of their own, no scratch, the occupancy and LDS of their
    non-carry twins.  They are the kernels of a translation unit of their own (cpi_running_resume.hip) and stand in that unit's
    table, resource_usage_running_resume.txt; resource_usage.txt keeps exactly the kernels it listed before."""
    from cpi_amd import build
    rows = {}
    own = build.UNIT_REPORTS["cpi_running_resume"]
    assert os.path.basename(own) == "resource_usage_running_resume.txt"
    assert "_carry_kernel<" not in open(build.REPORT).read().replace("cpi_mean_carry_kernel<", "").replace("cpi_cov_carry_kernel<", "")
    assert len(open(own).read().splitlines()) == 1 + 16    # nothing but the sixteen new instantiations (no second copy of another kernel)
    for ln in open(build.REPORT).read().splitlines()[1:] + open(own).read().splitlines()[1:]:
        name, rest = ln.rsplit(">", 1) if ">" in ln else (ln.split()[0], ln[len(ln.split()[0]):])
        rows[name + (">" if ">" in ln else "")] = rest.split()
    new = [k for k in rows if k.startswith(("cpi_mean_running_carry_kernel<", "cpi_cov_running_carry_kernel<"))]
    assert len(new) == 16 and not any(k.startswith("cpi_mean_running_carry_kernel<2, true") for k in new)
    for k in new:
        twin = k.replace("_carry_kernel", "_kernel")
        assert twin in rows, twin
        sgpr, vgpr, agpr, scratch, occ, lds = rows[k]
        assert scratch == "0", (k, scratch)                 # no spilling that the twins do not have
        assert (occ, lds) == (rows[twin][4], rows[twin][5]), (k, rows[k], rows[twin])
