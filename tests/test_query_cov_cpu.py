"""CPU-only checks of the covariance at arbitrary times (cpi_query_cov_batch / cpi_query_cov_batch_host): the symbols are declared
with the issue's signatures, listed under "additions within 3" and exported, the ABI version is still 3, a NULL context is refused
without a device, the kernels stand in a translation unit and a build report of their own beside the unchanged ones, and the Python
layer and the C++ facade reach the new entries without changing the signatures of the old ones."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_query_cov_batch", "cpi_query_cov_batch_host")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "cpi_amd.h")).read()


def test_symbols_are_declared_and_exported(lib):
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int
    flat = re.sub(r"\s+", " ", _header())
    dev = ("int cpi_query_cov_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, const int64_t *first, "
           "const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *rows, int64_t Q, const int32_t *qwin, "
           "const double *qtime, const cpi_outputs *out);")
    host = ("int cpi_query_cov_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, "
            "const int64_t *first, const int32_t *count, int64_t n_knots, const double *lin, const double *q_k_lin, int64_t Q, "
            "const int32_t *qwin, const double *qtime, const cpi_outputs *out);")
    assert dev in flat and host in flat
    assert list(lib.cpi_query_cov_batch.argtypes) == list(lib.cpi_query_batch.argtypes)
    assert list(lib.cpi_query_cov_batch_host.argtypes) == list(lib.cpi_query_batch_host.argtypes)
    assert lib.cpi_abi_version() == 3 and "#define CPI_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", _header())
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    assert "cpi_query_cov_batch, cpi_query_cov_batch_host" in within3


def test_header_says_what_is_still_missing_and_points_from_the_old_entry():
    flat = re.sub(r"\s+", " ", _header())
    new = flat.split("int cpi_query_cov_batch(")[0].rsplit("Still not provided:", 1)[1]
    for gap in ("model-2 Jacobians at query times", "cut from IMU streams in place", "carry record", "extrapolation past t_n"):
        assert gap in new, gap
    old = flat.split("int cpi_query_batch(")[0].rsplit("Not provided:", 1)[1]
    assert "P / P_sym at query times" in old and "cpi_query_cov_batch" in old and "stream entries" not in old
    host = flat.split("int cpi_query_cov_batch_host(")[0].rsplit("/*", 1)[1]
    assert "W * N rows" in host and "960 B" in host


def test_rejects_a_null_context_without_touching_a_device(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, rows, out = CpiParams(), CpiOutputs(), CpiOutputs()
    assert lib.cpi_query_cov_batch(None, C.byref(prm), 1, 1, None, None, None, None, None, C.byref(rows), 1, None, None, C.byref(out)) == 1
    assert lib.cpi_query_cov_batch_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, 1, None, None, C.byref(out)) == 1


def _report(path):
    lines = open(path).read().splitlines()[1:]
    return sorted(ln.rsplit(">", 1)[0] + ">" for ln in lines), [ln.rsplit(">", 1)[1].split() for ln in lines]


def test_kernels_have_a_unit_and_a_report_of_their_own():
    """The unit's table lists exactly its three instantiations (model 1 has no imu_avg instance: with the reading held the averaging
    is the identity), none with scratch, each with at least two wavefronts per SIMD within 256 registers; cpi_query keeps its four
    lines and no other table names the new kernel."""
    from cpi_amd import _lib, build
    _lib.load()
    assert build.UNITS["cpi_query_cov"][-2:] == ["cpi_query_cov.hip", "cpi_query_cov_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_query_cov"]
    assert os.path.basename(own) == "resource_usage_query_cov.txt"
    names, cols = _report(own)
    assert names == ["cpi_query_cov_kernel<1, false>", "cpi_query_cov_kernel<2, false>", "cpi_query_cov_kernel<2, true>"]
    for sgpr, vgpr, agpr, scratch, occ, lds in cols:
        assert scratch == "0" and int(occ) >= 2 and int(vgpr) + int(agpr) <= 256, (vgpr, agpr, scratch, occ)
    assert _report(build.UNIT_REPORTS["cpi_query"])[0] == ["cpi_query_kernel<1, false, false>", "cpi_query_kernel<1, true, false>",
                                                            "cpi_query_kernel<2, false, false>", "cpi_query_kernel<2, false, true>"]
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_query_cov_kernel" in open(path).read()) == (unit == "cpi_query_cov"), path
    # no existing unit includes the new kernels
    for unit, deps in build.UNITS.items():
        assert unit == "cpi_query_cov" or not any("query_cov" in d for d in deps), unit


def test_cpp_facade_has_at_cov_and_at_unchanged():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "std::vector<std::vector<CpiResult>> at(const Context &ctx, const std::vector<std::vector<double>> &times) const" in src
    assert "std::vector<std::vector<CpiResult>> at_cov(const Context &ctx, const std::vector<std::vector<double>> &times) const" in src
    assert "cpi_query_cov_batch_host(" in src and "cpi_query_batch_host(" in src
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_query_cov.cpp"))


def test_engine_routes_cov_requests_and_keeps_its_signatures():
    import cpi_amd
    q = inspect.signature(cpi_amd.Engine.query)
    assert list(q.parameters) == ["self", "knots", "lin", "rows", "qwin", "qtime", "q_k_lin", "params", "want", "first", "count", "N", "out"]
    h = inspect.signature(cpi_amd.Engine.query_host)
    assert list(h.parameters) == ["self", "knots", "lin", "qwin", "qtime", "q_k_lin", "params", "want", "count", "pinned", "out"]
    assert q.parameters["want"].default == ("mean",) and h.parameters["want"].default == ("mean",)
    for fn, new, old in ((cpi_amd.Engine.query, "cpi_query_cov_batch", "cpi_query_batch"),
                         (cpi_amd.Engine.query_host, "cpi_query_cov_batch_host", "cpi_query_batch_host")):
        src = inspect.getsource(fn)
        assert "self.lib.%s " % new in src and "self.lib.%s\n" % old in src and '"cov_sym"' in fn.__doc__
    assert cpi_amd.Engine._wants_cov(("mean", "cov")) and cpi_amd.Engine._wants_cov(("cov_sym",)) and not cpi_amd.Engine._wants_cov(("mean", "jac"))
