"""CPU-only checks of the measurement at arbitrary times (cpi_query_batch / cpi_query_batch_host): the symbols are declared with
the header's signatures, listed under "additions within 3" and exported, no cpi_preintegrate_* prototype came with them, the Python
layer and the C++ facade know them, a NULL context is refused without a device, and the kernels stand in a build report of
their own beside the two unchanged ones."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_query_batch", "cpi_query_batch_host")
# every cpi_preintegrate_* prototype of the header before these entries existed
PREINTEGRATE = {"cpi_preintegrate_batch", "cpi_preintegrate_resume", "cpi_preintegrate_running", "cpi_preintegrate_running_resume",
                "cpi_preintegrate_stream", "cpi_preintegrate_streams", "cpi_preintegrate_stream_running", "cpi_preintegrate_streams_running",
                "cpi_preintegrate_tiled_batch", "cpi_preintegrate_batch_host", "cpi_preintegrate_running_host",
                "cpi_preintegrate_running_resume_host", "cpi_preintegrate_resume_host", "cpi_preintegrate_tiled_batch_host",
                "cpi_preintegrate_stream_host", "cpi_preintegrate_streams_host", "cpi_preintegrate_stream_running_host",
                "cpi_preintegrate_streams_running_host"}


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
    dev = ("int cpi_query_batch(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, const int64_t *first, "
           "const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *rows, int64_t Q, const int32_t *qwin, "
           "const double *qtime, const cpi_outputs *out);")
    host = ("int cpi_query_batch_host(cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, "
            "const int64_t *first, const int32_t *count, int64_t n_knots, const double *lin, const double *q_k_lin, int64_t Q, "
            "const int32_t *qwin, const double *qtime, const cpi_outputs *out);")
    assert dev in flat and host in flat
    assert len(lib.cpi_query_batch.argtypes) == 14 and len(lib.cpi_query_batch_host.argtypes) == 14
    assert lib.cpi_abi_version() == 3 and "#define CPI_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", header)
    assert "cpi_query_batch, cpi_query_batch_host" in flat.split("typedef struct cpi_ctx")[0]       # "additions within 3"
    for gap in ("P / P_sym at query times", "Jacobians for model 2", "cut from IMU streams in place", "carry record", "extrapolation past t_n"):
        assert gap in flat.split("int cpi_query_batch(")[0].rsplit("Not provided:", 1)[1], gap


def test_no_preintegrate_prototype_was_added():
    header = open(os.path.join(ROOT, "include", "cpi_amd.h")).read()
    assert set(re.findall(r"\bint (cpi_preintegrate_\w+)\(", header)) == PREINTEGRATE


def test_rejects_a_null_context_without_touching_a_device(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, rows, out = CpiParams(), CpiOutputs(), CpiOutputs()
    assert lib.cpi_query_batch(None, C.byref(prm), 1, 1, None, None, None, None, None, C.byref(rows), 1, None, None, C.byref(out)) == 1
    assert lib.cpi_query_batch_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, 1, None, None, C.byref(out)) == 1


def test_engine_has_query_and_query_host():
    import cpi_amd
    q = inspect.signature(cpi_amd.Engine.query)
    assert list(q.parameters) == ["self", "knots", "lin", "rows", "qwin", "qtime", "q_k_lin", "params", "want", "first", "count", "N", "out"]
    assert q.parameters["want"].default == ("mean",) and all(q.parameters[k].default is None for k in ("q_k_lin", "params", "first", "count", "N", "out"))
    h = inspect.signature(cpi_amd.Engine.query_host)
    assert list(h.parameters) == ["self", "knots", "lin", "qwin", "qtime", "q_k_lin", "params", "want", "count", "pinned", "out"]
    assert h.parameters["want"].default == ("mean",) and h.parameters["pinned"].default is True


def test_query_kernels_have_a_report_of_their_own():
    """The query unit's table lists exactly its four instantiations (model 1 with and without Jacobians -- no imu_avg instance:
    with the reading held the averaging is the identity --, model 2 with and without imu_avg), none with scratch; the two older
    tables are what the parent commit holds."""
    from cpi_amd import _lib, build
    _lib.load()
    assert "cpi_query" in build.UNITS
    own = build.UNIT_REPORTS["cpi_query"]
    assert os.path.basename(own) == "resource_usage_query.txt"
    lines = open(own).read().splitlines()[1:]
    names = sorted(ln.rsplit(">", 1)[0] + ">" for ln in lines)
    assert names == ["cpi_query_kernel<1, false, false>", "cpi_query_kernel<1, true, false>", "cpi_query_kernel<2, false, false>",
                     "cpi_query_kernel<2, false, true>"]
    for ln in lines:
        sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(">", 1)[1].split()
        assert scratch == "0" and int(occ) >= 2, ln
    for path in (build.REPORT, build.UNIT_REPORTS["cpi_running_resume"]):
        assert "cpi_query_kernel" not in open(path).read()
        # the build rewrites the tables: what it wrote must be what the commit holds (the commit's are the parent's, untouched)
        p = subprocess.run(["git", "show", "HEAD:" + os.path.relpath(path, ROOT)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode == 0:        # (an exported tree without history has nothing to compare with)
            assert open(path).read() == p.stdout, path


def test_cpp_facade_has_at():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "std::vector<std::vector<CpiResult>> at(const Context &ctx, const std::vector<std::vector<double>> &times) const" in src
    assert "cpi_query_batch_host(" in src
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_query.cpp"))   # compiled by tests/test_abi.py's facade check
