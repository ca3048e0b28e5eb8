"""CPU: the contract of cpi_stream_running_stj_batch[_host] and cpi_query_stream_batch[_host] that needs no GPU -- the four symbols
are declared with their signatures, exported and listed under "additions within 3" of an ABI that is still 3; a NULL context is
refused without a device; the Engine methods and the facade members exist; the new unit's kernels have a resource report of their
own that no other report shares."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = (r"cpi_ctx \*ctx, const cpi_params \*prm, int64_t R, int64_t K, const double \*stream, const int64_t \*stream_offsets, "
           r"int64_t U, const double \*update_times, const int64_t \*update_offsets, int32_t N, const double \*lin, const double \*q_k_lin, ")
SIGNATURES = {
    "cpi_stream_running_stj_batch": STREAMS + r"void \*workspace, const cpi_outputs \*rows",
    "cpi_stream_running_stj_batch_host": STREAMS + r"const cpi_outputs \*rows, int32_t \*count",
    "cpi_query_stream_batch": STREAMS + (r"void \*workspace, const cpi_outputs \*rows, int64_t Q, const int32_t \*qrun, const double \*qtime, "
                                         r"int32_t \*qwin_out, const cpi_outputs \*out"),
    "cpi_query_stream_batch_host": STREAMS + r"int64_t Q, const int32_t \*qrun, const double \*qtime, int32_t \*qwin_out, const cpi_outputs \*out",
}
KERNELS = ["cpi_squery_cov_kernel<1, false>", "cpi_squery_cov_kernel<2, false>", "cpi_squery_cov_kernel<2, true>",
           "cpi_squery_jac2_kernel<false>", "cpi_squery_jac2_kernel<true>",
           "cpi_squery_mean_kernel<1, false, false>", "cpi_squery_mean_kernel<1, true, false>", "cpi_squery_mean_kernel<2, false, false>",
           "cpi_squery_mean_kernel<2, false, true>"]


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def test_symbols_are_declared_exported_and_listed(lib):
    from cpi_amd import build
    header = open(os.path.join(ROOT, "include", "cpi_amd.h")).read()
    flat = re.sub(r"\s+", " ", header)
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    additions = header.split("typedef struct cpi_ctx")[0].split("additions within 3")[1]
    for s, args in SIGNATURES.items():
        assert re.search(r"\bint %s\(%s\);" % (s, args), flat), s
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int and len(getattr(lib, s).argtypes) == args.count(",") + 1, s
        assert re.search(r"\b%s\b" % s, additions), s
        assert not s.startswith("cpi_preintegrate_")
    assert lib.cpi_abi_version() == 3 and re.search(r"#define CPI_ABI_VERSION\s+3\b", header)
    # what the header still does not provide after this
    doc = flat.split("int cpi_query_stream_batch(")[0].rsplit("/*", 1)[1]
    for gap in ("rows from a carry record", "model 2's analytic Jacobians", "extrapolation past t_n", "the device-set (cpi_group_*) path"):
        assert gap in doc.replace(" * ", " "), gap


def test_a_null_context_is_refused_without_a_device(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, rows, out = CpiParams(), CpiOutputs(), CpiOutputs()
    s = (1, 1, None, None, 1, None, None, 1, None, None)
    assert lib.cpi_stream_running_stj_batch(None, C.byref(prm), *s, None, C.byref(rows)) == 1
    assert lib.cpi_stream_running_stj_batch_host(None, C.byref(prm), *s, C.byref(rows), None) == 1
    assert lib.cpi_query_stream_batch(None, C.byref(prm), *s, None, C.byref(rows), 1, None, None, None, C.byref(out)) == 1
    assert lib.cpi_query_stream_batch_host(None, C.byref(prm), *s, 1, None, None, None, C.byref(out)) == 1
    assert lib.cpi_last_error(None) == b"ctx is NULL"


def test_engine_methods():
    import cpi_amd
    q = inspect.signature(cpi_amd.Engine.query_stream)
    assert list(q.parameters) == ["self", "stream", "update_times", "lin", "rows", "qtime", "q_k_lin", "params", "want", "N", "stream_offsets",
                                  "update_offsets", "qrun", "workspace", "out"]
    assert q.parameters["want"].default == ("mean",)
    assert all(q.parameters[k].default is None for k in list(q.parameters)[6:] if k != "want")
    h = inspect.signature(cpi_amd.Engine.query_stream_host)
    assert list(h.parameters)[:5] == ["self", "stream", "update_times", "lin", "qtime"] and "rows" not in h.parameters
    for name in ("preintegrate_stream_running_stj", "preintegrate_streams_running_stj", "preintegrate_stream_running_stj_host",
                 "preintegrate_streams_running_stj_host"):
        assert callable(getattr(cpi_amd.Engine, name)), name


def test_cpp_facade_members():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    one = src.split("class ImuStream {")[1].split("\n};")[0]
    many = src.split("class ImuStreamSet {")[1].split("\n};")[0]
    for member in ("at", "at_cov", "at_stj"):
        assert re.search(r"std::vector<CpiResult> %s\(const Context &ctx, const cpi_params &prm, const std::vector<double> &update_times" % member, one), member
        assert re.search(r"std::vector<CpiResult> %s\(const Context &ctx, const cpi_params &prm, const std::vector<int32_t> &runs" % member, many), member
    assert "cpi_query_stream_batch_host(" in src


def test_kernels_have_a_unit_and_a_report_of_their_own():
    from cpi_amd import _lib, build
    _lib.load()
    assert build.UNITS["cpi_query_stream"][-2:] == ["cpi_query_kernels.hpp", "cpi_query_stream_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_query_stream"]
    assert os.path.basename(own) == "resource_usage_query_stream.txt"
    lines = open(own).read().splitlines()[1:]
    assert sorted(ln.rsplit(">", 1)[0] + ">" for ln in lines) == KERNELS
    for ln in lines:
        sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(">", 1)[1].split()
        assert scratch == "0" and int(occ) >= 2 and int(vgpr) + int(agpr) <= 256, ln
    for unit, path in list(build.UNIT_REPORTS.items()) + [("", build.REPORT)]:
        assert ("cpi_squery_" in open(path).read()) == (unit == "cpi_query_stream"), path
    # the new argument block is a struct of its own, and the lookup loads are plain global loads (nothing is staged for them)
    args = open(os.path.join(build.CSRC, "cpi_args.hpp")).read()
    assert "struct StreamQueryArgs {" in args
    src = open(os.path.join(build.CSRC, "cpi_query_stream_kernels.hpp")).read()
    for helper in ("squery_window(", "squery_stamp(", "squery_interval("):
        assert re.search(r"CPI_HD \w[\w ]* %s" % re.escape(helper), src), helper
