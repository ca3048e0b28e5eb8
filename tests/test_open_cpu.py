"""CPU-only checks of the open-window entries (cpi_running_resume_stj_batch / cpi_query_open_batch and their _host forms): the symbols
are declared with the argument lists the issue gives them, listed under "additions within 3" and exported, the ABI version is still
3, cpi_carry_doubles is what it was, a NULL context is refused without a device, the kernels stand in two translation units with
build reports of their own (no scratch, two wavefronts per SIMD for the covariance-type kernels) beside the older reports, which are
what HEAD holds, and the Python layer and the C++ facade reach the new entries.

Neither name begins with cpi_preintegrate_: tests/test_query_cpu.py and tests/test_gpu_entry_contract.py pin that set of prototypes."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_running_resume_stj_batch", "cpi_running_resume_stj_batch_host", "cpi_query_open_batch", "cpi_query_open_batch_host")
OLD_REPORTS = ("resource_usage.txt", "resource_usage_running_resume.txt", "resource_usage_query.txt", "resource_usage_query_cov.txt",
               "resource_usage_stj.txt", "resource_usage_query_stream.txt")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def _flat_header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cpi_amd.h")).read())


def _args(flat, name):
    return flat.split("int %s(" % name, 1)[1].split(");", 1)[0]


def test_symbols_are_declared_listed_and_exported(lib):
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in SYMBOLS:
        assert not s.startswith("cpi_preintegrate_")
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int
    flat = _flat_header()
    for new, twin in (("cpi_running_resume_stj_batch", "cpi_preintegrate_running_resume"),
                      ("cpi_running_resume_stj_batch_host", "cpi_preintegrate_running_resume_host")):
        assert _args(flat, new) == _args(flat, twin), new
        assert list(getattr(lib, new).argtypes) == list(getattr(lib, twin).argtypes), new
    assert _args(flat, "cpi_query_open_batch") == _args(flat, "cpi_query_stj_batch") + ", const cpi_outputs *base, int32_t base_N"
    assert list(lib.cpi_query_open_batch.argtypes[:-2]) == list(lib.cpi_query_stj_batch.argtypes)
    assert lib.cpi_query_open_batch.argtypes[-1] is C.c_int32 and len(lib.cpi_query_open_batch.argtypes) == 16
    host = _args(flat, "cpi_query_open_batch_host")
    assert host == ("cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, const int64_t *first, const int32_t *count, "
                    "int64_t n_knots, const double *lin, const double *q_k_lin, const double *carry_in, double *carry_out, int64_t Q, "
                    "const int32_t *qwin, const double *qtime, const cpi_outputs *out")
    assert len(lib.cpi_query_open_batch_host.argtypes) == 16
    assert lib.cpi_abi_version() == 3 and "#define CPI_ABI_VERSION 3" in flat
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    for s in SYMBOLS:
        assert s in within3, s
    # the set of cpi_preintegrate_* prototypes is the one the contract table knows
    assert "cpi_preintegrate_running_resume_stj" not in flat and "cpi_preintegrate_query" not in flat


def test_carry_doubles_is_unchanged(lib):
    assert [lib.cpi_carry_doubles(m) for m in (0, 1, 2, 3)] == [0, 288, 566, 0]


def test_header_points_to_the_new_entries_and_says_what_is_still_missing():
    flat = _flat_header()
    for name in ("cpi_running_resume_stj_batch", "cpi_query_open_batch"):
        tail = flat.split("int %s(" % name)[0].rsplit("Still not provided:", 1)[1]
        for gap in ("carry records for the stream entries", "analytic Jacobians in running form", "extrapolation past t_n"):
            assert gap in tail, (name, gap)
    old = flat.split("int cpi_preintegrate_running_resume(")[0].rsplit("Not provided:", 1)[1]
    assert "running Jacobian rows for model 2" in old and "cpi_running_resume_stj_batch" in old
    for entry in ("cpi_query_batch", "cpi_query_cov_batch", "cpi_query_stj_batch"):
        old = flat.split("int %s(" % entry)[0].rsplit("ot provided:", 1)[1]
        assert "carry record" in old and "cpi_query_open_batch" in old, entry
    old = flat.split("int cpi_running_stj_batch(")[0].rsplit("Still not provided:", 1)[1]
    assert "cpi_running_resume_stj_batch" in old


def test_rejects_a_null_context_without_touching_a_device(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, rows, out = CpiParams(), CpiOutputs(), CpiOutputs()
    assert lib.cpi_running_resume_stj_batch(None, C.byref(prm), 1, 1, None, None, None, None, None, None, None, C.byref(rows)) == 1
    assert lib.cpi_running_resume_stj_batch_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, None, None, C.byref(rows)) == 1
    assert lib.cpi_query_open_batch(None, C.byref(prm), 1, 1, None, None, None, None, None, C.byref(rows), 1, None, None, C.byref(out),
                                    C.byref(rows), 1) == 1
    assert lib.cpi_query_open_batch_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, None, None, 1, None, None, C.byref(out)) == 1


def _rows(path):
    out = {}
    for ln in open(path).read().splitlines()[1:]:
        sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(">", 1)[1].split()
        out[ln.rsplit(">", 1)[0] + ">"] = dict(vgpr=int(vgpr), agpr=int(agpr), scratch=int(scratch), occ=int(occ), lds=int(lds))
    return out


def test_kernels_have_units_and_reports_of_their_own():
    """Two units, each with its own table: the carry variant of the running Jacobian read-out keeps the occupancy and the LDS of
    cpi_cov_running_stj_kernel; the open query kernels keep the LDS of their closed twins; nothing spills; every covariance-type
    kernel holds the two wavefronts per SIMD its launch bounds ask for; no older table names a new kernel."""
    from cpi_amd import _lib, build
    _lib.load()
    assert "cpi_cov_kernels.hpp" in build.UNITS["cpi_running_resume_stj"] and "cpi_running_resume_stj.hip" in build.UNITS["cpi_running_resume_stj"]
    for f in ("cpi_query_open.hip", "cpi_query_open_kernels.hpp", "cpi_query_locate.hpp", "cpi_query_kernels.hpp", "cpi_covq_body.hpp", "cpi_covq_body.inc",
              "cpi_stj_kernels.hpp"):
        assert f in build.UNITS["cpi_query_open"], f
    a = _rows(build.UNIT_REPORTS["cpi_running_resume_stj"])
    assert sorted(a) == ["cpi_cov_running_stj_carry_kernel<false>", "cpi_cov_running_stj_carry_kernel<true>"]
    closed = _rows(build.UNIT_REPORTS["cpi_stj"])
    for avg in ("true", "false"):
        new, old = a["cpi_cov_running_stj_carry_kernel<%s>" % avg], closed["cpi_cov_running_stj_kernel<%s>" % avg]
        assert new["scratch"] == 0 and new["occ"] == 2 and new["vgpr"] + new["agpr"] <= 256 and new["lds"] <= old["lds"], (new, old)
    b = _rows(build.UNIT_REPORTS["cpi_query_open"])
    twins = dict(_rows(build.UNIT_REPORTS["cpi_query"]), **_rows(build.UNIT_REPORTS["cpi_query_cov"]))
    twins.update({k: v for k, v in closed.items() if k.startswith("cpi_query_stj_kernel")})
    assert sorted(k.replace("_open_kernel", "_kernel") for k in b) == sorted(twins)
    for name, r in b.items():
        old = twins[name.replace("_open_kernel", "_kernel")]
        assert r["scratch"] == 0 and r["lds"] == old["lds"] and r["vgpr"] + r["agpr"] <= 256, (name, r)
        if "_cov_" in name or "_stj_" in name:
            assert r["occ"] >= 2, (name, r)
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        txt = open(path).read()
        assert ("_open_kernel" in txt) == (unit == "cpi_query_open"), path
        assert ("_stj_carry_kernel" in txt) == (unit == "cpi_running_resume_stj"), path


def test_the_older_reports_are_what_head_holds():
    from cpi_amd import _lib
    _lib.load()
    if subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("not a git checkout: nothing to compare the reports with")
    for name in OLD_REPORTS:
        rel = "cpi_amd/csrc/" + name
        head = subprocess.run(["git", "show", "HEAD:" + rel], cwd=ROOT, stdout=subprocess.PIPE, check=True).stdout
        assert open(os.path.join(ROOT, rel), "rb").read() == head, name


def test_staging_limit_is_derived_not_a_literal():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_abi.hip")).read()
    assert re.search(r"static constexpr int kMax = \d+ \+ 3 \* kOutFields;", src)


def test_engine_and_facades_reach_the_new_entries():
    import cpi_amd
    from cpi_amd import engine
    E = cpi_amd.Engine
    assert str(inspect.signature(E.preintegrate_running_resume_stj)) == str(inspect.signature(E.preintegrate_running_resume))
    assert str(inspect.signature(E.preintegrate_running_resume_stj_host)) == str(inspect.signature(E.preintegrate_running_resume_host))
    assert list(inspect.signature(E.query_open).parameters)[:7] == ["self", "knots", "lin", "rows", "qwin", "qtime", "base"]
    for fn, entry in ((E.preintegrate_running_resume_stj, "cpi_running_resume_stj_batch"),
                      (E.preintegrate_running_resume_stj_host, "cpi_running_resume_stj_batch_host"),
                      (E.query_open, "cpi_query_open_batch"), (E.query_open_host, "cpi_query_open_batch_host")):
        assert "self.lib.%s(" % entry in inspect.getsource(fn)
    # read_rows keeps its entry; at() is new
    assert "preintegrate_running_resume(" in inspect.getsource(engine._CpiBase.read_rows)
    assert "query_open(" in inspect.getsource(engine._CpiBase.at)
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "std::vector<CpiResult> at(const Context &ctx, const std::vector<double> &times)" in src and "cpi_query_open_batch_host(" in src
    with pytest.raises(RuntimeError, match="set_incremental"):
        cpi_amd.CpiV2(1, 1, 1, 1).at([0.0])


def test_the_facade_program_compiles_here():
    """tests/cpp/test_open_at.cpp (the GPU test's program) compiles and links against the library on a machine without a GPU."""
    from cpi_amd import _lib
    _lib.load()
    exe = os.path.join(tempfile.mkdtemp(), "test_open_at")
    libdir = os.path.join(ROOT, "cpi_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_open_at.cpp"), "-o", exe,
                           "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
