"""CPU-only checks of model 2's bias Jacobians after every interval and at query times (cpi_running_stj_batch / cpi_query_stj_batch and
their _host forms): the symbols are declared with the argument lists of their twins, listed under "additions within 3" and exported,
the ABI version is still 3, a NULL context is refused without a device, the kernels stand in a translation unit and a build report of
their own (no scratch, at least two wavefronts per SIMD) beside the four older reports, which are what HEAD holds, and the Python
layer and the C++ facade reach the new entries without changing the signatures of the old ones.

The running entries are NOT named cpi_preintegrate_*: tests/test_query_cpu.py and tests/test_gpu_entry_contract.py pin the set of
`int cpi_preintegrate_*(` prototypes of the header (every one of them has a row in the contract table), so the superset entry of
cpi_preintegrate_running is cpi_running_stj_batch, named like its companion cpi_query_stj_batch."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cpi_running_stj_batch", "cpi_running_stj_batch_host", "cpi_query_stj_batch", "cpi_query_stj_batch_host")
OLD_REPORTS = ("resource_usage.txt", "resource_usage_running_resume.txt", "resource_usage_query.txt", "resource_usage_query_cov.txt")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


def _flat_header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cpi_amd.h")).read())


def _args(flat, name):
    return flat.split("int %s(" % name, 1)[1].split(");", 1)[0]


def test_symbols_are_declared_with_their_twins_arguments_and_exported(lib):
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int
    flat = _flat_header()
    for new, twin in (("cpi_running_stj_batch", "cpi_preintegrate_running"), ("cpi_running_stj_batch_host", "cpi_preintegrate_running_host"),
                      ("cpi_query_stj_batch", "cpi_query_cov_batch"), ("cpi_query_stj_batch_host", "cpi_query_cov_batch_host")):
        assert _args(flat, new) == _args(flat, twin), new
        assert list(getattr(lib, new).argtypes) == list(getattr(lib, twin).argtypes), new
    assert _args(flat, "cpi_running_stj_batch") == ("cpi_ctx *ctx, const cpi_params *prm, int64_t W, int32_t N, const double *knots, const int64_t *first, "
                                                    "const int32_t *count, const double *lin, const double *q_k_lin, const cpi_outputs *rows")
    assert _args(flat, "cpi_query_stj_batch").endswith("const cpi_outputs *rows, int64_t Q, const int32_t *qwin, const double *qtime, const cpi_outputs *out")
    assert lib.cpi_abi_version() == 3 and "#define CPI_ABI_VERSION 3" in flat
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    assert "cpi_running_stj_batch, cpi_running_stj_batch_host, cpi_query_stj_batch, cpi_query_stj_batch_host" in within3


def test_header_says_what_is_still_missing_and_points_from_the_old_entries():
    flat = _flat_header()
    for name in ("cpi_running_stj_batch", "cpi_query_stj_batch"):
        tail = flat.split("int %s(" % name)[0].rsplit("Still not provided:", 1)[1]
        for gap in ("stream entries", "carry", "cpi_preintegrate_running_resume", "analytic Jacobians", "extrapolation past t_n"):
            assert gap in tail, (name, gap)
    # the older entries keep their sentences and point to the new ones
    old = flat.split("int cpi_preintegrate_running_resume(")[0].rsplit("Not provided:", 1)[1]
    assert "running Jacobian rows for model 2" in old and "cpi_running_stj_batch" in old
    old = flat.split("int cpi_query_cov_batch(")[0].rsplit("Still not provided:", 1)[1]
    assert "model-2 Jacobians at query times" in old and "cpi_query_stj_batch" in old
    old = flat.split("int cpi_query_batch(")[0].rsplit("Not provided:", 1)[1]
    assert "Jacobians for model 2" in old and "cpi_query_stj_batch" in old
    assert "cpi_running_stj_batch" in flat.split("int cpi_preintegrate_running(")[0].rsplit("/*", 1)[1]


def test_rejects_a_null_context_without_touching_a_device(lib):
    from cpi_amd._lib import CpiOutputs, CpiParams
    prm, rows, out = CpiParams(), CpiOutputs(), CpiOutputs()
    assert lib.cpi_running_stj_batch(None, C.byref(prm), 1, 1, None, None, None, None, None, C.byref(rows)) == 1
    assert lib.cpi_running_stj_batch_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, C.byref(rows)) == 1
    assert lib.cpi_query_stj_batch(None, C.byref(prm), 1, 1, None, None, None, None, None, C.byref(rows), 1, None, None, C.byref(out)) == 1
    assert lib.cpi_query_stj_batch_host(None, C.byref(prm), 1, 1, None, None, None, 0, None, None, 1, None, None, C.byref(out)) == 1


def _report(path):
    lines = open(path).read().splitlines()[1:]
    return sorted(ln.rsplit(">", 1)[0] + ">" for ln in lines), [ln.rsplit(">", 1)[1].split() for ln in lines]


def test_kernels_have_a_unit_and_a_report_of_their_own():
    """The unit's table lists exactly its four instantiations, none with scratch, each with at least two wavefronts per SIMD within
    256 registers; the running instantiation keeps the occupancy and the LDS of cpi_cov_running_kernel<2, *>; the unit takes cov_body
    through cpi_cov_kernels.hpp and does not include the query-covariance kernels; no other table names the new kernels."""
    from cpi_amd import _lib, build
    _lib.load()
    assert build.UNITS["cpi_stj"][-3:] == ["cpi_stj.hip", "cpi_cov_kernels.hpp", "cpi_stj_kernels.hpp"]
    src = open(os.path.join(build.CSRC, "cpi_stj.hip")).read() + open(os.path.join(build.CSRC, "cpi_stj_kernels.hpp")).read()
    assert "#define CPI_COV_TEMPLATES_ONLY" in src and "#include \"cpi_query_cov_kernels.hpp\"" not in src
    own = build.UNIT_REPORTS["cpi_stj"]
    assert os.path.basename(own) == "resource_usage_stj.txt"
    names, _ = _report(own)
    assert names == ["cpi_cov_running_stj_kernel<false>", "cpi_cov_running_stj_kernel<true>", "cpi_query_stj_kernel<false>", "cpi_query_stj_kernel<true>"]
    got = {}
    for ln in open(own).read().splitlines()[1:]:
        name = ln.rsplit(">", 1)[0] + ">"
        sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(">", 1)[1].split()
        assert scratch == "0" and int(occ) >= 2 and int(vgpr) + int(agpr) <= 256, ln
        got[name] = (int(occ), int(lds))
    base = {}
    for ln in open(build.REPORT).read().splitlines()[1:]:
        if ln.startswith("cpi_cov_running_kernel<2,"):
            cols = ln.rsplit(">", 1)[1].split()
            base[ln.split(">")[0].split(", ")[1]] = (int(cols[4]), int(cols[5]))
    assert set(base) == {"true", "false"}
    for avg in ("true", "false"):
        occ, lds = got["cpi_cov_running_stj_kernel<%s>" % avg]
        assert occ >= base[avg][0] and lds <= base[avg][1], (avg, occ, lds, base[avg])
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("_stj_kernel" in open(path).read()) == (unit == "cpi_stj"), path


def test_the_older_reports_are_what_head_holds():
    from cpi_amd import _lib
    _lib.load()
    if subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("not a git checkout: nothing to compare the reports with")
    for name in OLD_REPORTS:
        rel = "cpi_amd/csrc/" + name
        head = subprocess.run(["git", "show", "HEAD:" + rel], cwd=ROOT, stdout=subprocess.PIPE, check=True).stdout
        assert open(os.path.join(ROOT, rel), "rb").read() == head, name


def test_cpp_facade_has_the_new_members_and_the_old_ones_unchanged():
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    for sig in ("std::vector<std::vector<CpiResult>> running(const Context &ctx) const",
                "std::vector<std::vector<CpiResult>> running_stj(const Context &ctx) const",
                "std::vector<std::vector<CpiResult>> at(const Context &ctx, const std::vector<std::vector<double>> &times) const",
                "std::vector<std::vector<CpiResult>> at_cov(const Context &ctx, const std::vector<std::vector<double>> &times) const",
                "std::vector<std::vector<CpiResult>> at_stj(const Context &ctx, const std::vector<std::vector<double>> &times) const"):
        assert sig in src, sig
    for entry in ("cpi_running_stj_batch_host(", "cpi_query_stj_batch_host(", "cpi_preintegrate_running_host(", "cpi_query_cov_batch_host(", "cpi_query_batch_host("):
        assert entry in src, entry
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_query_stj.cpp"))


def test_engine_has_the_new_methods_and_keeps_the_old_signatures():
    import cpi_amd
    E = cpi_amd.Engine
    for new, old in ((E.preintegrate_running_stj, E.preintegrate_running), (E.preintegrate_running_stj_host, E.preintegrate_running_host),
                     (E.query_stj, E.query), (E.query_stj_host, E.query_host)):
        assert str(inspect.signature(new)) == str(inspect.signature(old)), new.__name__
    assert list(inspect.signature(E.preintegrate_running).parameters) == ["self", "knots", "lin", "q_k_lin", "params", "want", "first", "count", "N", "packed", "out"]
    assert list(inspect.signature(E.query).parameters) == ["self", "knots", "lin", "rows", "qwin", "qtime", "q_k_lin", "params", "want", "first", "count", "N", "out"]
    for fn, entry in ((E.preintegrate_running_stj, "cpi_running_stj_batch"), (E.preintegrate_running_stj_host, "cpi_running_stj_batch_host"),
                      (E.query_stj, "cpi_query_stj_batch"), (E.query_stj_host, "cpi_query_stj_batch_host")):
        assert "self.lib.%s(" % entry in inspect.getsource(fn)
    # the old methods do not reach the new entries
    for fn in (E.preintegrate_running, E.preintegrate_running_host, E.query, E.query_host):
        assert "_stj" not in inspect.getsource(fn)
    # model 2: "jac" means all seven matrices for the new methods, and is still dropped from the default want of the old one
    assert E._running_want(("mean", "jac", "cov"), 2) == ("mean", "cov")


def test_the_facade_program_compiles_here():
    """tests/cpp/test_query_stj.cpp (the GPU test's program) compiles and links against the library on a machine without a GPU."""
    import tempfile
    from cpi_amd import _lib
    _lib.load()
    exe = os.path.join(tempfile.mkdtemp(), "test_query_stj")
    libdir = os.path.join(ROOT, "cpi_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_query_stj.cpp"), "-o", exe,
                           "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
