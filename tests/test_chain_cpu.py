"""CPU: cpi_chain_solve_batch without a GPU -- declarations, contract, and the arithmetic.

1. Declarations: the entries are exported, declared in include/cpi_amd.h with their exact argument lists, listed among the additions
   within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_chain has a resource report of its own, no other report names one of its
   kernels, it uses no scratch; Engine, the module and the C++ facade have the entries.
2. The contract through ctypes: every refusal comes before the context is looked at, so a NULL context shows code and text; every
   pair (output, input) and (output, output) that may not overlap is tried.  The host form names the chain whose range is wrong.
3. The inputs of tests/chain_cases.py are what they claim to be (finite float64 Cholesky, cond <= 1e11), and the host twin
   (tests/hostsim/hostsim_chain.cpp over namespace chn of cpi_math.hpp, compiled with -ffp-contract=off) meets the gates against the
   longdouble reference on every layout, damping and prior variant of the GPU tests.  Both metrics are printed first.
4. The edges of the contract (the cases of tests/chain_cases.py, the checks of tests/chain_edge_checks.py) on the twin, before
   tests/test_gpu_chain_edges.py asks the same of the device; and the twin with one rule of the contract broken, built in tmp_path,
   fails the check that states the rule."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import chain_edge_checks as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_chain.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_chain.so")
_HDRS = [os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")]

HEAD = ("cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count, const int64_t *ffirst, "
        "const double *hess, const double *prior, const double *lambda, int32_t damping, double *delta, int32_t *status")
DECLS = {"cpi_chain_solve_batch": HEAD + ", double *workspace", "cpi_chain_solve_batch_host": HEAD}


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- declarations
def test_symbols_are_declared_bound_and_exported(lib):
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cpi_amd.h")).read())
    for s, args in DECLS.items():
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int and len(getattr(lib, s).argtypes) == args.count(",") + 1, s
        assert flat.split("int %s(" % s, 1)[1].split(");", 1)[0] == args, s
    assert re.search(r" T cpi_chain_solve_workspace_doubles$", dyn, re.M)
    assert "size_t cpi_chain_solve_workspace_doubles(int64_t S);" in flat and lib.cpi_chain_solve_workspace_doubles.restype is C.c_size_t
    assert "enum { CPI_DAMP_IDENTITY = 0, CPI_DAMP_DIAGONAL = 1 };" in flat
    assert lib.cpi_abi_version() == 3
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    for s in list(DECLS) + ["cpi_chain_solve_workspace_doubles"]:
        assert s in within3, s
    doc = flat.split("enum { CPI_DAMP_IDENTITY")[0].rsplit("/*", 1)[1]
    for text in ("PARITY UNPINNED", "GTSAM's linear solver", "minDiagonal", "maxDiagonal", "overlaps", "allocates nothing", "DEVICE doubles",
                 "no parallelism ALONG a chain"):
        assert text in doc, text
    # the section stands after the cost entries, and the trial-step comment is still the last "/* ----" block before cpi_retract_batch
    assert flat.index("int cpi_factor_cost_tri_batch(") < flat.index("int cpi_chain_solve_batch(") < flat.index("/* ---- Device sets")
    trial = flat.split("int cpi_retract_batch(")[0].rsplit("/* ----", 1)[1]
    assert "No solver is provided" not in trial and "cpi_chain_solve_batch" in trial and "JPLNavState.cpp:37-71" in trial


def test_kernel_has_a_unit_and_a_report_of_its_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_chain"][-3:] == ["cpi_chain.hip", "cpi_factor_kernels.hpp", "cpi_chain_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_chain"]
    assert os.path.basename(own) == "resource_usage_chain.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == ["cpi_chain_solve_kernel"]
    for name, (regs, scratch, occ, lds) in rows.items():
        assert name.startswith("cpi_chain_") and scratch == 0 and regs <= 512 and occ >= 1, (name, regs, scratch, occ)
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_chain_" in open(path).read()) == (unit == "cpi_chain"), path
    math = open(os.path.join(build.CSRC, "cpi_math.hpp")).read()
    body = math.split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    for helper in ("factor_block(", "solve_w(", "schur(", "solve_chain("):
        assert re.search(r"CPI_HD \w[\w<> ]* %s" % re.escape(helper), body), helper


def test_engine_module_and_facade_have_the_entries():
    import inspect
    import cpi_amd
    E = cpi_amd.Engine
    for fn, sym in ((E.chain_solve, "cpi_chain_solve_batch("), (E.chain_solve_host, "cpi_chain_solve_batch_host("),
                    (E.chain_solve_workspace_doubles, "cpi_chain_solve_workspace_doubles(")):
        assert sym in inspect.getsource(fn), sym
    assert list(inspect.signature(E.chain_solve).parameters)[1:] == ["hess", "C", "G", "first", "count", "ffirst", "prior", "lam", "damping",
                                                                      "out", "status", "workspace"]
    assert inspect.signature(E.chain_solve).parameters["damping"].default == "identity"
    assert list(inspect.signature(E.chain_solve_host).parameters)[1:] == ["hess", "C", "G", "first", "count", "ffirst", "prior", "lam",
                                                                           "damping", "out", "status"]
    assert list(inspect.signature(E.chain_indices).parameters) == ["C", "G", "first", "count"]
    assert callable(cpi_amd.chain_solve)
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_chain_solve_batch_host(" in src and re.search(r"std::vector<double> chain_solve\(const Context &ctx", src)


def test_chain_indices_are_the_pairs_the_solve_reads():
    import torch
    import cpi_amd
    ii, jj = cpi_amd.Engine.chain_indices(3, 4)
    assert ii.dtype == torch.int32 and ii.tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 10] and jj.tolist() == [1, 2, 3, 5, 6, 7, 9, 10, 11]
    first = torch.tensor([10, 0, 5], dtype=torch.int64)
    count = torch.tensor([3, 1, 9], dtype=torch.int32)                     # 9 is clamped to G = 4
    ii, jj = cpi_amd.Engine.chain_indices(3, 4, first, count)
    assert ii.tolist() == [10, 11, 5, 6, 7] and jj.tolist() == [11, 12, 6, 7, 8]
    ii, jj = cpi_amd.Engine.chain_indices(2, 1)
    assert ii.numel() == 0 and jj.numel() == 0


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


@pytest.mark.parametrize("entry", ["cpi_chain_solve_batch", "cpi_chain_solve_batch_host"])
def test_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    host = entry.endswith("_host")
    Cn, G = 4, 3
    S, F = Cn * G, Cn * (G - 1)
    a = {"first": np.arange(Cn, dtype=np.int64) * G, "count": np.full(Cn, G, dtype=np.int32), "ffirst": np.arange(Cn, dtype=np.int64) * (G - 1),
         "hess": np.zeros(F * 496), "prior": np.zeros(S * 136), "lambda": np.zeros(Cn), "delta": np.zeros(S * 15),
         "status": np.zeros(Cn, dtype=np.int32), "workspace": np.zeros(lib.cpi_chain_solve_workspace_doubles(S))}
    # status heads a buffer as long as the workspace: a workspace that begins inside status then ends inside that buffer, wherever
    # numpy put the other arrays (with delta behind status, "delta overlaps" was reported where "status overlaps" is expected)
    a["status"] = np.zeros(Cn + 2 * a["workspace"].size, dtype=np.int32)[:Cn]
    ptr = lambda x, off=0: None if x is None else x.ctypes.data + off

    def call(C_=Cn, G_=G, S_=S, F_=F, damping=0, **kw):
        v = {k: ptr(x) for k, x in a.items()}
        v.update(kw)
        args = [None, C_, G_, S_, F_, v["first"], v["count"], v["ffirst"], v["hess"], v["prior"], v["lambda"], damping, v["delta"], v["status"]]
        rc = f(*(args if host else args + [v["workspace"]]))
        return rc, _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")                                       # a valid call gets as far as the context
    assert call(first=None, count=None, ffirst=None, prior=None, status=None, **{"lambda": None}) == (1, "ctx is NULL")
    assert call(damping=1) == (1, "ctx is NULL")
    assert call(G_=1, F_=0, hess=None, S_=Cn, first=None, ffirst=None) == (1, "ctx is NULL")   # chains of one state need no hess
    assert call(C_=0, delta=None, workspace=None, hess=None) == (1, "ctx is NULL")   # C == 0 is a no-op: nothing to refuse
    refused("negative size", C_=-1)
    refused("negative size", S_=-1)
    refused("negative size", F_=-1)
    refused("G (the longest chain in states) must be >= 1", G_=0)
    refused("G exceeds 2^31 - 1", G_=2 ** 31)
    refused("damping must be", damping=2)
    refused("damping must be", damping=-1)
    refused("hess is NULL", hess=None)
    refused("delta is NULL", delta=None)
    if not host:
        refused("workspace is NULL", workspace=None)
    outs = ("delta", "status") + (() if host else ("workspace",))
    for o in outs:                                                            # every output against every input ...
        for i in ("first", "count", "ffirst", "hess", "prior", "lambda"):
            # the output begins inside the input's last element (the workspace is long enough to reach the arrays numpy put behind it
            # as well: whichever output the text names, it is an overlap)
            refused("overlaps" if o == "workspace" else "%s overlaps" % o, **{o: ptr(a[i], a[i].nbytes - 8)})
            refused("overlaps", **{i: ptr(a[o], 8)})                          # the input begins inside the output
    refused("delta overlaps", status=ptr(a["delta"], 8 * (S * 15 - 1)))      # ... and against every other output
    if not host:
        refused("delta overlaps", workspace=ptr(a["delta"], 8))
        refused("status overlaps", workspace=ptr(a["status"], 4))
    buf = np.zeros(S * 15 + Cn)
    assert call(delta=ptr(buf), status=ptr(buf, 8 * S * 15)) == (1, "ctx is NULL")   # back to back: fine


def test_host_form_names_the_chain_whose_range_is_wrong(lib):
    f, entry = lib.cpi_chain_solve_batch_host, "cpi_chain_solve_batch_host"
    Cn, G = 4, 3
    S, F = Cn * G, Cn * (G - 1)
    hess, delta = np.zeros(F * 496), np.zeros(S * 15)
    first, ffirst = np.arange(Cn, dtype=np.int64) * G, np.arange(Cn, dtype=np.int64) * (G - 1)
    d = lambda x: None if x is None else x.ctypes.data

    def call(first_=first, ffirst_=ffirst, count_=None, S_=S, F_=F):
        rc = f(None, Cn, G, S_, F_, d(first_), d(count_), d(ffirst_), d(hess), None, None, 0, d(delta), None)
        return rc, _err(lib)

    assert call() == (1, "ctx is NULL")
    assert call(first_=None, ffirst_=None) == (1, "ctx is NULL")
    bad = ffirst.copy()
    bad[2] = F - 1                                                            # two factor rows from F - 1 on: one past the end
    rc, msg = call(ffirst_=bad)
    assert rc == 1 and msg.startswith(entry + ": ") and "the factor rows of chain 2 leave [0, F)" in msg, msg
    bad[2] = -1
    assert "the factor rows of chain 2 leave [0, F)" in call(ffirst_=bad)[1]
    assert "the factor rows of chain 3 leave [0, F)" in call(F_=F - 1)[1]     # the last chain's range past a shorter hess
    bad = first.copy()
    bad[1] = S - 2                                                            # three states from S - 2 on
    rc, msg = call(first_=bad)
    assert rc == 1 and msg.startswith(entry + ": ") and "the states of chain 1 leave [0, S)" in msg, msg
    bad[1] = -3
    assert "the states of chain 1 leave [0, S)" in call(first_=bad)[1]
    assert "the states of chain 3 leave [0, S)" in call(S_=S - 1)[1]
    ok = first.copy()
    ok[1] = S - 2
    assert call(first_=ok, count_=np.array([3, 2, 3, 3], dtype=np.int32), ffirst_=ffirst) == (1, "ctx is NULL")   # two states fit


def test_workspace_size(lib):
    n = [lib.cpi_chain_solve_workspace_doubles(S) for S in (-5, 0, 1, 2, 17, 1000, 10 ** 6, 2 ** 31 - 1)]
    assert all(v >= 1 for v in n) and n == sorted(n)
    assert n[2] >= 360 and n[5] >= 360 * 1000


# ---------------------------------------------------------------- host twin
@pytest.fixture(scope="module")
def hs():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in [_SRC] + _HDRS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB, _SRC])
    lib = C.CDLL(_LIB)
    vp = C.c_void_p
    lib.hsc_chain_solve.argtypes = [C.c_longlong] * 4 + [vp] * 6 + [C.c_int, vp, vp, vp]
    return lib


def host_solve(hs, b, lam, diagonal, explicit=None, with_prior=True):
    explicit = b.explicit if explicit is None else explicit
    delta = np.full((b.S, 15), -7.0)
    status = np.full(b.C, 99, dtype=np.int32)
    ws = np.zeros(max(b.S, 1) * hs.hsc_ws_doubles())
    p = lambda x: None if x is None else x.ctypes.data
    count = b.count if (explicit or (b.count != b.G).any()) else None
    assert hs.hsc_chain_solve(b.C, b.G, b.S, b.F, p(b.first if explicit else None), p(count), p(b.ffirst if explicit else None), p(b.hess),
                              p(b.prior if with_prior else None), p(lam), int(diagonal), p(delta), p(status), p(ws)) == 0
    return delta, status


def test_twin_metrics_against_the_reference(lib, hs):
    worst_a = worst_b = lap_a = lap_b = 0.0
    print("| layout | prior | damping | cond max | (a) twin | (b) twin | (a) LAPACK | (b) LAPACK |")
    for name, (counts, layout) in cc.LAYOUTS.items():
        for prior_all in (False, True):
            b = cc.Batch(counts, seed=3, prior_all=prior_all, layout=layout)
            for dname, lam_v, diagonal in cc.DAMPINGS:
                lam = cc.lam_of(b, lam_v)
                ref = cc.Reference(b, lam, diagonal)
                ref.check_inputs()                                            # a condition on the inputs, before anything is compared
                delta, status = host_solve(hs, b, lam, diagonal)
                a, bb = ref.metrics(delta)
                la, lb = ref.lapack_metrics()
                print("| %s | %s | %s | %.1e | %.2e | %.2e | %.2e | %.2e |" % (name, "all" if prior_all else "first", dname, ref.cond.max(), a, bb, la, lb))
                assert (status == 0).all(), (name, status)
                untouched = np.ones(b.S, dtype=bool)
                for c in range(b.C):
                    untouched[b.rows(c)] = False
                assert (delta[untouched] == -7.0).all(), name                 # rows of no chain are not written
                worst_a, worst_b, lap_a, lap_b = max(worst_a, a), max(worst_b, bb), max(lap_a, la), max(lap_b, lb)
    print("largest: twin (a) %.3e (b) %.3e; LAPACK (a) %.3e (b) %.3e; gates (a) %.2e (b) %.2e"
          % (worst_a, worst_b, lap_a, lap_b, cc.GATE_BACKWARD_HOST, cc.GATE_FORWARD_HOST))
    assert worst_a <= cc.GATE_BACKWARD_HOST and worst_b <= cc.GATE_FORWARD_HOST


def test_twin_many_chains_and_failures(hs):
    b = cc.Batch([5] * 1000, seed=5)
    ref = cc.Reference(b)
    ref.check_inputs()
    delta, status = host_solve(hs, b, None, False)
    a, bb = ref.metrics(delta)
    print("C = 1000, G = 5: twin (a) %.3e (b) %.3e" % (a, bb))
    assert (status == 0).all() and a <= cc.GATE_BACKWARD_HOST and bb <= cc.GATE_FORWARD_HOST
    # an indefinite block at state 3 of chain 4 and an ffirst out of range: status 4 / -1, NaN rows, the neighbours bit for bit
    r = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
    good, _ = host_solve(hs, r, None, False)
    r.prior[r.first[4] + 3, 2 + 2 * 3 // 2] = -1e9                           # entry (2, 2) of the state's prior block
    r.ffirst[6] = r.F - 1
    bad, status = host_solve(hs, r, None, False)
    assert status[4] == 4 and status[6] == -1 and [int(s) for k, s in enumerate(status) if k not in (4, 6)] == [0] * 9
    assert np.isnan(bad[r.rows(4)]).all() and np.isnan(bad[r.rows(6)]).all()
    for c in range(r.C):
        if c not in (4, 6):
            assert np.array_equal(bad[r.rows(c)], good[r.rows(c)]), c


def test_twin_without_a_prior(hs):
    """prior == NULL: the blocks are the factors' alone (singular without damping: the chain is free to move as a whole), identity
    damping makes them definite; a chain of one state is then lambda delta = 0."""
    b = cc.Batch(cc.RAGGED, seed=3)
    lam = cc.lam_of(b, 3.0)
    ref = cc.Reference(b, lam, False, with_prior=False)
    ref.check_inputs()
    delta, status = host_solve(hs, b, lam, False, with_prior=False)
    a, bb = ref.metrics(delta)
    print("no prior, identity damping: cond max %.1e, twin (a) %.3e (b) %.3e" % (ref.cond.max(), a, bb))
    assert (status == 0).all() and a <= cc.GATE_BACKWARD_HOST and bb <= cc.GATE_FORWARD_HOST
    for c in range(b.C):
        if b.count[c] == 1:
            assert (delta[b.rows(c)] == 0.0).all(), c


def test_the_reference_step_lowers_the_cost_of_the_device_hess_case():
    """What tests/test_gpu_chain.py asks of the device's own hess, settled here first on the restatement of tests/factor_cases.py: the
    chains of tests/chain_pipeline.py linearised with hessian_longdouble, solved by the reference, retracted -- the whitened cost
    falls.  This ties the SIGN of delta to the factors (hess holds g = A^T b with b = -R e; the step is +delta)."""
    from tests import chain_pipeline as cp
    r = cp.cpu_case()
    print("cond max %.1e: cost before %.6e, after the reference step %.6e" % (r["cond"], r["before"], r["after"]))
    assert r["after"] < 1e-3 * r["before"]


# ---------------------------------------------------------------- the edges of the contract, on the twin first
def _bind(path):
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.hsc_chain_solve.argtypes = [C.c_longlong] * 4 + [vp] * 6 + [C.c_int, vp, vp, vp]
    return lib


def twin_run(hs):
    """run(call) of tests/chain_edge_checks.py on the solve's twin.  hess gets one more row of NaN behind its F rows: a twin whose range
    rule is a row too lax (the mutants below) reads that instead of memory that is not the test's."""
    def run(call, status_in=None):
        b = call.b
        p = lambda x: None if x is None else x.ctypes.data
        delta = np.full((b.S, 15), ck.SENTINEL)
        status = np.full(call.C, 99, dtype=np.int32)
        ws = np.full(max(call.S, 1) * hs.hsc_ws_doubles(), np.nan)
        hess = np.concatenate([b.hess, np.full((1, 496), np.nan)])
        assert hs.hsc_chain_solve(call.C, call.G, call.S, b.F, p(call.first), p(call.count), p(call.ffirst), p(hess),
                                  p(b.prior if call.with_prior else None), p(call.lam), int(call.diagonal), p(delta), p(status), p(ws)) == 0
        return ck.Result(delta, status)
    return run


def test_twin_status_names_the_state_of_the_first_failure(hs):
    ck.check_failure_plan(twin_run(hs))


def test_twin_nan_in_the_inputs(hs):
    ck.check_nan_plan(twin_run(hs))


def test_twin_refusal_boundary_of_ffirst(hs):
    ck.check_ffirst_boundaries(twin_run(hs))


def test_twin_ffirst_null_with_an_explicit_first(hs):
    ck.check_ffirst_null(twin_run(hs))


def test_twin_clamps_of_first_count_G_and_S(hs):
    ck.check_clamps(twin_run(hs))


def test_twin_a_wavefront_of_empty_chains(hs):
    ck.check_empty_wave(twin_run(hs), cc.GATE_BACKWARD_HOST, cc.GATE_FORWARD_HOST)


def test_twin_a_zero_block_is_a_failed_pivot(hs):
    ck.check_zero_pivot(twin_run(hs))


def test_twin_long_chain_beside_short_ones(hs):
    b, ref = cc.long_case()
    r = twin_run(hs)(cc.Call(b, count=b.count))
    a, bb = ref.metrics(r.delta)
    print("LONG %s: cond max %.1e, twin (a) %.3e (b) %.3e" % (cc.LONG, ref.cond.max(), a, bb))
    assert r.status.tolist() == [0] * 4 and a <= cc.GATE_BACKWARD_HOST and bb <= cc.GATE_FORWARD_HOST
    ck.unowned(r, cc.Call(b, count=b.count))


@pytest.mark.parametrize("e", cc.SCALED_EXPONENTS)
def test_twin_scaled_by_a_power_of_two(hs, e):
    _, ref = cc.scaled_reference()
    b = cc.scaled_batch(e)
    r = twin_run(hs)(cc.Call(b, count=b.count))
    a, bb = ref.metrics(r.delta)
    print("hess, prior x 2^%d: cond max %.1e, twin (a) %.3e (b) %.3e" % (e, ref.cond.max(), a, bb))
    assert (r.status == 0).all() and a <= cc.GATE_BACKWARD_HOST and bb <= cc.GATE_FORWARD_HOST


def test_twin_diagonal_damping_without_a_prior(hs):
    b, lam, ref = cc.no_prior_diagonal_case()
    r = twin_run(hs)(cc.Call(b, count=b.count, lam=lam, diagonal=True, with_prior=False))
    a, bb = ref.metrics(r.delta)
    print("no prior, diagonal damping 0.25: cond max %.1e, twin (a) %.3e (b) %.3e" % (ref.cond.max(), a, bb))
    assert (r.status == 0).all() and a <= cc.GATE_BACKWARD_HOST and bb <= cc.GATE_FORWARD_HOST


# the rules the edge tests are there for, each broken in a copy of the twin: (file, old, new, the check that must notice)
MUTANTS = {
    "the ffirst range one row too lax": ("tests/hostsim/hostsim_chain.cpp", "ff > F - (n - 1)", "ff > F - (n - 2)", ck.check_ffirst_boundaries),
    "the last failure wins": ("cpi_amd/csrc/cpi_math.hpp", "if (!factor_block(A) && status == 0) status = s + 1;",
                              "if (!factor_block(A)) status = s + 1;", ck.check_failure_plan),
    "ffirst NULL is the tile rule": ("tests/hostsim/hostsim_chain.cpp", "ffirst[c] : f - c;", "ffirst[c] : c * (G - 1);", ck.check_ffirst_null),
    "count is not clamped to G": ("tests/hostsim/hostsim_chain.cpp", "n = n < 0 ? 0 : (n > G ? G : n);", "n = n < 0 ? 0 : n;",
                                  lambda run: ck.check_clamps(run, only="G = 17")),
}


@pytest.mark.parametrize("what", list(MUTANTS))
def test_a_broken_rule_fails_its_edge_test(hs, tmp_path, what):
    """Do the edge tests bite?  The twin with one rule of the contract broken, built in tmp_path, fails the check that states the rule
    (every access of these mutants stays inside the arrays: see twin_run), and the twin as it is passes it."""
    rel, old, new, check = MUTANTS[what]
    files = {"tests/hostsim/hostsim_chain.cpp": open(_SRC).read(), "cpi_amd/csrc/cpi_math.hpp": open(_HDRS[0]).read()}
    assert files[rel].count(old) == 1, old
    files[rel] = files[rel].replace(old, new)
    for name, text in files.items():
        os.makedirs(tmp_path / os.path.dirname(name), exist_ok=True)
        (tmp_path / name).write_text(text)
    out = str(tmp_path / "libmutant.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out,
                           str(tmp_path / "tests/hostsim/hostsim_chain.cpp")])
    check(twin_run(hs))
    with pytest.raises(AssertionError):
        check(twin_run(_bind(out)))
