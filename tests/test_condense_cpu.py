"""CPU: cpi_chain_condense_batch / cpi_chain_expand_batch without a GPU -- declarations, contract, and the arithmetic.

1. Declarations: the entries are exported, declared in include/cpi_amd.h with their exact argument lists, listed among the additions
   within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_condense has a resource report of its own, no other report names its
   kernels, they use no scratch; the solve's and the marginalize unit do not include it; Engine, the module and the C++ facade have
   the entries.
2. The contract through ctypes: every refusal comes before the context is looked at, so a NULL context shows code and text.
3. The host twin (tests/hostsim/hostsim_condense.cpp over chn::condense_segment / condense_separator / expand_segment of cpi_math.hpp,
   compiled with -ffp-contract=off) against the longdouble references of tests/condense_cases.py on every case; the metrics are
   printed first.  K = 1 copies; rows the twin must not read are NaN (cc.Batch); a failed interior fails its segment and its chain
   alone; a wrong entry of a reduced row fails the gates."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import condense_cases as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_condense.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_condense.so")
_MATH = os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")

_CONDENSE = ("cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count, const int64_t *ffirst, "
             "const double *hess, const double *prior, const double *lambda, int32_t damping, int64_t K, double *rhess, double *rprior, "
             "int32_t *rcount, int32_t *status, double *%s")
_EXPAND = ("cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, const int64_t *first, const int32_t *count, int64_t K, const double *rdelta, "
           "const double *workspace, double *delta")
DECLS = {"cpi_chain_condense_batch": _CONDENSE % "workspace", "cpi_chain_condense_batch_host": _CONDENSE % "workspace_out",
         "cpi_chain_expand_batch": _EXPAND, "cpi_chain_expand_batch_host": _EXPAND}


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
    assert "int64_t cpi_chain_condense_states(int64_t G, int64_t K);" in flat
    assert "size_t cpi_chain_condense_workspace_doubles(int64_t S);" in flat
    assert lib.cpi_abi_version() == 3
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    for s in list(DECLS) + ["cpi_chain_condense_states", "cpi_chain_condense_workspace_doubles"]:
        assert s in within3, s
    doc = flat.split("int64_t cpi_chain_condense_states(")[0].rsplit("/*", 1)[1]
    for text in ("PARITY UNPINNED", "Schur complement", "bit for bit", "lambda = NULL", "Entry 135".lower(), "Out of scope", "recursion",
                 "per segment", "585 doubles", "capturable", "overlaps", "WITHOUT the Schur term"):
        assert text in doc, text
    assert flat.index("int cpi_chain_marginalize_batch(") < flat.index("int cpi_chain_condense_batch(") < flat.index("/* ---- Device sets")
    assert "\n## 3s." in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "3.5h" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_layout_functions(lib):
    for G in (0, 1, 2, 3, 5, 21, 100, 549):
        for K in (1, 2, 4, 7, 12, 23, 1000):
            assert lib.cpi_chain_condense_states(G, K) == cd.reduced_states(G, K), (G, K)
    assert lib.cpi_chain_condense_states(549, 23) == 25
    assert lib.cpi_chain_condense_workspace_doubles(10) == 5850 and lib.cpi_chain_condense_workspace_doubles(0) == 1


def test_kernels_have_a_unit_and_a_report_of_their_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_condense"][-4:] == ["cpi_condense.hip", "cpi_factor_kernels.hpp", "cpi_chain_util.hpp", "cpi_condense_kernels.hpp"]
    for other in ("cpi_chain", "cpi_marginalize", "cpi_marginals"):
        assert "cpi_condense_kernels.hpp" not in build.UNITS[other]
    unit = open(os.path.join(build.CSRC, "cpi_condense.hip")).read() + open(os.path.join(build.CSRC, "cpi_condense_kernels.hpp")).read()
    assert '#include "cpi_chain_kernels.hpp"' not in unit and '#include "cpi_chain_util.hpp"' in unit
    for helper in ("chain_pivot_step<0>(a, j, fail)", "chain_w(a, u)", "chain_w(a, v)", "chain_schur(nxt, u)", "chain_range(A,"):
        assert helper in unit, helper
    own = build.UNIT_REPORTS["cpi_condense"]
    assert os.path.basename(own) == "resource_usage_condense.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == ["cpi_condense_kernel", "cpi_expand_kernel"]
    for name, (regs, scratch, occ, lds) in rows.items():
        print("%s: %d registers, scratch %d, occupancy %d, LDS %d" % (name, regs, scratch, occ, lds))
        assert scratch == 0 and regs <= 256 and occ >= 2, name
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        text = open(path).read()
        assert (("cpi_condense_kernel" in text) or ("cpi_expand_kernel" in text)) == (unit == "cpi_condense"), path
    body = open(_MATH).read().split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    for sig in ("CPI_HD int condense_segment(int nf, const double *hess, const double *prior, double lam, int diagonal, double *ws, double *out)",
                "CPI_HD void condense_separator(", "CPI_HD void expand_segment(int nf, const double *ws, const double *da, const double *db, double *delta)"):
        assert sig in body, sig


def test_engine_module_and_facade_have_the_entries():
    import cpi_amd
    E = cpi_amd.Engine
    for fn, sym in ((E.chain_condense, "cpi_chain_condense_batch("), (E.chain_condense_host, "cpi_chain_condense_batch_host("),
                    (E.chain_expand, "cpi_chain_expand_batch("), (E.chain_expand_host, "cpi_chain_expand_batch_host(")):
        assert sym in inspect.getsource(fn), sym
    src = inspect.getsource(E.chain_solve_segmented)
    assert src.index("self.chain_condense(") < src.index("self.chain_solve(") < src.index("self.chain_expand(")
    for name in ("chain_condense", "chain_expand", "chain_solve_segmented"):
        assert callable(getattr(cpi_amd, name)), name
    host = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    for text in ("inline CondensedChains chain_condense(", "inline std::vector<double> chain_expand(", "inline std::vector<double> chain_solve_segmented("):
        assert text in host, text
    assert "chain_solve_segmented(ctx, C, G, K, hess, prior" in open(os.path.join(ROOT, "tests", "cpp", "test_condense.cpp")).read()


# ---------------------------------------------------------------- the contract, before the context is looked at
def _refused(lib, rc, text):
    assert rc == 1 and text in lib.cpi_last_error(None).decode(), (rc, lib.cpi_last_error(None))


def test_refusals_come_before_the_context(lib):
    Cn, G, K = 2, 5, 2
    Gr = cd.reduced_states(G, K)
    S, F = Cn * G, Cn * (G - 1)
    f64 = lambda n: np.zeros(max(n, 1))
    hess, prior, lam = f64(F * 496), f64(S * 136), f64(Cn)
    rh, rp, ws = f64(Cn * (Gr - 1) * 496), f64(Cn * Gr * 136), f64(S * 585)
    rc_, st = np.zeros(Cn, np.int32), np.zeros(Cn * (Gr - 1), np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def condense(C_=Cn, G_=G, S_=S, F_=F, hess_=hess, prior_=prior, lam_=lam, damping=0, K_=K, rh_=rh, rp_=rp, rc__=rc_, st_=st, ws_=ws, host=False):
        fn = lib.cpi_chain_condense_batch_host if host else lib.cpi_chain_condense_batch
        return fn(None, C_, G_, S_, F_, None, None, None, p(hess_), p(prior_), p(lam_), damping, K_, p(rh_), p(rp_), p(rc__), p(st_), p(ws_))

    _refused(lib, condense(C_=-1), "negative size")
    _refused(lib, condense(G_=0), "G (the longest chain in states) must be >= 1")
    _refused(lib, condense(G_=2 ** 31), "G exceeds")
    _refused(lib, condense(K_=0), "K (the factors of a segment) must be >= 1")
    _refused(lib, condense(damping=2), "damping must be")
    _refused(lib, condense(hess_=None), "hess is NULL")
    _refused(lib, condense(rh_=None), "rhess is NULL")
    _refused(lib, condense(rp_=None), "rprior is NULL")
    _refused(lib, condense(rc__=None), "rcount is NULL")
    _refused(lib, condense(ws_=None), "workspace is NULL")
    _refused(lib, condense(rh_=hess), "overlaps")
    _refused(lib, condense(rp_=prior), "overlaps")
    _refused(lib, condense(ws_=rh), "overlaps")
    _refused(lib, condense(), "ctx is NULL")
    _refused(lib, condense(ws_=None, host=True), "ctx is NULL")              # the host form wants no workspace
    assert condense(C_=0) == 1 and "ctx is NULL" in lib.cpi_last_error(None).decode()
    bad = np.array([0, 8], dtype=np.int64)                                   # chain 1: states 8 .. 12 leave [0, 10)
    rc = lib.cpi_chain_condense_batch_host(None, Cn, G, S, F, p(bad), None, None, p(hess), p(prior), None, 0, K, p(rh), p(rp), p(rc_), p(st), None)
    _refused(lib, rc, "the states of chain 1 leave")

    rd, delta = f64(Cn * Gr * 15), f64(S * 15)

    def expand(C_=Cn, G_=G, S_=S, K_=K, rd_=rd, ws_=ws, d_=delta, first=None, host=False):
        fn = lib.cpi_chain_expand_batch_host if host else lib.cpi_chain_expand_batch
        return fn(None, C_, G_, S_, p(first), None, K_, p(rd_), p(ws_), p(d_))

    _refused(lib, expand(S_=-1), "negative size")
    _refused(lib, expand(G_=0), "G (the longest chain in states) must be >= 1")
    _refused(lib, expand(K_=0), "K (the factors of a segment) must be >= 1")
    _refused(lib, expand(rd_=None), "rdelta is NULL")
    _refused(lib, expand(ws_=None), "workspace is NULL")
    _refused(lib, expand(d_=None), "delta is NULL")
    _refused(lib, expand(d_=rd), "overlaps")
    _refused(lib, expand(d_=ws), "overlaps")
    _refused(lib, expand(), "ctx is NULL")
    _refused(lib, expand(first=bad, host=True), "the states of chain 1 leave")


# ---------------------------------------------------------------- the host twin
@pytest.fixture(scope="module")
def twin():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(_MATH)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", _SRC, "-o", _LIB])
    return C.CDLL(_LIB)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_twin(twin, b, K, lam, diagonal, with_prior=True):
    """condense -> the solve's restatement on the reduced chains -> expand, on the arrays of batch b; everything numpy."""
    LL = C.c_longlong
    Gr = cd.reduced_states(b.G, K)
    first, ffirst = (b.first, b.ffirst) if b.explicit else (None, None)
    hess, prior = np.ascontiguousarray(b.hess), (np.ascontiguousarray(b.prior) if with_prior else None)
    lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
    res = dict(rhess=np.full((b.C * (Gr - 1), 496), cd.SENTINEL), rprior=np.full((b.C * Gr, 136), cd.SENTINEL), rcount=np.full(b.C, 99, np.int32),
               seg_status=np.full(b.C * (Gr - 1), 99, np.int32), status=np.full(b.C, 99, np.int32), delta=np.full((b.S, 15), cd.SENTINEL),
               rdelta=np.full((b.C * Gr, 15), cd.SENTINEL), workspace=np.full(max(b.S, 1) * 585, np.nan))
    assert twin.hsc_chain_condense(LL(b.C), LL(b.G), LL(b.S), LL(b.F), _p(first), _p(b.count), _p(ffirst), _p(hess), _p(prior), _p(lam),
                                   int(diagonal), LL(K), _p(res["rhess"]), _p(res["rprior"]), _p(res["rcount"]), _p(res["seg_status"]),
                                   _p(res["workspace"])) == 0
    assert twin.hsc_chain_solve(LL(b.C), LL(Gr), LL(b.C * Gr), LL(b.C * (Gr - 1)), None, _p(res["rcount"]), None, _p(res["rhess"]), _p(res["rprior"]),
                                None, 0, _p(res["rdelta"]), _p(res["status"])) == 0
    assert twin.hsc_chain_expand(LL(b.C), LL(b.G), LL(b.S), _p(first), _p(b.count), LL(K), _p(res["rdelta"]), _p(res["workspace"]), _p(res["delta"])) == 0
    return res


WORST = np.zeros(4)


@pytest.mark.parametrize("name,k", cd.all_cases())
def test_twin_against_the_longdouble_references(twin, name, k):
    case = cd.case(name, k)
    res = run_twin(twin, case.batch, case.K, case.lam, case.diagonal, case.with_prior)
    WORST[:] = np.maximum(WORST, case.check(res, cd.GATES_HOST))
    print("largest so far: (a) %.3e (b) %.3e (r) %.3e (c) %.3e; gates %s" % (*WORST, cd.GATES_HOST))
    b, Gr = case.batch, case.Gr
    for c in range(b.C):                                                     # rows of reduced slots beyond m_c are not written
        m = cd.reduced_states(int(b.count[c]), case.K)
        assert (res["rprior"][c * Gr + m:(c + 1) * Gr] == cd.SENTINEL).all()
        assert (res["rhess"][c * (Gr - 1) + max(m - 1, 0):(c + 1) * (Gr - 1)] == cd.SENTINEL).all()


def test_k1_copies_the_rows(twin):
    b = cc.Batch(cd.counts_for(4), seed=3, layout="gaps")
    res = run_twin(twin, b, 1, None, False)
    Gr = b.G
    for c in range(b.C):
        n = int(b.count[c])
        assert np.array_equal(res["rhess"][c * (Gr - 1):c * (Gr - 1) + max(n - 1, 0)].view(np.int64), b.chain(c)[0].view(np.int64))
        want = b.chain(c)[1].copy()
        want[:, 135] = 0.0
        assert np.array_equal(res["rprior"][c * Gr:c * Gr + n], want)
    assert res["rcount"].tolist() == b.count.tolist()


def test_a_failed_interior_fails_its_segment_and_its_chain_alone(twin):
    good, bad, K, chain, slot, code = cd.failure_plan()
    r0, r1 = run_twin(twin, good, K, None, False), run_twin(twin, bad, K, None, False)
    Gr = cd.reduced_states(good.G, K)
    want = np.zeros(good.C * (Gr - 1), np.int32)
    want[chain * (Gr - 1) + slot] = code
    assert np.array_equal(r1["seg_status"], want) and (r0["seg_status"] == 0).all()
    assert np.isnan(r1["rhess"][chain * (Gr - 1) + slot]).all()
    assert (r1["status"] != 0).tolist() == [c == chain for c in range(good.C)]
    assert np.isnan(r1["delta"][good.rows(chain)]).all()
    others = np.ones(good.S, dtype=bool)
    others[good.rows(chain)] = False
    assert np.array_equal(r1["delta"][others], r0["delta"][others])


def test_a_wrong_entry_of_a_reduced_row_fails_the_gates():
    case = cd.case("k4_tile", 0)
    Gr = case.Gr
    rh = np.stack([cc.pack_upper(np.asarray(case.rows.get((c, j), np.zeros((31, 31))), dtype=np.float64)) for c in range(case.batch.C) for j in range(Gr - 1)])
    assert case.rows_metric(rh) <= cd.GATES_HOST[3]
    c, j = next(k for k in case.rows if case.cond[k] > 1.0)
    rh[c * (Gr - 1) + j, cc.tri(20) + 3] *= 1.0 + 1e-6
    assert case.rows_metric(rh) > cd.GATES_HOST[3]
