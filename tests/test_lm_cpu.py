"""CPU: the Levenberg-Marquardt step per chain without a GPU -- declarations, contract, and the arithmetic.

1. cpi_prior_relinearize_batch, cpi_chain_cost_batch, cpi_chain_accept_batch and their _host forms are declared in include/cpi_amd.h
   between cpi_chain_marginalize_batch and the device sets, listed among the additions within ABI 3 and bound in cpi_amd/_lib.py; the
   unit cpi_lm has a resource report of its own with exactly its three kernels, scratch 0, and no other report names them.
2. Every refusal and every forbidden overlap, through ctypes with a NULL context: the refusals come before the context is looked at.
3. The host twin (tests/hostsim/hostsim_lm.cpp over chn::prior_relinearize / chain_cost / lm_decide of cpi_math.hpp, compiled with
   -ffp-contract=off): bit for bit against the float64 restatements of tests/lm_cases.py, within the gates of the longdouble references.
4. Mutations of the twin, built in tmp_path, that must fail: eta0 with the wrong sign, <= for < in the accept test, a butterfly stride
   dropped, lambda raised on accept.
5. The rule table of chain_accept on the twin, one chain per rule.
6. The edges that tests/test_gpu_lm_edges.py runs on the device, settled on the twin first: lc.hard_prior_case against the reference,
   and lc.RULES_EDGE -- the rule's equalities and infinities and chains around the copy loop's trip --, which a twin with < in place
   of <= at lam_max fails while it still passes the table of RULES.
The figures are printed before anything is asserted (pytest -s shows them; profiles/chain_lm.md records them)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import lm_cases as lc
from tests import test_marginals_cpu as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_lm.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_lm.so")
_MATH = os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")
KERNELS = ["cpi_lm_accept_kernel", "cpi_lm_cost_kernel", "cpi_lm_prior_kernel"]

_CHAINS = "cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count, const int64_t *ffirst, "
_PRIOR = ("cpi_ctx *ctx, int64_t S, int64_t P, const int32_t *idx, const double *states, const double *anchor, const double *prior0, "
          "double *prior, double *pcost")
_COST = _CHAINS + "const double *chi2, const double *pcost, double *cost"
_ACCEPT = _CHAINS + ("const cpi_lm_params *params, const double *chi2_new, const double *pcost_new, const double *trial, double *cost, "
                     "double *states, double *chi2, double *lambda, int32_t *phase, int32_t *accepted")
DECLS = {"cpi_prior_relinearize_batch": _PRIOR, "cpi_prior_relinearize_batch_host": _PRIOR, "cpi_chain_cost_batch": _COST,
         "cpi_chain_cost_batch_host": _COST, "cpi_chain_accept_batch": _ACCEPT, "cpi_chain_accept_batch_host": _ACCEPT}


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
    assert lib.cpi_abi_version() == 3
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    for s in DECLS:
        assert s in within3, s
    assert "global: cpi_*;" in open(os.path.join(build.CSRC, "exports.map")).read()
    assert (flat.index("int cpi_chain_marginalize_batch(") < flat.index("int cpi_prior_relinearize_batch(") < flat.index("int cpi_chain_cost_batch(")
            < flat.index("int cpi_chain_accept_batch(") < flat.index("/* ---- Device sets"))
    assert "typedef struct { double lam_down, lam_up, lam_min, lam_max, abs_tol, rel_tol; } cpi_lm_params;" in flat
    assert "enum { CPI_LM_RUNNING = 0, CPI_LM_CONVERGED = 1, CPI_LM_GAVE_UP = 2 };" in flat
    doc = flat.split("int cpi_chain_marginalize_batch(")[1].split("int cpi_chain_accept_batch(")[0]
    for text in ("PARITY UNPINNED", "LevenbergMarquardtParams", "{ 0.1, 10, 0, 1e5, 1e-5, 1e-5 }", "STARTING FROM eta0_i", "entry 135 is never read", "entry 135 as 0.0",
                 "v_q = v_q + v_{q ^ 8}", "false for any NaN", "CPI_LM_GAVE_UP", "allocates nothing", "without parallel branches", "overlaps",
                 "before the context is looked at", "not on C, P or its position"):
        assert text in doc, text
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## 3p." in integ
    sec = integ.split("\n## 3p.", 1)[1].split("\n## ", 1)[0]
    for text in ("prior_relinearize", "chain_cost", "chain_accept", "chain_lm", "phase"):
        assert text in sec, text
    for part in ("\n## 3m.", "\n## 3o."):
        assert "3p" in integ.split(part, 1)[1].split("\n## ", 1)[0], part


def test_kernels_have_a_unit_and_a_report_of_their_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_lm"][-4:] == ["cpi_lm.hip", "cpi_factor_kernels.hpp", "cpi_chain_util.hpp", "cpi_lm_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_lm"]
    assert os.path.basename(own) == "resource_usage_lm.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == KERNELS
    for k in KERNELS:
        regs, scratch, occ, lds = rows[k]
        print("%s: %d registers, scratch %d, occupancy %d, LDS %d" % (k, regs, scratch, occ, lds))
        assert scratch == 0 and regs <= 128 and occ >= 4
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        text = open(path).read()
        for k in KERNELS:
            assert (k in text) == (unit == "cpi_lm"), (path, k)
        assert ("cpi_chain_" in text) == (unit == "cpi_chain"), path
    body = open(_MATH).read().split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    for sig in ("CPI_HD double prior_eta_row(const double *P0, const double *xi, int i)", "CPI_HD double prior_cost(const double *xi, const double *t)",
                "CPI_HD double chain_cost(int n, const double *chi2, const double *pcost)",
                "CPI_HD int lm_decide(double cur, double nw, const LmParams &p, double &lambda, int &phase)"):
        assert sig in body, sig
    kern = open(os.path.join(build.CSRC, "cpi_lm_kernels.hpp")).read()
    for call in ("chn::prior_eta_row(", "chn::prior_cost(", "chn::chain_cost_slot(", "chn::lm_decide(", "chain_range(A, c)", "local_coordinates("):
        assert call in kern, call
    twin = open(_SRC).read()
    for call in ("chn::prior_relinearize(", "chn::chain_cost(", "chn::lm_decide(", "local_coordinates("):
        assert call in twin, call


def test_engine_module_and_facade_have_the_entries():
    import cpi_amd
    E = cpi_amd.Engine
    for fn, sym in ((E.prior_relinearize, "cpi_prior_relinearize_batch"), (E.prior_relinearize_host, "cpi_prior_relinearize_batch_host"),
                    (E.chain_cost, "cpi_chain_cost_batch"), (E.chain_cost_host, "cpi_chain_cost_batch_host"),
                    (E.chain_accept, "cpi_chain_accept_batch"), (E.chain_accept_host, "cpi_chain_accept_batch_host")):
        assert "self.lib.%s," % sym in inspect.getsource(fn), sym
    assert "_chain_ranges" in inspect.getsource(E._chain_args) and "_chain_ranges" in inspect.getsource(E._lm_sizes)
    src = inspect.getsource(E.chain_lm)
    src = src[src.index("for it in range(iterations)"):]
    order = [src.index(s) for s in ("for it in range(iterations)", "self.prior_relinearize(states", "self.factor_hessian(", "self.chain_solve(", "self.retract(",
                                    "self.factor_cost(model, meas, lin, q_k_lin, b[\"trial\"]", "self.prior_relinearize(b[\"trial\"]", "self.chain_accept(")]
    assert order == sorted(order)
    for word in (".item()", ".cpu()", ".tolist()", "synchronize"):
        assert word not in src, word                                          # no host read
    p = inspect.signature(E.chain_lm).parameters
    assert list(p)[1:9] == ["model", "meas", "lin", "q_k_lin", "states", "R_tri", "C", "G"] and p["damping"].default == "diagonal"
    for name in ("prior0", "anchor", "prior_idx", "lam", "iterations", "params"):
        assert name in p, name
    for name in ("prior_relinearize", "chain_cost", "chain_accept", "chain_lm"):
        assert callable(getattr(cpi_amd, name)), name
    host = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    for sym, fn in (("cpi_prior_relinearize_batch_host(", r"inline PriorRows prior_relinearize\(const Context &ctx"),
                    ("cpi_chain_cost_batch_host(", r"inline std::vector<double> chain_cost\(const Context &ctx"),
                    ("cpi_chain_accept_batch_host(", r"inline std::vector<int32_t> chain_accept\(const Context &ctx")):
        assert sym in host and re.search(fn, host), sym
    prog = open(os.path.join(ROOT, "tests", "cpp", "test_lm.cpp")).read()
    for call in ("prior_relinearize(ctx, states, anchor, prior0, idx)", "chain_cost(ctx, C, G, chi2, pr.pcost)", "chain_accept(ctx, C, G, chi2_new, pr.pcost, trial, st)"):
        assert call in prog, call


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


def _ptr(x, off=0):
    return None if x is None else x.ctypes.data + off


def _refuser(lib, entry, call):
    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)
    return refused


@pytest.mark.parametrize("entry", ["cpi_prior_relinearize_batch", "cpi_prior_relinearize_batch_host"])
def test_prior_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    S, P = 6, 4
    a = {"idx": np.arange(P, dtype=np.int32), "states": np.zeros(S * 16), "anchor": np.zeros(P * 16), "prior0": np.zeros(P * 136),
         "prior": np.zeros(S * 136), "pcost": np.zeros(S)}

    def call(S_=S, P_=P, **kw):
        v = {k: _ptr(x) for k, x in a.items()}
        v.update(kw)
        return f(None, S_, P_, v["idx"], v["states"], v["anchor"], v["prior0"], v["prior"], v["pcost"]), _err(lib)

    refused = _refuser(lib, entry, call)
    assert call() == (1, "ctx is NULL")                                       # a valid call gets as far as the context
    assert call(idx=None) == (1, "ctx is NULL") and call(prior=None) == (1, "ctx is NULL") and call(pcost=None) == (1, "ctx is NULL")
    assert call(S_=2) == (1, "ctx is NULL")                                   # P > S is fine with an idx
    refused("negative size", S_=-1)
    refused("negative size", P_=-1)
    refused("P > S with idx NULL", idx=None, S_=3)
    for k in ("states", "anchor", "prior0"):
        refused("NULL argument", **{k: None})
    assert call(S_=0, states=None) == (1, "ctx is NULL")                      # S == 0: every record is skipped, states is never read
    refused("prior and pcost are both NULL", prior=None, pcost=None)
    assert call(P_=0, states=None, anchor=None, prior0=None, prior=None, pcost=None)[0] == 1 and _err(lib) == "ctx is NULL"   # P == 0: nothing to refuse
    for o in ("prior", "pcost"):
        for i in ("idx", "states", "anchor", "prior0"):
            refused("overlaps", **{o: _ptr(a[i], a[i].nbytes - 4)})
            refused("overlaps", **{i: _ptr(a[o], 4)})
    refused("prior overlaps", pcost=_ptr(a["prior"], 8))
    refused("overlaps", prior=_ptr(a["pcost"], 0))


def _chain_arrays(Cn=4, G=3):
    S, F = Cn * G, Cn * (G - 1)
    return {"first": np.arange(Cn, dtype=np.int64) * G, "count": np.full(Cn, G, dtype=np.int32), "ffirst": np.arange(Cn, dtype=np.int64) * (G - 1),
            "chi2_new": np.zeros(F), "pcost_new": np.zeros(S), "trial": np.zeros(S * 16), "cost": np.zeros(Cn), "states": np.zeros(S * 16),
            "chi2": np.zeros(F), "lambda": np.ones(Cn), "phase": np.zeros(Cn, dtype=np.int32), "accepted": np.zeros(Cn, dtype=np.int32)}, S, F


def _sizes_refused(refused):
    for k in ("C_", "S_", "F_"):
        refused("negative size", **{k: -1})
    refused("G (the longest chain in states) must be >= 1", G_=0)
    refused("G exceeds 2^31 - 1", G_=2 ** 31)


@pytest.mark.parametrize("entry", ["cpi_chain_cost_batch", "cpi_chain_cost_batch_host"])
def test_cost_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    Cn, G = 4, 3
    a, S, F = _chain_arrays(Cn, G)

    def call(C_=Cn, G_=G, S_=S, F_=F, **kw):
        v = {k: _ptr(x) for k, x in a.items()}
        v.update(kw)
        return f(None, C_, G_, S_, F_, v["first"], v["count"], v["ffirst"], v["chi2_new"], v["pcost_new"], v["cost"]), _err(lib)

    refused = _refuser(lib, entry, call)
    assert call() == (1, "ctx is NULL")
    assert call(first=None, count=None, ffirst=None, pcost_new=None) == (1, "ctx is NULL")
    assert call(G_=1, F_=0, S_=Cn, chi2_new=None, first=None, ffirst=None, count=None) == (1, "ctx is NULL")   # chains of one state need no chi2
    _sizes_refused(refused)
    refused("chi2 is NULL", chi2_new=None)
    refused("cost is NULL", cost=None)
    for i in ("first", "count", "ffirst", "chi2_new", "pcost_new"):
        refused("cost overlaps", cost=_ptr(a[i], a[i].nbytes - 4))
        refused("cost overlaps", **{i: _ptr(a["cost"], 4)})


@pytest.mark.parametrize("entry", ["cpi_chain_accept_batch", "cpi_chain_accept_batch_host"])
def test_accept_refusals_come_before_the_context(lib, entry):
    from cpi_amd._lib import CpiLmParams
    f = getattr(lib, entry)
    Cn, G = 4, 3
    a, S, F = _chain_arrays(Cn, G)
    names = ("first", "count", "ffirst", "chi2_new", "pcost_new", "trial", "cost", "states", "chi2", "lambda", "phase", "accepted")

    def call(C_=Cn, G_=G, S_=S, F_=F, params=None, **kw):
        v = {k: _ptr(x) for k, x in a.items()}
        v.update(kw)
        p = None
        if params is not None:
            p = CpiLmParams(*[float(dict(lc.DEFAULTS, **params)[n]) for n in lc.PARAM_NAMES])
        return f(None, C_, G_, S_, F_, v["first"], v["count"], v["ffirst"], None if p is None else C.byref(p), *[v[n] for n in names[3:]]), _err(lib)

    refused = _refuser(lib, entry, call)
    assert call() == (1, "ctx is NULL")
    assert call(params={}) == (1, "ctx is NULL")
    assert call(first=None, count=None, ffirst=None, pcost_new=None, chi2=None, accepted=None) == (1, "ctx is NULL")
    assert call(params=dict(lam_down=1.0, lam_up=1.0, lam_min=0.0, lam_max=0.0, abs_tol=0.0, rel_tol=0.0)) == (1, "ctx is NULL")   # the edges are inside
    assert call(params=dict(lam_up=float("inf"), lam_max=float("inf"))) == (1, "ctx is NULL")
    _sizes_refused(refused)
    nan = float("nan")
    for bad in (dict(lam_down=0.0), dict(lam_down=-0.1), dict(lam_down=1.5), dict(lam_down=nan), dict(lam_up=0.5), dict(lam_up=nan)):
        refused("0 < lam_down <= 1 <= lam_up", params=bad)
    for bad in (dict(lam_min=-1.0), dict(lam_min=2e5), dict(lam_min=nan), dict(lam_max=nan), dict(lam_max=-1.0)):
        refused("0 <= lam_min <= lam_max", params=bad)
    for bad in (dict(abs_tol=-1e-9), dict(rel_tol=-1e-9), dict(abs_tol=nan), dict(rel_tol=nan)):
        refused("a tolerance is negative or NaN", params=bad)
    refused("params", params=dict(lam_down=nan), C_=0)                        # the parameters are looked at whatever C is
    for k in ("cost", "lambda", "phase"):
        refused("cost, lambda or phase is NULL", **{k: None})
    for k in ("states", "trial"):
        refused("states or trial is NULL", **{k: None})
    refused("chi2_new is NULL", chi2_new=None)
    inout = ("cost", "states", "chi2", "lambda", "phase", "accepted")
    for o in inout:                                                           # trial / chi2_new / pcost_new and the ranges against every in/out array
        for i in ("first", "count", "ffirst", "chi2_new", "pcost_new", "trial"):
            refused("overlaps", **{o: _ptr(a[i], a[i].nbytes - 4)})
            refused("overlaps", **{i: _ptr(a[o], 4)})
    for k, o in enumerate(inout):                                             # ... and the in/out arrays against each other
        for q in inout[k + 1:]:
            refused(("%s overlaps" % o), **{q: _ptr(a[o], 4)})


def test_host_forms_name_the_chain_whose_range_is_wrong(lib):
    Cn, G = 4, 3
    a, S, F = _chain_arrays(Cn, G)
    for entry in ("cpi_chain_cost_batch_host", "cpi_chain_accept_batch_host"):
        f = getattr(lib, entry)

        def refused(text, S_=S, F_=F, **kw):
            v = {k: _ptr(x) for k, x in a.items()}
            v.update({k: _ptr(x) for k, x in kw.items()})
            if entry == "cpi_chain_cost_batch_host":
                rc = f(None, Cn, G, S_, F_, v["first"], v["count"], v["ffirst"], v["chi2_new"], v["pcost_new"], v["cost"])
            else:
                rc = f(None, Cn, G, S_, F_, v["first"], v["count"], v["ffirst"], None, v["chi2_new"], v["pcost_new"], v["trial"], v["cost"], v["states"],
                       v["chi2"], v["lambda"], v["phase"], v["accepted"])
            msg = _err(lib)
            assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

        bad = a["ffirst"].copy()
        bad[2] = F - 1
        refused("the factor rows of chain 2 leave [0, F)", ffirst=bad)
        refused("the factor rows of chain 3 leave [0, F)", F_=F - 1)
        bad = a["first"].copy()
        bad[1] = S - 2
        refused("the states of chain 1 leave [0, S)", first=bad)
        refused("the states of chain 3 leave [0, S)", S_=S - 1)


# ---------------------------------------------------------------- host twin
def _bind(path):
    lib = C.CDLL(path)
    vp, ll = C.c_void_p, C.c_longlong
    lib.hsl_local.argtypes = [ll, vp, vp, vp]
    lib.hsl_prior_from_xi.argtypes = [ll, vp, vp, vp, vp]
    lib.hsl_prior_relinearize.argtypes = [ll, ll] + [vp] * 6
    lib.hsl_chain_cost.argtypes = [ll] * 4 + [vp] * 6
    lib.hsl_chain_accept.argtypes = [ll] * 4 + [vp] * 13
    return lib


@pytest.fixture(scope="module")
def hl():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in (_SRC, _MATH)):
        tm._build(_SRC, _LIB)
    return _bind(_LIB)


def _mutant(tmp_path, old, new):
    text = open(_MATH).read()
    assert text.count(old) == 1, old
    os.makedirs(tmp_path / "cpi_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "hostsim")
    (tmp_path / "cpi_amd" / "csrc" / "cpi_math.hpp").write_text(text.replace(old, new))
    shutil.copy(_SRC, tmp_path / "tests" / "hostsim" / "hostsim_lm.cpp")
    out = str(tmp_path / "libmutant.so")
    tm._build(str(tmp_path / "tests" / "hostsim" / "hostsim_lm.cpp"), out)
    return _bind(out)


def twin_prior(hl, S, idx, states, anchor, prior0, want_prior=True, want_cost=True):
    """hsl_prior_relinearize -> (prior [S, 136], pcost [S]) with sentinels wherever nothing is written (None where not asked for)."""
    prior = np.full((S, 136), lc.SENTINEL) if want_prior else None
    pcost = np.full(S, lc.SENTINEL) if want_cost else None
    i32 = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    assert hl.hsl_prior_relinearize(S, len(anchor), _ptr(i32), _ptr(states), _ptr(anchor), _ptr(prior0), _ptr(prior), _ptr(pcost)) == 0
    return prior, pcost


def twin_cost(hl, call, chi2, pcost):
    b = call.b
    cost = np.full(call.C + 1, lc.SENTINEL)
    assert hl.hsl_chain_cost(call.C, call.G, call.S, b.F, _ptr(call.first), _ptr(call.count), _ptr(call.ffirst), _ptr(chi2), _ptr(pcost), _ptr(cost)) == 0
    assert cost[call.C] == lc.SENTINEL
    return cost[:call.C]


def twin_accept(hl, case, with_chi2=True, with_accepted=True):
    """hsl_chain_accept on copies of the case's arrays -> (cost, states, chi2, lam, phase, accepted) as accept_expected gives them."""
    call, b = case.call, case.call.b
    cost, states, lam, phase = case.cost.copy(), case.states.copy(), case.lam.copy(), case.phase.copy()
    chi2 = case.chi2.copy() if with_chi2 else None
    acc = np.full(call.C, 99, dtype=np.int32) if with_accepted else None
    par = None if case.params is None else np.array([dict(lc.DEFAULTS, **case.params)[n] for n in lc.PARAM_NAMES])
    assert hl.hsl_chain_accept(call.C, call.G, call.S, b.F, _ptr(call.first), _ptr(call.count), _ptr(call.ffirst), _ptr(par), _ptr(case.chi2_new),
                               _ptr(case.pcost_new), _ptr(case.trial), _ptr(cost), _ptr(states), _ptr(chi2), _ptr(lam), _ptr(phase), _ptr(acc)) == 0
    return cost, states, chi2, lam, phase, acc


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_accept(got, want):
    for name, g, w in zip(("cost", "states", "chi2", "lambda", "phase", "accepted"), got, want):
        if g is None:
            continue
        assert same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), (name, g, w)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_twin_prior_against_the_restatement_and_the_reference(hl, S):
    states, anchor, prior0 = lc.prior_case(S)
    xi = np.zeros((S, 15))
    assert hl.hsl_local(S, _ptr(states), _ptr(anchor), _ptr(xi)) == 0
    prior, pcost = twin_prior(hl, S, None, states, anchor, prior0)
    rows, pc = lc.prior_documented(xi, prior0)
    assert same_bits(prior, rows) and same_bits(pcost, pc)                    # bit for bit the documented orders
    assert same_bits(prior[:, :120], prior0[:, :120]) and (prior[:, 135] == 0.0).all()
    at = np.arange(S) % 4 == 0                                                # a record at its anchor: prior0 with entry 135 zeroed, pcost 0
    assert (xi[at] == 0.0).all() and same_bits(prior[at, :135], prior0[at, :135]) and (pcost[at] == 0.0).all()
    m_eta, m_pc = lc.prior_metrics(prior, pcost, lc.oracle_local(states, anchor), prior0, skip=at)
    print("twin, S %d: eta %.3g units (gate %.0f), pcost %.3g units (gate %.0f)" % (S, m_eta, lc.GATE_ETA_HOST, m_pc, lc.GATE_PCOST_HOST))
    assert m_eta <= lc.GATE_ETA_HOST and m_pc <= lc.GATE_PCOST_HOST


def test_twin_prior_idx_outputs_and_nan(hl):
    S = 9
    states, anchor, prior0 = (x.copy() for x in lc.prior_case(S))
    full, full_pc = twin_prior(hl, S, None, states, anchor, prior0)
    idx = np.array([-1, 8, 6, 5, 3, 1, S], dtype=np.int32)                    # reverse order, skipped at either end, states without a record
    sub = idx[1:-1]
    an, p0 = np.zeros((7, 16)), np.zeros((7, 136))
    an[1:-1], p0[1:-1] = anchor[sub], prior0[sub]
    an[0] = an[-1] = p0[0] = p0[-1] = np.nan                                  # a skipped record is not read: NaN would show
    prior, pcost = twin_prior(hl, S, idx, states, an, p0)
    assert same_bits(prior[sub], full[sub]) and same_bits(pcost[sub], full_pc[sub])
    rest = np.setdiff1d(np.arange(S), sub)
    assert (prior[rest] == lc.SENTINEL).all() and (pcost[rest] == lc.SENTINEL).all()
    only_p, none = twin_prior(hl, S, idx, states, an, p0, want_cost=False)
    none2, only_c = twin_prior(hl, S, idx, states, an, p0, want_prior=False)
    assert none is None and none2 is None and same_bits(only_p, prior) and same_bits(only_c, pcost)
    states[5, 7] = np.nan                                                     # NaN in one record reaches that record's outputs only
    bad, bad_pc = twin_prior(hl, S, None, states, anchor, prior0)
    others = np.arange(S) != 5
    assert same_bits(bad[others], full[others]) and same_bits(bad_pc[others], full_pc[others])
    assert np.isnan(bad_pc[5]) and np.isnan(bad[5, 120:135]).any() and same_bits(bad[5, :120], prior0[5, :120])


def test_twin_cost_against_the_restatement_and_the_reference(hl):
    worst = 0.0
    for name, counts, layout in lc.COST_LAYOUTS:
        b = cc.Batch(counts, seed=3, layout=layout)
        call = lc.cost_call(b)
        for negative in (False, True):
            chi2, pcost = lc.cost_terms(b, negative=negative)
            for pc in (pcost, None):
                got = twin_cost(hl, call, chi2 if b.G > 1 else None, pc)
                assert same_bits(got, lc.chain_costs(call, chi2, pc)), name
                worst = max(worst, lc.cost_metric(got, call, chi2, pc))
            if negative:
                assert (twin_cost(hl, call, chi2, pcost)[b.count > 0] < 0).all(), name
        empty = b.count == 0
        zero = twin_cost(hl, call, chi2, pcost)[empty]
        assert (zero == 0.0).all() and not np.signbit(zero).any()             # a chain without states: +0.0
    print("twin, every layout: cost %.3g units (gate %.0f)" % (worst, lc.GATE_COST_HOST))
    assert worst <= lc.GATE_COST_HOST


def test_twin_cost_nan_refused_chain_and_position(hl):
    b = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
    call = cc.Call.explicit(b)
    chi2, pcost = lc.cost_terms(b)
    good = twin_cost(hl, call, chi2, pcost)
    bad2 = chi2.copy()
    bad2[b.ffirst[5] + 16] = np.nan                                           # chain 5 (40 states), slot 0, second trip
    got = twin_cost(hl, call, bad2, pcost)
    assert np.isnan(got[5]) and same_bits(np.delete(got, 5), np.delete(good, 5))
    out = cc.clone(b)
    out.ffirst[5] = b.F - 3                                                   # 39 rows from F - 3 on
    got = twin_cost(hl, cc.Call.explicit(out), chi2, pcost)
    assert np.isnan(got[5]) and same_bits(np.delete(got, 5), np.delete(good, 5))
    order = np.array([7, 3, 10, 4, 0, 5])                                     # other positions, another C: the same bits
    assert same_bits(twin_cost(hl, cc.Call.explicit(b, chains=order), chi2, pcost), good[order])


def test_twin_rule_table(hl):
    case, want = lc.rule_table()
    got = twin_accept(hl, case)
    for c, (rule, (acc, phase, lam)) in enumerate(zip(lc.RULES, want)):
        print("%-26s accepted %d phase %d lambda %g" % (rule[0], got[5][c], got[4][c], got[3][c]))
        assert (got[5][c], got[4][c], got[3][c]) == (acc, phase, lam), rule[0]
    check_accept(got, case.expected())
    # what each rule leaves of the chain's rows: the trial's where accepted, the sentinels everywhere else (rows of no chain included)
    moved = np.zeros(case.call.b.S, dtype=bool)
    for c, (f, n, ff, bad) in enumerate(lc.chain_ranges(case.call)):
        if want[c][0]:
            moved[f:f + n] = True
    assert same_bits(got[1][moved], case.trial[moved]) and same_bits(got[1][~moved], case.states[~moved])
    check_accept(twin_accept(hl, case, with_chi2=False, with_accepted=False), case.expected(with_chi2=False))


def test_twin_prior_on_the_hard_case(hl):
    """The honesty condition of lc.hard_prior_case: the twin against the restatement bit for bit and against the longdouble reference
    within the host gates, at GPS-sized positions, float32-rounded and scaled quaternions."""
    S = 65
    states, anchor, prior0 = lc.hard_prior_case(S)
    easy = lc.prior_case(S)
    assert np.abs(states[:, 13:16]).max() > 4e6 and np.array_equal(prior0, easy[2], equal_nan=True)
    n = np.linalg.norm(states[:, :4], axis=1)
    assert (np.abs(n[1::6] - 1) < 1e-7).all() and (n[1::6] != 1).any() and (np.abs(n[0::6] - 0.5) < 1e-7).all() and (np.abs(n[3::6] - 2) < 1e-6).all()
    xi = np.zeros((S, 15))
    assert hl.hsl_local(S, _ptr(states), _ptr(anchor), _ptr(xi)) == 0
    prior, pcost = twin_prior(hl, S, None, states, anchor, prior0)
    rows, pc = lc.prior_documented(xi, prior0)
    assert same_bits(prior, rows) and same_bits(pcost, pc)
    assert same_bits(prior[:, :120], prior0[:, :120]) and (prior[:, 135] == 0.0).all()
    at = np.arange(S) % 4 == 0
    m_eta, m_pc = lc.prior_metrics(prior, pcost, lc.oracle_local(states, anchor), prior0, skip=at)
    print("twin, the hard prior case, S %d: eta %.3g units (gate %.0f), pcost %.3g units (gate %.0f); at the anchor |xi| max %.3g"
          % (S, m_eta, lc.GATE_ETA_HOST, m_pc, lc.GATE_PCOST_HOST, np.abs(xi[at]).max()))
    assert m_eta <= lc.GATE_ETA_HOST and m_pc <= lc.GATE_PCOST_HOST


def test_twin_edge_rule_table(hl):
    """The equalities and infinities of the rule and the chains around the copy loop's trip (lc.RULES_EDGE): the triples as written
    there, the rows bit for bit and every sentinel around them."""
    case, want = lc.edge_rule_table()
    got = twin_accept(hl, case)
    for c, (rule, (acc, phase, lam)) in enumerate(zip(lc.RULES_EDGE, want)):
        print("%-28s accepted %d phase %d lambda %g cost %g" % (rule[0], got[5][c], got[4][c], got[3][c], got[0][c]))
        assert (got[5][c], got[4][c], got[3][c]) == (acc, phase, lam), rule[0]
    check_accept(got, case.expected())
    b = case.call.b
    for c in (6, 7, 8):                                                       # 16, 17 and 32 states: the trial's rows, the sentinels on either side
        rows = b.rows(c)
        assert same_bits(got[1][rows], case.trial[rows])
        assert same_bits(got[1][rows.start - 2:rows.start], case.states[rows.start - 2:rows.start])
        assert same_bits(got[1][rows.stop:rows.stop + 2], case.states[rows.stop:rows.stop + 2])


@pytest.mark.parametrize("layout", ["tile", "gaps", "reverse"])
def test_twin_accept_ragged(hl, layout):
    case = lc.ragged_accept_case(layout)
    got = twin_accept(hl, case)
    check_accept(got, case.expected())
    n = case.call.b.count
    assert got[5].tolist() == [int(c % 2 == 0 and c != 5 and n[c] > 0) for c in range(case.call.C)]
    assert same_bits(got[0][got[5] == 1], twin_cost(hl, case.call, case.chi2_new, case.pcost_new)[got[5] == 1])   # new is chain_cost's value


MUTATIONS = {
    "eta0 added with the wrong sign": ("t[i] = eta[i] + P0[tri(15) + i];", "t[i] = eta[i] - P0[tri(15) + i];"),
    "<= in place of < in the accept test": ("    if (nw < cur) {", "    if (nw <= cur) {"),
    "a butterfly stride dropped": ("for (int s = 8; s >= 1; s >>= 1) {\n        for (int q = 0; q < 16; q++) w[q]", "for (int s = 4; s >= 1; s >>= 1) {\n        for (int q = 0; q < 16; q++) w[q]"),
    "lambda raised on accept": ("const double l = lambda * p.lam_down;", "const double l = lambda * p.lam_up;"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_wrong_term_fails_its_gate(hl, tmp_path, what):
    """The twin with one term wrong, built in tmp_path: the numeric gates are left by orders of magnitude, the rule table is not met."""
    mutant = _mutant(tmp_path, *MUTATIONS[what])
    S = 65
    states, anchor, prior0 = lc.prior_case(S)
    xi = lc.oracle_local(states, anchor)
    b = cc.Batch(cc.RAGGED, seed=3)
    call = lc.cost_call(b)
    chi2, pcost = lc.cost_terms(b)
    case, _ = lc.rule_table()
    res = {}
    for name, h in (("twin", hl), ("mutant", mutant)):
        m_eta, m_pc = lc.prior_metrics(*twin_prior(h, S, None, states, anchor, prior0), xi, prior0, skip=np.arange(S) % 4 == 0)
        m_cost = lc.cost_metric(twin_cost(h, call, chi2, pcost), call, chi2, pcost)
        try:
            check_accept(twin_accept(h, case), case.expected())
            table = True
        except AssertionError:
            table = False
        res[name] = (m_eta, m_pc, m_cost, table)
        print("%s, %s: eta %.3g, pcost %.3g, cost %.3g units, the rule table holds: %s" % (what, name, m_eta, m_pc, m_cost, table))
    assert res["twin"][0] <= lc.GATE_ETA_HOST and res["twin"][1] <= lc.GATE_PCOST_HOST and res["twin"][2] <= lc.GATE_COST_HOST and res["twin"][3]
    m = res["mutant"]
    failed = {"eta0 added with the wrong sign": m[1] > 1e3 * lc.GATE_PCOST_HOST, "a butterfly stride dropped": m[2] > 1e3 * lc.GATE_COST_HOST,
              "<= in place of < in the accept test": not m[3], "lambda raised on accept": not m[3]}[what]
    assert failed, m


def test_a_strict_comparison_at_lam_max_fails_the_edge_table(hl, tmp_path):
    """< in place of <= at lam_max: the table of RULES keeps holding (no rule of it sits on the bound), the edge table does not."""
    mutant = _mutant(tmp_path, "if (!(l <= p.lam_max)) phase = 2;", "if (!(l < p.lam_max)) phase = 2;")
    plain, _ = lc.rule_table()
    edge, want = lc.edge_rule_table()
    check_accept(twin_accept(hl, edge), edge.expected())
    check_accept(twin_accept(mutant, plain), plain.expected())
    got = twin_accept(mutant, edge)
    print("the mutant on 'lambda * lam_up == lam_max': phase %d lambda %g (the rule: %s)" % (got[4][0], got[3][0], want[0]))
    assert (got[4][0], got[3][0]) == (lc.GAVE_UP, 1e4)
    with pytest.raises(AssertionError):
        check_accept(got, edge.expected())


def test_the_stand_alone_twin_program(tmp_path):
    exe = str(tmp_path / "hostsim_lm_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-ffp-contract=off", "-DHOSTSIM_LM_MAIN", "-o", exe, _SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout
