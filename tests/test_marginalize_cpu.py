"""CPU: cpi_chain_marginalize_batch without a GPU -- declarations, contract, and the arithmetic.

1. Declarations: the entries are exported, declared in include/cpi_amd.h with their exact argument lists after
   cpi_chain_marginals_batch, listed among the additions within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_marginalize has a
   resource report of its own, no other report names its kernel, it uses no scratch; Engine, the module and the C++ facade have
   the entries.
2. The contract through ctypes: every refusal comes before the context is looked at, so a NULL context shows code and text; every
   forbidden overlap is tried.  The host form names the chain whose range or whose drop is wrong.
3. The host twin (tests/hostsim/hostsim_marginalize.cpp over chn::marginalize_chain of cpi_math.hpp, compiled with
   -ffp-contract=off) against the longdouble Schur complement of tests/marginalize_cases.py on every layout, both priors and every
   drop plan; the metrics are printed first.  Equivalence: the twin of the solve on the reduced chains gives the full chains' delta.
   What the twin must not read is NaN; m = 0 passes the prior through; a failed eliminated block is NaN and alone; mutations of the
   twin built in tmp_path must fail the gates.
4. The edges of the contract (tests/marginalize_edge_checks.py, which tests/test_gpu_marginalize_edges.py runs on the device): frozen
   chains beside failing ones, NaN at status 0, the status across marginalize and the reduced solve, a zero block, ffirst, the clamps,
   status == NULL, call sizes, powers of two.  Four rules of the contract, each broken in a copy of the twin, fail their check."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import marginalize_cases as mz
from tests import marginalize_edge_checks as mk
from tests import test_marginals_cpu as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_marginalize.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_marginalize.so")
_MATH = os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")
SENTINEL = -7.0

_COMMON = ("cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, const int32_t *count, const int64_t *ffirst, "
           "const double *hess, const double *prior, int32_t M, const int32_t *drop, double *out, int32_t *status")
DECLS = {"cpi_chain_marginalize_batch": _COMMON, "cpi_chain_marginalize_batch_host": _COMMON}


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
    doc = flat.split("int cpi_chain_marginalize_batch(")[0].rsplit("/*", 1)[1]
    for text in ("PARITY UNPINNED", "Schur complement", "UNDAMPED", "do NOT enter", "Entry 135 is written as 0.0", "symmetric by construction",
                 "outside [0, n_c)", "NaN row", "WHAT IT GUARANTEES", "LINEAR prior", "overlapping", "allocates nothing", "no workspace",
                 "without parallel branches", "no parallelism ALONG a chain"):
        assert text in doc, text
    assert flat.index("int cpi_chain_marginals_batch(") < flat.index("int cpi_chain_marginalize_batch(") < flat.index("/* ---- Device sets")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## 3o." in integ
    sec = integ.split("\n## 3o.", 1)[1]
    for text in ("chain_marginalize", "local_coordinates", "x_lin", "eta0"):
        assert text in sec, text


def test_kernel_has_a_unit_and_a_report_of_its_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_marginalize"][-4:] == ["cpi_marginalize.hip", "cpi_factor_kernels.hpp", "cpi_chain_util.hpp", "cpi_marginalize_kernels.hpp"]
    assert "cpi_chain_kernels.hpp" not in build.UNITS["cpi_marginalize"]
    unit = open(os.path.join(build.CSRC, "cpi_marginalize.hip")).read() + open(os.path.join(build.CSRC, "cpi_marginalize_kernels.hpp")).read()
    assert '#include "cpi_chain_kernels.hpp"' not in unit and '#include "cpi_chain_util.hpp"' in unit
    own = build.UNIT_REPORTS["cpi_marginalize"]
    assert os.path.basename(own) == "resource_usage_marginalize.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == ["cpi_marginalize_kernel"]
    regs, scratch, occ, lds = rows["cpi_marginalize_kernel"]
    print("cpi_marginalize_kernel: %d registers, scratch %d, occupancy %d, LDS %d" % (regs, scratch, occ, lds))
    assert scratch == 0 and regs <= 512 and occ >= 1
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_marginalize_kernel" in open(path).read()) == (unit == "cpi_marginalize"), path
    body = open(_MATH).read().split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    assert "CPI_HD int marginalize_chain(int n, int m, const double *hess, const double *prior, double *out)" in body
    mine = body.split("CPI_HD int marginalize_chain(", 1)[1]
    for helper in ("factor_block(A)", "solve_w(A, U)", "schur(U, A, N)"):
        assert helper in mine, helper


def test_engine_module_and_facade_have_the_entries():
    import cpi_amd
    E = cpi_amd.Engine
    for fn, sym in ((E.chain_marginalize, "cpi_chain_marginalize_batch("), (E.chain_marginalize_host, "cpi_chain_marginalize_batch_host(")):
        assert sym in inspect.getsource(fn), sym
        assert list(inspect.signature(fn).parameters)[1:] == ["hess", "C", "G", "first", "count", "ffirst", "prior", "drop", "out", "status"]
        assert inspect.signature(fn).parameters["drop"].default == 1
    assert callable(cpi_amd.chain_marginalize)
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_chain_marginalize_batch_host(" in src and re.search(r"std::vector<double> chain_marginalize\(const Context &ctx", src)
    assert "chain_marginalize(ctx, C, G, hess, prior, drop, &status)" in open(os.path.join(ROOT, "tests", "cpp", "test_marginalize.cpp")).read()


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


def _arrays(Cn=4, G=3):
    S, F = Cn * G, Cn * (G - 1)
    return {"first": np.arange(Cn, dtype=np.int64) * G, "count": np.full(Cn, G, dtype=np.int32), "ffirst": np.arange(Cn, dtype=np.int64) * (G - 1),
            "hess": np.zeros(F * 496), "prior": np.zeros(S * 136), "drop": np.ones(Cn, dtype=np.int32), "out": np.zeros(Cn * 136),
            "status": np.zeros(Cn, dtype=np.int32)}, S, F


@pytest.mark.parametrize("entry", list(DECLS))
def test_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    Cn, G = 4, 3
    a, S, F = _arrays(Cn, G)
    ptr = lambda x, off=0: None if x is None else x.ctypes.data + off

    def call(C_=Cn, G_=G, S_=S, F_=F, M_=1, **kw):
        v = {k: ptr(x) for k, x in a.items()}
        v.update(kw)
        return f(None, C_, G_, S_, F_, v["first"], v["count"], v["ffirst"], v["hess"], v["prior"], M_, v["drop"], v["out"], v["status"]), _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")                                       # a valid call gets as far as the context
    assert call(first=None, count=None, ffirst=None, prior=None, drop=None, status=None) == (1, "ctx is NULL")
    assert call(G_=1, F_=0, hess=None, S_=Cn, first=None, ffirst=None, M_=0, drop=None) == (1, "ctx is NULL")   # chains of one state need no hess
    for k in ("C_", "S_", "F_"):
        refused("negative size", **{k: -1})
    refused("G (the longest chain in states) must be >= 1", G_=0)
    refused("G (the longest chain in states) must be >= 1", G_=-3)
    refused("G exceeds 2^31 - 1", G_=2 ** 31)
    refused("hess is NULL", hess=None)
    refused("out is NULL", out=None)
    refused("negative size", F_=-1, G_=0)                                     # which refusal wins when two apply: sizes, then pointers,
    refused("hess is NULL", hess=None, out=None)                              # then overlaps
    for o in ("out", "status"):                                               # every output against every input ...
        for i in ("first", "count", "ffirst", "hess", "prior", "drop"):
            refused("overlaps", **{o: ptr(a[i], a[i].nbytes - 4)})            # the output begins inside the input's last element
            refused("overlaps", **{i: ptr(a[o], 4)})                          # the input begins inside the output
    refused("out overlaps", status=ptr(a["out"], 8))                          # ... and against the other output
    refused("overlaps", out=ptr(a["status"], 0))


def test_host_form_names_the_chain_whose_range_or_drop_is_wrong(lib):
    f, entry = lib.cpi_chain_marginalize_batch_host, "cpi_chain_marginalize_batch_host"
    Cn, G = 4, 3
    a, S, F = _arrays(Cn, G)
    ptr = lambda x: None if x is None else x.ctypes.data

    def refused(text, C_=Cn, G_=G, S_=S, F_=F, M_=1, **kw):
        v = {k: ptr(x) for k, x in a.items()}
        v.update({k: ptr(x) for k, x in kw.items()})
        rc = f(None, C_, G_, S_, F_, v["first"], v["count"], v["ffirst"], v["hess"], v["prior"], M_, v["drop"], v["out"], v["status"])
        msg = _err(lib)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    bad = a["ffirst"].copy()
    bad[2] = F - 1                                                            # two factor rows from F - 1 on: one past the end
    refused("the factor rows of chain 2 leave [0, F)", ffirst=bad)
    bad[2] = -1
    refused("the factor rows of chain 2 leave [0, F)", ffirst=bad)
    refused("the factor rows of chain 3 leave [0, F)", F_=F - 1)
    bad = a["first"].copy()
    bad[1] = S - 2                                                            # three states from S - 2 on
    refused("the states of chain 1 leave [0, S)", first=bad)
    refused("the states of chain 3 leave [0, S)", S_=S - 1)
    bad = a["drop"].copy()
    bad[2] = G                                                                # m = n
    refused("drop of chain 2 leaves [0, count)", drop=bad)
    bad[2] = -1
    refused("drop of chain 2 leaves [0, count)", drop=bad)
    refused("drop of chain 0 leaves [0, count)", drop=None, M_=G)             # the scalar: every chain, the first one is named
    cnt = a["count"].copy()
    cnt[3] = 1                                                                # one state and m = 1
    refused("drop of chain 3 leaves [0, count)", count=cnt)
    refused("the states of chain 1 leave [0, S)", first=np.array([0, S - 2, 6, 9], dtype=np.int64), drop=bad)   # ranges before drop


# ---------------------------------------------------------------- host twin
def _bind(path):
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.hsz_chain_marginalize.argtypes = [C.c_longlong] * 4 + [vp] * 5 + [C.c_int] + [vp] * 3
    return lib


@pytest.fixture(scope="module")
def hz():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in (_SRC, _MATH)):
        tm._build(_SRC, _LIB)
    return _bind(_LIB)


@pytest.fixture(scope="module")
def hs():
    if (not os.path.exists(tm._LIB)) or os.path.getmtime(tm._LIB) < max(os.path.getmtime(p) for p in (tm._SRC, _MATH)):
        tm._build(tm._SRC, tm._LIB)
    return tm._bind(tm._LIB)


def twin(hz, b, drop, with_prior=True, hess=None, prior=None, first=None, count=None, ffirst=None):
    """marginalize_chain of batch b under drop (an int: M with drop = NULL) -> (out [C, 136], status [C]); a row of sentinels follows out."""
    p = lambda x: None if x is None else x.ctypes.data
    hess = b.hess if hess is None else hess
    prior = (b.prior if prior is None else prior) if with_prior else None
    first, count, ffirst = (np.ascontiguousarray(x if y is None else y) for x, y in ((b.first, first), (b.count, count), (b.ffirst, ffirst)))
    Cn = len(first)
    out = np.full((Cn + 1, 136), SENTINEL)
    status = np.full(Cn, 99, dtype=np.int32)
    M, d = (int(drop), None) if np.isscalar(drop) else (0, np.ascontiguousarray(drop, dtype=np.int32))
    assert hz.hsz_chain_marginalize(Cn, b.G, b.S, b.F, p(first), p(count), p(ffirst), p(hess), p(prior), M, p(d), p(out), p(status)) == 0
    assert (out[Cn] == SENTINEL).all()
    return out[:Cn], status


def twin_solve(hs, b, first, count, ffirst, prior):
    """solve_chain (lambda = NULL) of the chains first / count / ffirst on b.hess and prior -> (delta [S, 15], status)."""
    p = lambda x: None if x is None else x.ctypes.data
    first, count, ffirst = np.ascontiguousarray(first, dtype=np.int64), np.ascontiguousarray(count, dtype=np.int32), np.ascontiguousarray(ffirst, dtype=np.int64)
    delta = np.full((b.S, 15), SENTINEL)
    status = np.full(len(first), 99, dtype=np.int32)
    ws = np.full(max(b.S, 1) * hs.hsm_ws_doubles(), np.nan)
    assert hs.hsm_chain_solve(len(first), b.G, b.S, b.F, p(first), p(count), p(ffirst), p(b.hess), p(prior), None, 0, p(delta), p(status), p(ws), 0) == 0
    return delta, status


def sweep(hz, hs=None):
    """The largest (c), (d) -- and (a), (b) of the equivalence when hs is given -- of the twin over every layout, prior and plan."""
    worst = np.zeros(4)
    cmax = 0.0
    for name, prior_all in mz.cases():
        for plan in mz.PLANS:
            b, drop, ref, full = mz.reference(name, prior_all, plan)
            out, status = twin(hz, b, 1 if plan == "scalar1" else drop)
            m_c, m_d = ref.metrics(out)
            e_a = e_b = 0.0
            if hs is not None:
                delta, st2 = twin_solve(hs, b, *mz.reduced(b, drop, out, status))
                assert (st2 == 0).all(), (name, plan, st2)
                e_a, e_b = mz.equivalence(full, drop, status, delta)
            print("| %s | %s | %s | %.1e | %.3e | %.3e | %.3e | %.3e |" % (name, "all" if prior_all else "first", plan, ref.cond.max(), m_c, m_d, e_a, e_b))
            assert np.array_equal(status, ref.status), (name, plan, status)
            assert np.isnan(out[status != 0]).all() and np.isfinite(out[status == 0]).all()
            assert (out[status == 0, 135] == 0.0).all()
            worst = np.maximum(worst, [m_c, m_d, e_a, e_b])
            cmax = max(cmax, ref.cond.max())
    return worst, cmax


def test_twin_meets_the_gates_on_every_layout_and_plan(hz, hs):
    print("| layout | prior | plan | cond(A_EE) max | (c) | (d) | (e): (a) | (e): (b) |")
    worst, cmax = sweep(hz, hs)
    print("largest (c) %.3e (floor %.3e, gate %.2e); (d) %.3e (floor %.3e, gate %.2e); equivalence (a) %.3e, (b) %.3e (gate %.2e); largest cond %.2e"
          % (worst[0], mz.FLOOR_LAM_HOST, mz.GATE_LAM_HOST, worst[1], mz.FLOOR_ETA_HOST, mz.GATE_ETA_HOST, worst[2], worst[3],
             cc.GATE_FORWARD_HOST, cmax))
    assert cmax <= cc.COND_MAX
    assert worst[0] <= mz.GATE_LAM_HOST and worst[1] <= mz.GATE_ETA_HOST
    assert worst[3] <= cc.GATE_FORWARD_HOST                                   # (a) is printed for the record: marginalize_cases.py says why


def test_m_zero_passes_the_prior_through(hz):
    b, _ = mz.case("ragged", True)
    out, status = twin(hz, b, 0)
    has = b.count > 0
    assert status.tolist() == np.where(has, 0, -1).tolist()
    for c in np.nonzero(has)[0]:
        assert np.array_equal(out[c, :135], b.prior[b.first[c], :135]) and out[c, 135] == 0.0, c
    assert np.isnan(out[~has]).all()
    none, status = twin(hz, b, 0, with_prior=False)
    assert (none[has] == 0.0).all() and not np.signbit(none[has]).any() and np.isnan(none[~has]).all()


def test_only_what_is_eliminated_is_read(hz):
    for name in ("ragged", "reverse"):
        b, drop, ref, _ = mz.reference(name, True, "mixed2")
        good, status = twin(hz, b, drop)
        hess, prior = b.hess.copy(), b.prior.copy()
        for c in range(b.C):
            n, m = int(b.count[c]), int(drop[c])
            hess[b.ffirst[c] + m:b.ffirst[c] + max(n - 1, 0)] = np.nan
            prior[b.first[c] + m + 1:b.first[c] + n] = np.nan
        out, st = twin(hz, b, drop, hess=hess, prior=prior)
        assert np.array_equal(st, status) and np.array_equal(out, good, equal_nan=True), name


def test_the_triangle_is_mirrored_and_the_block_positive_definite(hz):
    b, drop, ref, _ = mz.reference("ragged", False, "mixed1")
    out, status = twin(hz, b, drop)
    for c in ref.lam:
        Lam, _ = mz.unpack_out(out[c])
        assert np.isfinite(np.linalg.cholesky(Lam)).all(), c


def test_a_failed_eliminated_block_is_nan_and_alone(hz):
    good, bad, st_solve = cc.failure_plan()
    clean, status = twin(hz, good.b, 3)
    assert (status == 0).all()
    ref = mz.Reference(good.b, np.full(good.b.C, 3))
    ref.check_inputs()
    for m in (1, 2, 3):
        out, status = twin(hz, bad.b, m)
        want = [s if 0 < s <= m else 0 for s in st_solve]                     # a bad block at a state >= m is not looked at
        assert status.tolist() == want, (m, status)
        assert np.isnan(out[status != 0]).all() and np.isfinite(out[status == 0]).all()
        if m == 3:
            ok = [c for c in range(good.b.C) if c not in cc.FAILURES]
            assert np.array_equal(out[ok], clean[ok])
            m_c, m_d = ref.metrics(out, ok)
            assert m_c <= mz.GATE_LAM_HOST and m_d <= mz.GATE_ETA_HOST


def test_composition_of_two_marginalisations(hz):
    """drop = a, then drop = b on the reduced chain with the first output as its prior, against drop = a + b at once: each is within
    its gate of the truth, so they differ by at most two gates."""
    b, full = mz.case("dense_9x17", True)                                     # a prior on every state: the two routes add it in different places
    a_, b_ = 5, 7
    ref = mz.Reference(b, np.full(b.C, a_ + b_))
    ref.check_inputs()
    once, st = twin(hz, b, a_ + b_)
    first_out, st1 = twin(hz, b, a_)
    f2, n2, ff2, prior2 = mz.reduced(b, np.full(b.C, a_), first_out, st1)
    twice, st2 = twin(hz, b, b_, prior=prior2, first=f2, count=n2, ffirst=ff2)
    assert (st == 0).all() and (st1 == 0).all() and (st2 == 0).all()
    worst_c = worst_d = 0.0
    for c in range(b.C):
        L1, e1 = mz.unpack_out(once[c])
        L2, e2 = mz.unpack_out(twice[c])
        d = np.sqrt(np.diagonal(ref.lam[c])).astype(np.float64)
        unit = ref.cond[c] * cc.EPS_HALF
        worst_c = max(worst_c, float((np.abs(L1 - L2) / (d[:, None] * d[None, :])).max() / unit))
        worst_d = max(worst_d, float((np.abs(e1 - e2) / (d * float(ref.q[c]))).max() / unit))
    print("5 then 7 against 12 at once: (c) %.3e (gate %.2e), (d) %.3e (gate %.2e)" % (worst_c, 2 * mz.GATE_LAM_HOST, worst_d, 2 * mz.GATE_ETA_HOST))
    assert worst_c <= 2 * mz.GATE_LAM_HOST and worst_d <= 2 * mz.GATE_ETA_HOST


@pytest.mark.parametrize("what", ["the Schur term", "the carried right-hand side"])
def test_a_wrong_term_fails_the_gate(hz, tmp_path, what):
    """The twin with one term of marginalize_chain wrong, built in tmp_path: a metric leaves its gate by orders of magnitude."""
    old, new = {"the Schur term": ("        schur(U, A, N);\n    }\n    const double *Pr = prior", "    }\n    const double *Pr = prior"),
                "the carried right-hand side": ("N[i][j] = sym_at(H, 15 + i, (j < 15) ? 15 + j : 30);\n        }\n        solve_w(A, U);\n        schur(U, A, N);\n    }\n    const",
                                                "N[i][j] = sym_at(H, 15 + i, (j < 15) ? 15 + j : 29);\n        }\n        solve_w(A, U);\n        schur(U, A, N);\n    }\n    const")}[what]
    text = open(_MATH).read()
    assert text.count(old) == 1, old
    os.makedirs(tmp_path / "cpi_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "hostsim")
    (tmp_path / "cpi_amd" / "csrc" / "cpi_math.hpp").write_text(text.replace(old, new))
    shutil.copy(_SRC, tmp_path / "tests" / "hostsim" / "hostsim_marginalize.cpp")
    out = str(tmp_path / "libmutant.so")
    tm._build(str(tmp_path / "tests" / "hostsim" / "hostsim_marginalize.cpp"), out)
    mutant = _bind(out)
    b, drop, ref, _ = mz.reference("ragged", False, "mixed2")
    g_c, g_d = ref.metrics(twin(hz, b, drop)[0])
    b_c, b_d = ref.metrics(twin(mutant, b, drop)[0])
    print("%s wrong: (c) %.3e (d) %.3e (the twin as it is: %.3e, %.3e)" % (what, b_c, b_d, g_c, g_d))
    assert g_c <= mz.GATE_LAM_HOST and g_d <= mz.GATE_ETA_HOST
    assert max(b_c / mz.GATE_LAM_HOST, b_d / mz.GATE_ETA_HOST) > 1e3


# ---------------------------------------------------------------- the edges of the contract, on the twin first
def twin_run(hz):
    """run(b, drop, **kw) of tests/marginalize_edge_checks.py on the twin.  hess and prior get one more row of NaN behind their F and S
    rows: a twin whose range rule is a row too lax (the mutants below) reads that instead of memory that is not the test's."""
    def run(b, drop, with_prior=True, hess=None, prior=None, G=None, S=None, status_in=None, no_status=False, **kw):
        p = lambda x: None if x is None else x.ctypes.data
        ptr = {"first": (b.first, np.int64), "count": (b.count, np.int32), "ffirst": (b.ffirst, np.int64)}
        arr = {k: None if kw.get(k, own) is None else np.ascontiguousarray(kw.get(k, own), dtype=dt) for k, (own, dt) in ptr.items()}
        assert set(kw) <= set(ptr), kw
        Cn = next((len(v) for v in arr.values() if v is not None), b.C)
        hess = np.concatenate([b.hess if hess is None else hess, np.full((1, 496), np.nan)])
        prior = np.concatenate([b.prior if prior is None else prior, np.full((1, 136), np.nan)]) if with_prior else None
        out = np.full((Cn + 1, 136), mk.SENTINEL)
        status = np.full(Cn + 1, 99, dtype=np.int32)
        if status_in is not None:
            status[:Cn] = status_in
        M, d = (int(drop), None) if np.isscalar(drop) else (0, np.ascontiguousarray(drop, dtype=np.int32))
        assert d is None or len(d) == Cn
        assert hz.hsz_chain_marginalize(Cn, b.G if G is None else G, b.S if S is None else S, b.F, p(arr["first"]), p(arr["count"]), p(arr["ffirst"]),
                                        p(hess), p(prior), M, p(d), p(out), None if no_status else p(status)) == 0
        assert (out[Cn] == mk.SENTINEL).all() and status[Cn] == 99
        if no_status:
            assert (status[:Cn] == (99 if status_in is None else status_in)).all()
        return out[:Cn], (None if no_status else status[:Cn])
    return run


def twin_solve_run(hs):
    def solve(b, first, count, ffirst, prior):
        return twin_solve(hs, b, first, count, ffirst, prior)
    return solve


def test_twin_frozen_chains_and_failures_with_an_m_per_chain(hz):
    mk.check_frozen_failures(twin_run(hz))


def test_twin_frozen_pivots_do_not_count(hz):
    mk.check_frozen_pivots_do_not_count(twin_run(hz))


def test_twin_long_chain_freezes_its_mates(hz):
    mk.check_long_freeze(twin_run(hz), mz.GATE_LAM_HOST, mz.GATE_ETA_HOST)


def test_twin_nan_in_the_inputs(hz):
    mk.check_nan_inputs(twin_run(hz))


def test_twin_status_law_across_marginalize_and_solve(hz, hs):
    mk.check_status_law(twin_run(hz), twin_solve_run(hs))


def test_twin_a_zero_block_is_a_failed_pivot(hz):
    mk.check_zero_block(twin_run(hz))


def test_twin_refusal_boundary_of_ffirst(hz):
    mk.check_ffirst_boundaries(twin_run(hz))


def test_twin_ffirst_null_with_an_explicit_first(hz):
    mk.check_ffirst_null(twin_run(hz))


def test_twin_clamps_of_first_count_G_and_S(hz):
    mk.check_clamps(twin_run(hz))


def test_twin_scalar_M_is_an_array_filled_with_M(hz):
    mk.check_scalar_against_array(twin_run(hz))


def test_twin_status_null(hz):
    mk.check_status_null(twin_run(hz))


def test_twin_call_sizes_around_a_wavefront(hz):
    mk.check_call_sizes(twin_run(hz))


def test_twin_scaled_by_a_power_of_two(hz):
    mk.check_scaling(twin_run(hz), mz.GATE_LAM_HOST, mz.GATE_ETA_HOST)


# the rules the edge tests are there for, each broken in a copy of the twin: (file, old, new, the check that must notice)
_TWIN = "tests/hostsim/hostsim_marginalize.cpp"
MUTANTS = {
    "the last failure wins": ("cpi_amd/csrc/cpi_math.hpp", "if (!pd && status == 0) status = s + 1;", "if (!pd) status = s + 1;", mk.check_frozen_failures),
    "a failed row is not filled with NaN": ("cpi_amd/csrc/cpi_math.hpp", "    if (status)\n        for (int i = 0; i < PRIOR_D; i++) out[i] = NAN;\n    return status;",
                                            "    return status;", mk.check_zero_block),
    "m = n is let through": (_TWIN, "|| m < 0 || m >= n) {", "|| m < 0 || m > n) {", mk.check_scalar_against_array),
    "ffirst is judged over the m rows that are read": (_TWIN, "if ((n > 1 && (ff < 0 || ff > F - (n - 1))) ||", "if ((m > 0 && (ff < 0 || ff > F - m)) ||",
                                                      mk.check_ffirst_boundaries),
}


@pytest.mark.parametrize("what", list(MUTANTS))
def test_a_broken_rule_fails_its_edge_test(hz, tmp_path, what):
    """Do the edge tests bite?  The twin with one rule of the contract broken, built in tmp_path, fails the check that states the rule
    (every access of these mutants stays inside the arrays: see twin_run and the tile layout of the chains that m = n is tried on),
    and the twin as it is passes it."""
    rel, old, new, check = MUTANTS[what]
    files = {_TWIN: open(_SRC).read(), "cpi_amd/csrc/cpi_math.hpp": open(_MATH).read()}
    assert files[rel].count(old) == 1, old
    files[rel] = files[rel].replace(old, new)
    for name, text in files.items():
        os.makedirs(tmp_path / os.path.dirname(name), exist_ok=True)
        (tmp_path / name).write_text(text)
    out = str(tmp_path / "libmutant.so")
    tm._build(str(tmp_path / _TWIN), out)
    check(twin_run(hz))
    with pytest.raises(AssertionError):
        check(twin_run(_bind(out)))
