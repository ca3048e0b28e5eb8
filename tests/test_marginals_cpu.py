"""CPU: cpi_chain_marginals_batch without a GPU -- declarations, contract, and the arithmetic.

1. Declarations: the entries are exported, declared in include/cpi_amd.h with their exact argument lists, listed among the additions
   within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_marginals has a resource report of its own, no other report names its
   kernel, it uses no scratch; Engine, the module and the C++ facade have the entries.
2. The contract through ctypes: every refusal comes before the context is looked at, so a NULL context shows code and text; every
   forbidden overlap is tried.  The host form names the chain whose range is wrong.
3. The host twin (tests/hostsim/hostsim_marginals.cpp over chn::solve_chain and chn::marginals_chain of cpi_math.hpp, compiled with
   -ffp-contract=off) against the longdouble dense inverse of tests/marginals_cases.py on every layout; the metric is printed first.
   The twin's solve writes a W record for a chain's last state; it is overwritten with NaN before the marginals run, so a read of it
   would show.  Mutations of the twin built in tmp_path (the R^-1 R^-T term dropped, the sign of cross) must fail the gate.
4. The edges of the contract (the cases of tests/chain_cases.py, the checks of tests/chain_edge_checks.py) on the twins of the solve
   and of the marginals together, before tests/test_gpu_chain_edges.py asks the same of the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import chain_edge_checks as ck
from tests import marginals_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_marginals.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_marginals.so")
_MATH = os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")
SENTINEL = -7.0

DECLS = {"cpi_chain_marginals_batch": "cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, const int64_t *first, const int32_t *count, "
                                      "const int32_t *status, const double *workspace, double *cov, double *cross",
         "cpi_chain_marginals_batch_host": "cpi_ctx *ctx, int64_t C, int64_t G, int64_t S, int64_t F, const int64_t *first, "
                                           "const int32_t *count, const int64_t *ffirst, const double *hess, const double *prior, "
                                           "double *cov, double *cross, int32_t *status"}


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
    doc = flat.split("int cpi_chain_marginals_batch(")[0].rsplit("/*", 1)[1]
    for text in ("PARITY UNPINNED", "Marginals", "DAMPING INCLUDED", "lambda = NULL", "convergence check", "cpi_retract_batch",
                 "cpi_sqrt_information_packed_batch", "overlaps", "allocates nothing", "read only", "not written",
                 "without parallel branches", "no parallelism ALONG a chain"):
        assert text in doc, text
    assert flat.index("int cpi_chain_solve_batch(") < flat.index("int cpi_chain_marginals_batch(") < flat.index("/* ---- Device sets")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## 3n." in integ and "chain_marginals" in integ.split("\n## 3n.", 1)[1] and "lam=None" in integ.split("\n## 3n.", 1)[1]


def test_kernel_has_a_unit_and_a_report_of_its_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_marginals"][-4:] == ["cpi_marginals.hip", "cpi_factor_kernels.hpp", "cpi_chain_util.hpp", "cpi_marginals_kernels.hpp"]
    assert "cpi_chain_kernels.hpp" not in build.UNITS["cpi_marginals"]
    unit = open(os.path.join(build.CSRC, "cpi_marginals.hip")).read() + open(os.path.join(build.CSRC, "cpi_marginals_kernels.hpp")).read()
    assert '#include "cpi_chain_kernels.hpp"' not in unit
    own = build.UNIT_REPORTS["cpi_marginals"]
    assert os.path.basename(own) == "resource_usage_marginals.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == ["cpi_marginals_kernel"]
    regs, scratch, occ, lds = rows["cpi_marginals_kernel"]
    print("cpi_marginals_kernel: %d registers, scratch %d, occupancy %d, LDS %d" % (regs, scratch, occ, lds))
    assert scratch == 0 and regs <= 512 and occ >= 1
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_marginals_kernel" in open(path).read()) == (unit == "cpi_marginals"), path
    body = open(_MATH).read().split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    for helper in ("factor_block(", "solve_w(", "schur(", "solve_chain(", "marginals_chain("):
        assert re.search(r"CPI_HD \w[\w<> ]* %s" % re.escape(helper), body), helper
    assert "CPI_HD void marginals_chain(int n, const double *ws, double *cov, double *cross)" in body


def test_engine_module_and_facade_have_the_entries():
    import inspect
    import cpi_amd
    E = cpi_amd.Engine
    for fn, sym in ((E.chain_marginals, "cpi_chain_marginals_batch("), (E.chain_marginals_host, "cpi_chain_marginals_batch_host(")):
        assert sym in inspect.getsource(fn), sym
    assert list(inspect.signature(E.chain_marginals).parameters)[1:] == ["workspace", "C", "G", "first", "count", "status", "out", "cross"]
    assert list(inspect.signature(E.chain_marginals_host).parameters)[1:9] == ["hess", "C", "G", "first", "count", "ffirst", "prior", "cross"]
    assert inspect.signature(E.chain_marginals_host).parameters["cross"].default is False
    assert callable(cpi_amd.chain_marginals)
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_chain_marginals_batch_host(" in src and re.search(r"std::vector<double> chain_marginals\(const Context &ctx", src)
    assert "chain_marginals(ctx, C, G, hess, prior, &cross, &status)" in open(os.path.join(ROOT, "tests", "cpp", "test_marginals.cpp")).read()


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


def test_device_form_refusals_come_before_the_context(lib):
    f, entry = lib.cpi_chain_marginals_batch, "cpi_chain_marginals_batch"
    Cn, G = 4, 3
    S = Cn * G
    a = {"first": np.arange(Cn, dtype=np.int64) * G, "count": np.full(Cn, G, dtype=np.int32), "status": np.zeros(Cn, dtype=np.int32),
         "workspace": np.zeros(lib.cpi_chain_solve_workspace_doubles(S)), "cov": np.zeros(S * 120), "cross": np.zeros(S * 225)}
    ptr = lambda x, off=0: None if x is None else x.ctypes.data + off

    def call(C_=Cn, G_=G, S_=S, **kw):
        v = {k: ptr(x) for k, x in a.items()}
        v.update(kw)
        return f(None, C_, G_, S_, v["first"], v["count"], v["status"], v["workspace"], v["cov"], v["cross"]), _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")                                       # a valid call gets as far as the context
    assert call(first=None, count=None, status=None, cross=None) == (1, "ctx is NULL")
    assert call(S_=0, workspace=None, cov=None, cross=None) == (1, "ctx is NULL")   # no states: nothing to point at
    refused("negative size", C_=-1)
    refused("negative size", S_=-1)
    refused("G (the longest chain in states) must be >= 1", G_=0)
    refused("G (the longest chain in states) must be >= 1", G_=-3)
    refused("G exceeds 2^31 - 1", G_=2 ** 31)
    refused("workspace is NULL", workspace=None)
    refused("cov is NULL", cov=None)
    for o in ("cov", "cross"):                                                # every output against every input ...
        for i in ("workspace", "first", "count", "status"):
            # the output begins inside the input's last element (it is long enough to reach the arrays numpy put behind it as well:
            # whichever output the text names, it is an overlap)
            refused("overlaps", **{o: ptr(a[i], a[i].nbytes - 4)})
            refused("overlaps", **{i: ptr(a[o], 8)})                          # the input begins inside the output
    refused("cov overlaps", cross=ptr(a["cov"], 8 * (S * 120 - 1)))           # ... and against the other output
    refused("cov overlaps", cov=ptr(a["cross"], 8 * (S * 225 - 1)))
    buf = np.zeros(S * 345)
    assert call(cov=ptr(buf), cross=ptr(buf, 8 * S * 120)) == (1, "ctx is NULL")   # back to back: fine


def test_host_form_refusals_and_the_chain_whose_range_is_wrong(lib):
    f, entry = lib.cpi_chain_marginals_batch_host, "cpi_chain_marginals_batch_host"
    Cn, G = 4, 3
    S, F = Cn * G, Cn * (G - 1)
    a = {"first": np.arange(Cn, dtype=np.int64) * G, "count": np.full(Cn, G, dtype=np.int32), "ffirst": np.arange(Cn, dtype=np.int64) * (G - 1),
         "hess": np.zeros(F * 496), "prior": np.zeros(S * 136), "cov": np.zeros(S * 120), "cross": np.zeros(S * 225),
         "status": np.zeros(Cn, dtype=np.int32)}
    ptr = lambda x, off=0: None if x is None else x.ctypes.data + off

    def call(C_=Cn, G_=G, S_=S, F_=F, **kw):
        v = {k: ptr(x) for k, x in a.items()}
        v.update(kw)
        return f(None, C_, G_, S_, F_, v["first"], v["count"], v["ffirst"], v["hess"], v["prior"], v["cov"], v["cross"], v["status"]), _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")
    assert call(first=None, count=None, ffirst=None, prior=None, cross=None, status=None) == (1, "ctx is NULL")
    assert call(G_=1, F_=0, hess=None, S_=Cn, first=None, ffirst=None) == (1, "ctx is NULL")   # chains of one state need no hess
    for k in ("C_", "S_", "F_"):
        refused("negative size", **{k: -1})
    refused("G (the longest chain in states) must be >= 1", G_=0)
    refused("G exceeds 2^31 - 1", G_=2 ** 31)
    refused("cov is NULL", cov=None)
    refused("hess is NULL", hess=None)
    refused("negative size", F_=-1, G_=0)                                     # which refusal wins when two apply: sizes, then pointers,
    refused("cov is NULL", cov=None, hess=None)                               # then overlaps, then the ranges
    refused("hess is NULL", hess=None, ffirst=ptr(a["cov"], 4))
    refused("cov overlaps", cov=ptr(a["hess"], 8), F_=F - 1)
    for o in ("cov", "cross", "status"):
        for i in ("first", "count", "ffirst", "hess", "prior"):
            refused("overlaps", **{o: ptr(a[i], a[i].nbytes - 4)})
            refused("overlaps", **{i: ptr(a[o], 4)})
    refused("cov overlaps", cross=ptr(a["cov"], 8 * (S * 120 - 1)))
    refused("overlaps", status=ptr(a["cross"], 8))
    # ranges, as cpi_chain_solve_batch_host validates them: the text names the chain
    bad = a["ffirst"].copy()
    bad[2] = F - 1                                                            # two factor rows from F - 1 on: one past the end
    refused("the factor rows of chain 2 leave [0, F)", ffirst=ptr(bad))
    bad[2] = -1
    refused("the factor rows of chain 2 leave [0, F)", ffirst=ptr(bad))
    refused("the factor rows of chain 3 leave [0, F)", F_=F - 1)
    bad = a["first"].copy()
    bad[1] = S - 2                                                            # three states from S - 2 on
    refused("the states of chain 1 leave [0, S)", first=ptr(bad))
    bad[1] = -3
    refused("the states of chain 1 leave [0, S)", first=ptr(bad))
    refused("the states of chain 3 leave [0, S)", S_=S - 1)


# ---------------------------------------------------------------- host twin
def _build(src, out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", out, src])


def _bind(path):
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.hsm_chain_solve.argtypes = [C.c_longlong] * 4 + [vp] * 6 + [C.c_int, vp, vp, vp, C.c_int]
    lib.hsm_chain_marginals.argtypes = [C.c_longlong] * 3 + [vp] * 6
    return lib


@pytest.fixture(scope="module")
def hs():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in (_SRC, _MATH)):
        _build(_SRC, _LIB)
    return _bind(_LIB)


def twin(hs, b, lam=None, with_prior=True, status_in=None, chains=None):
    """solve_chain (lam, identity damping) then marginals_chain of batch b -> (cov [S, 120], cross [S, 225], status [C]) with the
    sentinel in what nobody wrote.  The W record of every chain's last state is NaN when the marginals run."""
    p = lambda x: None if x is None else x.ctypes.data
    idx = np.arange(b.C) if chains is None else np.asarray(chains)
    first, count, ffirst = (np.ascontiguousarray(v[idx]) for v in (b.first, b.count, b.ffirst))
    lam = None if lam is None else np.ascontiguousarray(np.asarray(lam, dtype=np.float64)[idx])
    delta = np.zeros((b.S, 15))
    status = np.full(len(idx), 99, dtype=np.int32)
    ws = np.full(max(b.S, 1) * hs.hsm_ws_doubles(), np.nan)
    assert hs.hsm_chain_solve(len(idx), b.G, b.S, b.F, p(first), p(count), p(ffirst), p(b.hess), p(b.prior if with_prior else None), p(lam), 0,
                              p(delta), p(status), p(ws), 1) == 0
    cov, cross = np.full((b.S, 120), SENTINEL), np.full((b.S, 225), SENTINEL)
    st = status if status_in is None else np.ascontiguousarray(status_in, dtype=np.int32)
    assert hs.hsm_chain_marginals(len(idx), b.G, b.S, p(first), p(count), p(st), p(ws), p(cov), p(cross)) == 0
    return cov, cross, status


def sweep(hs, lam_v=None):
    """The largest metric of the twin over every layout and both priors (printed per case)."""
    worst = cmax = 0.0
    emin = np.inf
    for name in cc.LAYOUTS:
        for prior_all in (False, True):
            b, lam, ref = mc.case(name, prior_all, lam_v)
            cov, cross, status = twin(hs, b, lam)
            m = ref.metric(cov, cross)
            print("| %s | %s | %s | %.1e | %.3e |" % (name, "all" if prior_all else "first", lam_v, ref.cond.max(), m))
            assert (status == 0).all(), (name, status)
            worst, cmax, emin = max(worst, m), max(cmax, ref.cond.max()), min(emin, ref.min_correlation_eigenvalue())
    return worst, cmax, emin


def test_twin_meets_the_gate_on_every_layout(hs):
    print("| layout | prior | lambda | cond max | metric |")
    worst, cmax, emin = sweep(hs)
    print("largest metric %.3e (floor %.3e, gate %.2e); largest cond %.2e; smallest correlation eigenvalue %.2e" % (worst, mc.FLOOR_HOST, mc.GATE_HOST, cmax, emin))
    assert cmax <= cc.COND_MAX and emin > 1e-4
    assert worst <= mc.GATE_HOST


def test_twin_with_identity_damping_inverts_the_damped_matrix(hs):
    worst, _, _ = sweep(hs, 3.0)
    print("identity damping 3.0: largest metric %.3e (gate %.2e)" % (worst, mc.GATE_HOST))
    assert worst <= mc.GATE_HOST


def test_one_state_is_the_inverse_of_the_prior_block(hs):
    b, _, ref = mc.case("one_1", False)
    cov, cross, status = twin(hs, b)
    lam0 = 0.1 * cc.SCALES ** 2
    got = mc.unpack_cov(cov[0])
    # 1 / sqrt (two roundings), squared (one more, the error doubled), times lam0 (one more): below 8 x 2^-53
    print("count = 1: largest |cov lam0 - I| %.3e" % np.abs(got * lam0[None, :] - np.eye(15)).max())
    assert status.tolist() == [0] and np.abs(got * lam0[None, :] - np.eye(15)).max() <= 8 * cc.EPS_HALF
    assert (cross == SENTINEL).all()
    lam = np.array([3.0])
    cov, _, _ = twin(hs, b, lam)                                              # ... and of (Lam + damping)
    assert np.abs(mc.unpack_cov(cov[0]) * (lam0 + 3.0)[None, :] - np.eye(15)).max() <= 8 * cc.EPS_HALF


def test_blocks_are_positive_definite_and_unwritten_rows_keep_the_sentinel(hs):
    for name in cc.LAYOUTS:
        b, lam, ref = mc.case(name, False)
        cov, cross, _ = twin(hs, b)
        none = mc.untouched_rows(b)
        assert (cov[none] == SENTINEL).all() and (cross[none] == SENTINEL).all(), name          # rows of no chain
        assert (cross[mc.last_rows(b)] == SENTINEL).all(), name                                  # the cross row of a last state
        written = ~none
        assert np.isfinite(cov[written]).all()
        M = mc.unpack_cov(cov[written])
        assert np.array_equal(M, M.swapaxes(-1, -2))                                              # one triangle, mirrored
        assert np.isfinite(np.linalg.cholesky(M)).all(), name
        last = np.zeros(b.S, dtype=bool)
        last[mc.last_rows(b)] = True
        assert np.isfinite(cross[written & ~last]).all()


def test_a_failed_chain_is_nan_and_its_neighbours_keep_their_bits(hs):
    b = cc.Batch(cc.RAGGED, seed=mc.SEED, layout="gaps")
    good, goodx, status = twin(hs, b)
    assert (status == 0).all()
    b.prior[b.first[4] + 3, 2 + 2 * 3 // 2] = -1e9                           # entry (2, 2) of the block of state 3 of chain 4: indefinite
    bad, badx, status = twin(hs, b)
    assert status[4] == 4 and [int(s) for k, s in enumerate(status) if k != 4] == [0] * 10, status
    rows = b.rows(4)
    assert np.isnan(bad[rows]).all() and np.isnan(badx[rows][:-1]).all() and (badx[rows][-1] == SENTINEL).all()
    for c in range(b.C):
        if c != 4:
            assert np.array_equal(bad[b.rows(c)], good[b.rows(c)]) and np.array_equal(badx[b.rows(c)], goodx[b.rows(c)]), c
    assert (bad[mc.untouched_rows(b)] == SENTINEL).all()
    one, onex, _ = twin(hs, b, chains=[7])                                    # a chain alone and at another position: its own bits
    assert np.array_equal(one[b.rows(7)], good[b.rows(7)]) and np.array_equal(onex[b.rows(7)], goodx[b.rows(7)])
    assert (one[mc.untouched_rows(b, [7])] == SENTINEL).all()


@pytest.mark.parametrize("what", ["the R^-1 R^-T term", "the sign of cross"])
def test_a_wrong_term_fails_the_gate(hs, tmp_path, what):
    """The twin with one term wrong, built in tmp_path: the metric leaves the gate by orders of magnitude."""
    old, new = {"the R^-1 R^-T term": ("Sg[i][j] = g;", "Sg[i][j] = 0.0 * g;"),
                "the sign of cross": ("i + 15 * c] = -T[c][i];", "i + 15 * c] = T[c][i];")}[what]
    text = open(_MATH).read()
    assert text.count(old) == 1, old
    os.makedirs(tmp_path / "cpi_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "hostsim")
    (tmp_path / "cpi_amd" / "csrc" / "cpi_math.hpp").write_text(text.replace(old, new))
    shutil.copy(_SRC, tmp_path / "tests" / "hostsim" / "hostsim_marginals.cpp")
    out = str(tmp_path / "libmutant.so")
    _build(str(tmp_path / "tests" / "hostsim" / "hostsim_marginals.cpp"), out)
    mutant = _bind(out)
    b, lam, ref = mc.case("ragged", False)
    m_good = ref.metric(*twin(hs, b)[:2])
    m_bad = ref.metric(*twin(mutant, b)[:2])
    print("%s wrong: metric %.3e (the twin as it is: %.3e, gate %.2e)" % (what, m_bad, m_good, mc.GATE_HOST))
    assert m_good <= mc.GATE_HOST < 1e3 * mc.GATE_HOST < m_bad


# ---------------------------------------------------------------- the edges of the contract, on the twin first
def twin_run(hs):
    """run(call, status_in) of tests/chain_edge_checks.py on the twins of the solve and of the marginals, the W record of every last
    state poisoned in between.  cov and cross are pre-filled with the sentinel: a poisoned row and an unwritten one differ."""
    def run(call, status_in=None):
        b = call.b
        p = lambda x: None if x is None else x.ctypes.data
        delta = np.full((b.S, 15), ck.SENTINEL)
        status = np.full(call.C, 99, dtype=np.int32)
        ws = np.full(max(call.S, 1) * hs.hsm_ws_doubles(), np.nan)
        hess = np.concatenate([b.hess, np.full((1, 496), np.nan)])
        assert hs.hsm_chain_solve(call.C, call.G, call.S, b.F, p(call.first), p(call.count), p(call.ffirst), p(hess),
                                  p(b.prior if call.with_prior else None), p(call.lam), int(call.diagonal), p(delta), p(status), p(ws), 1) == 0
        cov, cross = np.full((b.S, 120), ck.SENTINEL), np.full((b.S, 225), ck.SENTINEL)
        st = status if status_in is None else np.ascontiguousarray(status_in, dtype=np.int32)
        assert hs.hsm_chain_marginals(call.C, call.G, call.S, p(call.first), p(call.count), p(st), p(ws), p(cov), p(cross)) == 0
        return ck.Result(delta, status, cov, cross, fill=ck.SENTINEL)
    return run


def test_twin_failed_chains_of_the_failure_plan_are_nan(hs):
    ck.check_failure_plan(twin_run(hs))


def test_twin_nan_in_g_leaves_the_covariances(hs):
    ck.check_nan_plan(twin_run(hs))


def test_twin_refused_chains_are_nan(hs):
    ck.check_ffirst_boundaries(twin_run(hs))


def test_twin_ffirst_null_with_an_explicit_first(hs):
    ck.check_ffirst_null(twin_run(hs))


def test_twin_clamps_of_first_count_G_and_S(hs):
    ck.check_clamps(twin_run(hs))


def test_twin_a_wavefront_of_empty_chains(hs):
    ck.check_empty_wave(twin_run(hs), cc.GATE_BACKWARD_HOST, cc.GATE_FORWARD_HOST)


def test_twin_a_zero_block_is_a_failed_pivot(hs):
    identity, _ = ck.check_zero_pivot(twin_run(hs))
    row = cc.zero_pivot_case(False)[0].rows(1).start
    # (0 + 2 I)^-1: 1 / sqrt (two roundings), squared (one more, the error doubled): below 8 x 2^-53
    assert np.abs(mc.unpack_cov(identity.cov[row]) - 0.5 * np.eye(15)).max() <= 8 * cc.EPS_HALF


def test_twin_a_status_of_the_callers_poisons_exactly_its_chain(hs):
    ck.check_status_overlay(twin_run(hs))


def test_twin_long_chain_beside_short_ones(hs):
    b, ref = mc.long_case()
    r = twin_run(hs)(cc.Call(b, count=b.count))
    m = ref.metric(r.cov, r.cross)
    print("LONG %s: cond max %.1e, smallest correlation eigenvalue %.2e, twin metric %.3e (gate %.2e)"
          % (cc.LONG, ref.cond.max(), ref.min_correlation_eigenvalue(), m, mc.GATE_HOST))
    assert r.status.tolist() == [0] * 4 and m <= mc.GATE_HOST
    own, _ = cc.Call(b, count=b.count).owned()
    assert np.isfinite(np.linalg.cholesky(mc.unpack_cov(r.cov[own]))).all()
    ck.unowned(r, cc.Call(b, count=b.count))


@pytest.mark.parametrize("e", [300, -300])
def test_twin_scaled_by_a_power_of_two(hs, e):
    _, ref = mc.scaled_reference()
    b = cc.scaled_batch(e)
    r = twin_run(hs)(cc.Call(b, count=b.count))
    m = ref.metric(r.cov * 2.0 ** e, r.cross * 2.0 ** e)
    print("hess, prior x 2^%d: cond max %.1e, twin metric %.3e (gate %.2e)" % (e, ref.cond.max(), m, mc.GATE_HOST))
    assert (r.status == 0).all() and m <= mc.GATE_HOST


def test_twin_with_diagonal_damping_inverts_the_damped_matrix(hs):
    b, lam, ref = mc.diagonal_case()
    r = twin_run(hs)(cc.Call(b, count=b.count, lam=lam, diagonal=True))
    m = ref.metric(r.cov, r.cross)
    print("diagonal damping 0.25: cond max %.1e, twin metric %.3e (gate %.2e)" % (ref.cond.max(), m, mc.GATE_HOST))
    assert (r.status == 0).all() and m <= mc.GATE_HOST
