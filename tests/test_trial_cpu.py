"""CPU: the optimiser's trial step without a GPU -- declarations, contract, and the arithmetic.

1. Declarations: the new entries are exported, declared in include/cpi_amd.h with their exact argument lists, listed among the
   additions within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_trial has a resource report of its own, no older report holds
   one of its kernels, none of them uses scratch; Engine and the C++ facade have the entries.
2. The contract through ctypes: every refusal comes before the context is looked at, so a NULL context shows code and text.
3. The host restatement (tests/hostsim/hostsim_trial.cpp over the CPI_HD functions of cpi_math.hpp the kernels call, compiled with
   -ffp-contract=off): retract / local against oracle/cpi_oracle.c on the inputs of tests/trial_cases.py (no case of the committed seed
   sits on one of the oracle's sign decisions); werr and chi2 of the cost against factor_cases.whitened_longdouble, chi2 bit for bit
   the documented summation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import factor_cases as fc
from tests import trial_cases as tc
from tests.tol import REG_FACTOR, sqrt_info_longdouble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_trial.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_trial.so")
_HDRS = [os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")]

COST_ARGS = ("cpi_ctx *ctx, int32_t model, const double grav[3], int64_t F, const cpi_outputs *meas, const double *lin, "
             "const double *q_k_lin, const double *states, int64_t S, const int32_t *idx_i, const int32_t *idx_j, ")
DECLS = {
    "cpi_retract_batch": "cpi_ctx *ctx, int64_t S, const double *states_in, const double *delta, double *states_out",
    "cpi_local_batch": "cpi_ctx *ctx, int64_t S, const double *x, const double *other, double *xi",
    "cpi_retract_batch_host": "cpi_ctx *ctx, int64_t S, const double *states_in, const double *delta, double *states_out",
    "cpi_local_batch_host": "cpi_ctx *ctx, int64_t S, const double *x, const double *other, double *xi",
    "cpi_factor_cost_batch": COST_ARGS + "const double *sqrt_info, double *chi2, double *werr, double *total",
    "cpi_factor_cost_tri_batch": COST_ARGS + "const double *R_tri, double *chi2, double *werr, double *total",
    "cpi_factor_cost_batch_host": COST_ARGS + "double *chi2, double *werr, double *total",
}
KERNELS = ("cpi_retract_kernel", "cpi_local_kernel", "cpi_factor_cost_kernel", "cpi_cost_partial_kernel", "cpi_cost_final_kernel")


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
    assert re.search(r" T cpi_factor_cost_total_doubles$", dyn, re.M)
    assert "size_t cpi_factor_cost_total_doubles(int64_t F);" in flat and lib.cpi_factor_cost_total_doubles.restype is C.c_size_t
    assert lib.cpi_abi_version() == 3
    within3 = flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1]
    for s in list(DECLS) + ["cpi_factor_cost_total_doubles"]:
        assert s in within3, s
    doc = flat.split("int cpi_retract_batch(")[0].rsplit("/* ----", 1)[1]
    for text in ("JPLNavState.cpp:37-71", "JPLNavState.cpp:80-88", "IN PLACE", "overlaps"):
        assert text in doc, text
    doc = flat.split("size_t cpi_factor_cost_total_doubles(")[0].rsplit("/*", 1)[1]
    for text in ("NoiseModelFactor::error", "PARITY UNPINNED", "cpi_factor_hessian_", "ascending", "chi2 = NaN", "allocates nothing"):
        assert text in doc, text


def test_kernels_have_a_unit_and_a_report_of_their_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_trial"][-3:] == ["cpi_trial.hip", "cpi_factor_kernels.hpp", "cpi_trial_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_trial"]
    assert os.path.basename(own) == "resource_usage_trial.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    want = ["cpi_retract_kernel", "cpi_local_kernel", "cpi_cost_partial_kernel", "cpi_cost_final_kernel"] + [
        "cpi_factor_cost_kernel<%d, %s, %d>" % (m, t, l) for m in (1, 2) for t in ("true", "false") for l in (16, 8, 4)]
    assert sorted(rows) == sorted(want)
    for name, (regs, scratch, occ, lds) in rows.items():
        assert scratch == 0 and regs <= 512, (name, regs, scratch)
        if name.startswith("cpi_factor_cost_kernel"):
            lpf = int(name.rsplit(",", 1)[1].strip(" >"))
            assert occ >= {16: 4, 8: 2, 4: 1}[lpf], (name, occ)        # what __launch_bounds__ asks for, the report shows
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        text = open(path).read()
        for k in KERNELS:
            assert (k in text) == (unit == "cpi_trial"), (path, k)
    math = open(os.path.join(build.CSRC, "cpi_math.hpp")).read()
    for helper in ("retract_dq(", "retract_state(", "local_coordinates(", "whiten_row(", "chi2_of("):
        assert re.search(r"CPI_HD \w[\w<> ]* %s" % re.escape(helper), math), helper


def test_engine_and_facade_have_the_entries():
    import inspect
    import cpi_amd
    E = cpi_amd.Engine
    for fn, sym in ((E.retract, "cpi_retract_batch"), (E.retract_host, "cpi_retract_batch_host"), (E.local_coordinates, "cpi_local_batch"),
                    (E.local_coordinates_host, "cpi_local_batch_host"), (E.factor_cost, "cpi_factor_cost_tri_batch"),
                    (E.factor_cost_host, "cpi_factor_cost_batch_host")):
        assert sym in inspect.getsource(fn), sym
    assert list(inspect.signature(E.retract).parameters)[1:] == ["states", "delta", "out"]
    assert list(inspect.signature(E.local_coordinates).parameters)[1:] == ["x", "other", "out"]
    assert list(inspect.signature(E.factor_cost).parameters)[1:] == ["model", "meas", "lin", "q_k_lin", "states", "sqrt_info", "idx_i", "idx_j",
                                                                      "grav", "want_err", "want_total", "out"]
    for name in ("retract", "local_coordinates", "factor_cost"):
        assert callable(getattr(cpi_amd, name))
    src = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_retract_batch_host(" in src and "cpi_local_batch_host(" in src and "cpi_factor_cost_batch_host(" in src
    assert re.search(r"std::vector<double> retract\(const Context &ctx", src) and re.search(r"double error\(const Context &ctx", src)


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


@pytest.mark.parametrize("entry", ["cpi_retract_batch", "cpi_retract_batch_host"])
def test_retract_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    buf = np.zeros(64 * 16)
    p = lambda off: buf.ctypes.data + 8 * off

    def refused(text, *a):
        rc = f(None, *a)
        assert rc == 1 and _err(lib).startswith(entry + ": ") and text in _err(lib), (a, rc, _err(lib))

    assert f(None, 4, p(0), p(200), p(400)) == 1 and _err(lib) == "ctx is NULL"      # a valid call gets as far as the context
    assert f(None, 4, p(0), p(200), p(0)) == 1 and _err(lib) == "ctx is NULL"        # in place
    refused("negative size", -1, p(0), p(200), p(400))
    refused("NULL argument", 4, None, p(200), p(400))
    refused("NULL argument", 4, p(0), None, p(400))
    refused("NULL argument", 4, p(0), p(200), None)
    refused("overlaps", 4, p(0), p(200), p(16))          # out = row 1 of in
    refused("overlaps", 4, p(0), p(200), p(63))          # out ends inside... begins inside in's last row
    refused("overlaps", 4, p(0), p(200), p(250))         # out begins inside delta
    refused("overlaps", 4, p(0), p(32), p(400))          # delta inside states_in
    assert f(None, 4, p(0), p(64), p(124)) == 1 and _err(lib) == "ctx is NULL"       # back to back: fine


@pytest.mark.parametrize("entry", ["cpi_local_batch", "cpi_local_batch_host"])
def test_local_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    buf = np.zeros(64 * 16)
    p = lambda off: buf.ctypes.data + 8 * off
    assert f(None, 4, p(0), p(64), p(128)) == 1 and _err(lib) == "ctx is NULL"
    assert f(None, 4, p(0), p(0), p(128)) == 1 and _err(lib) == "ctx is NULL"        # x == other is a question one may ask
    for text, a in (("negative size", (-1, p(0), p(64), p(128))), ("NULL argument", (4, None, p(64), p(128))),
                    ("NULL argument", (4, p(0), p(64), None)), ("overlaps", (4, p(0), p(64), p(60))), ("overlaps", (4, p(0), p(64), p(127)))):
        rc = f(None, *a)
        assert rc == 1 and _err(lib).startswith(entry + ": ") and text in _err(lib), (a, rc, _err(lib))


def _meas(F, model=2):
    from cpi_amd._lib import CpiOutputs
    o = CpiOutputs()
    names = ("DT", "alpha", "beta", "q", "J_q", "J_a", "J_b", "H_a", "H_b") + (("O_a", "O_b") if model == 2 else ())
    buf = np.zeros(16 * F * 16)
    for i, n in enumerate(names):
        setattr(o, n, buf.ctypes.data + 8 * F * 16 * i)    # never dereferenced: the call is refused, or stops at the NULL context
    o._keep = buf
    return o


@pytest.mark.parametrize("entry", ["cpi_factor_cost_batch", "cpi_factor_cost_tri_batch"])
def test_cost_refusals_come_before_the_context(lib, entry):
    f = getattr(lib, entry)
    F, S = 4, 8
    rd = 225 if entry == "cpi_factor_cost_batch" else 120
    g = (C.c_double * 3)(0, 0, 9.81)
    a = {k: np.zeros(n) for k, n in (("lin", F * 6), ("qk", F * 4), ("states", S * 16), ("R", F * rd), ("chi2", F), ("werr", F * 15), ("ws", 8))}
    idx = np.zeros(2 * F, dtype=np.int32)
    ptr = lambda x, off=0: None if x is None else x.ctypes.data + off

    def call(model=2, F=F, meas=None, S=S, **kw):
        v = dict(lin=ptr(a["lin"]), qk=ptr(a["qk"]), states=ptr(a["states"]), ii=ptr(idx), jj=ptr(idx, 4 * F), R=ptr(a["R"]),
                 chi2=ptr(a["chi2"]), werr=ptr(a["werr"]), total=ptr(a["ws"]))
        v.update(kw)
        m = _meas(max(F, 1), 2) if meas is None else meas
        rc = f(None, model, g, F, C.byref(m), v["lin"], v["qk"], v["states"], S, v["ii"], v["jj"], v["R"], v["chi2"], v["werr"], v["total"])
        return rc, _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")
    assert call(werr=None, total=None) == (1, "ctx is NULL")
    assert call(model=1, qk=None, meas=_meas(F, 1)) == (1, "ctx is NULL")
    refused("model must be 1 or 2", model=0)
    refused("model must be 1 or 2", model=3)               # the Forster comparator has no factor of its own
    refused("negative size", F=-1)
    refused("chi2 is NULL", chi2=None)
    refused("is NULL", R=None)
    refused("NULL argument", states=None)
    refused("model 2 needs q_k_lin", qk=None)
    refused("S (number of states)", S=0)
    refused("S (number of states)", ii=None, jj=None, S=F)
    refused("overlaps", chi2=ptr(a["states"], 8 * 16))     # an output inside the states
    refused("overlaps", werr=ptr(a["R"], 8 * (F * rd - 1)))
    refused("overlaps", total=ptr(a["lin"]))
    refused("overlaps", werr=ptr(a["chi2"], 8 * (F - 1)))  # two outputs
    refused("overlaps", total=ptr(a["chi2"]))
    refused("overlaps", chi2=ptr(idx, 4))
    m = _meas(F, 2)
    refused("overlaps", meas=m, chi2=m.J_a)


def test_host_cost_refusals(lib):
    f, entry = lib.cpi_factor_cost_batch_host, "cpi_factor_cost_batch_host"
    F, S = 4, 8
    g = (C.c_double * 3)(0, 0, 9.81)
    lin, qk, st, chi2 = np.zeros(F * 6), np.zeros(F * 4), np.zeros(S * 16), np.zeros(F)
    ii, jj = np.arange(F, dtype=np.int32), np.arange(F, dtype=np.int32) + 1
    m = _meas(F, 2)
    P = np.zeros(F * 225)
    d = lambda x: x.ctypes.data

    def call(model=2, meas=m, chi2_=d(chi2), ii_=ii, S_=S, F_=F, st_=d(st), jj_=jj):
        rc = f(None, model, g, F_, C.byref(meas), d(lin), d(qk), st_, S_, None if ii_ is None else d(ii_), None if jj_ is None else d(jj_),
               chi2_, None, None)
        return rc, _err(lib)

    assert call()[0] == 1 and "P_sym or P" in call()[1]
    m.P = d(P)
    assert call() == (1, "ctx is NULL")
    assert "model must be 1 or 2" in call(model=3)[1]
    assert "chi2 is NULL" in call(chi2_=None)[1]
    bad = ii.copy()
    bad[2] = S
    rc, msg = call(ii_=bad)
    assert rc == 1 and msg.startswith(entry + ": ") and "state index out of range at factor 2" in msg
    assert "too few states" in call(S_=0)[1]
    # the rest of what the entry refuses before the context, text and all; chained states (no index array) need F + 1 of them
    assert call(F_=-1) == (1, entry + ": negative size")
    assert call(st_=None) == (1, entry + ": NULL argument")
    assert call(ii_=None, S_=F - 1) == (1, entry + ": too few states")
    assert call(jj_=None, S_=F) == (1, entry + ": too few states")
    assert call(ii_=None, jj_=None, S_=F + 1) == (1, "ctx is NULL")
    bad = jj.copy()
    bad[1] = -1
    assert call(jj_=bad) == (1, entry + ": state index out of range at factor 1")
    assert call(jj_=bad, S_=0) == (1, entry + ": too few states")            # the count of states is looked at before the indices
    assert call(jj_=bad, chi2_=None) == (1, entry + ": chi2 is NULL")
    assert call(F_=0, chi2_=None, st_=None) == (1, "ctx is NULL")            # F == 0 is a no-op: nothing to refuse


def test_total_workspace_size(lib):
    n = [lib.cpi_factor_cost_total_doubles(F) for F in (-5, 0, 1, 2, 4095, 4096, 4097, 32768, 32769, 32768 + 5, 10 ** 6, 10 ** 9, 2 ** 31 - 1)]
    assert all(v >= 1 for v in n) and n == sorted(n)
    assert n[7] == 1 and n[8] > 1                          # from 32769 factors up the reduction has a second level
    assert n[10] == 1 + (10 ** 6 + 4095) // 4096


# ---------------------------------------------------------------- host restatement
@pytest.fixture(scope="module")
def hs():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in [_SRC] + _HDRS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB, _SRC])
    lib = C.CDLL(_LIB)
    vp = C.c_void_p
    lib.hst_retract.argtypes = [C.c_longlong, vp, vp, vp]
    lib.hst_local.argtypes = [C.c_longlong, vp, vp, vp]
    lib.hst_cost.argtypes = [C.c_int, C.c_longlong] + [vp] * 17 + [C.c_int, vp, vp]
    return lib


def test_no_case_sits_on_a_sign_decision():
    states, delta, other, mag = tc.states_and_steps()
    assert sorted(set(mag[:64])) == list(range(len(tc.MAGS)))        # every wavefront mixes the magnitudes
    assert (tc.retract_margins(states, delta) >= tc.MARGIN_MIN).all()
    assert (tc.local_margins(states, other) >= tc.MARGIN_MIN).all()
    assert np.abs(states[:, 13:]).max() > 1e6 and (np.linalg.norm(delta[:, :3], axis=1) == 0).sum() > 300


def test_hostsim_retract_and_local_match_the_oracle(hs):
    states, delta, other, mag = tc.states_and_steps()
    S = states.shape[0]
    want_r, want_l, want_z = tc.oracle_results()
    got = np.full((S, 16), np.nan)
    assert hs.hst_retract(S, states.ctypes.data, delta.ctypes.data, got.ctypes.data) == 0
    e = tc.quat_dev(got, want_r)
    print("hostsim retract vs oracle, quaternion, per |dtheta|: %s" % tc.per_mag(e, mag))
    assert e.max() <= REG_FACTOR
    assert np.array_equal(got[:, 4:], states[:, 4:] + delta[:, 3:])          # the IEEE sums, bit for bit
    assert np.array_equal(got[:, 4:], want_r[:, 4:])
    zero = np.zeros_like(delta)
    gz = np.full((S, 16), np.nan)
    assert hs.hst_retract(S, states.ctypes.data, zero.ctypes.data, gz.ctypes.data) == 0
    assert tc.quat_dev(gz, want_z).max() <= REG_FACTOR and np.array_equal(gz[:, 4:], states[:, 4:])
    assert np.abs(gz[:, :4] - states[:, :4]).max() > 1e-9                    # quat_multiply(identity, q) normalises and flips: no copy
    xi = np.full((S, 15), np.nan)
    assert hs.hst_local(S, states.ctypes.data, other.ctypes.data, xi.ctypes.data) == 0
    el = tc.local_rot_dev(xi, want_l)
    print("hostsim local vs oracle, rotation part: %.1e" % el.max())
    assert el.max() <= REG_FACTOR
    assert np.array_equal(xi[:, 3:], other[:, 4:] - states[:, 4:]) and np.array_equal(xi[:, 3:], want_l[:, 3:])


@pytest.mark.parametrize("model", [1, 2])
def test_hostsim_cost_matches_the_longdouble_reference(hs, model):
    from oracle import oracle_py as op
    F = 95                                                                   # five rounds of the regimes
    b = fc.mixed(model, F)
    bc = fc.base_cases(model)
    base = b["base"]
    out = op.oracle().run(op.make_params(model, 0, 1), np.ascontiguousarray(bc["knots"][base]), np.ascontiguousarray(bc["lin"][base]),
                          np.ascontiguousarray(bc["q_k_lin"][base]))
    Rrc = sqrt_info_longdouble(np.asarray(out["P"]).reshape(F, 15, 15))       # [row][col]; P is symmetric
    R = np.ascontiguousarray(Rrc.transpose(0, 2, 1).reshape(F, 225))          # column-major, used as given from here on
    tri = np.ascontiguousarray(np.stack([R[:, k * 15 + i] for k in range(15) for i in range(k + 1)], axis=1))
    ref = fc.evaluate_error_longdouble(model, b["rec"], b["xi"], b["xj"])
    assert (ref[3] >= fc.MARGIN_MIN).all()
    want = np.asarray(fc.whitened_longdouble(ref, R)[0], dtype=np.longdouble)
    meas, lin, qlin = fc.meas_of(b["rec"])
    grav = np.ascontiguousarray(b["rec"][0, fc.C_GRAV])
    assert (b["rec"][:, fc.C_GRAV] == grav).all()
    xi, xj = np.ascontiguousarray(b["xi"]), np.ascontiguousarray(b["xj"])
    d = lambda x: x.ctypes.data
    got = {}
    for name, Rm, flag in (("dense", R, 0), ("tri", tri, 1)):
        werr, chi2 = np.full((F, 15), np.nan), np.full(F, np.nan)
        assert hs.hst_cost(model, F, d(grav), d(meas["DT"]), d(meas["alpha"]), d(meas["beta"]), d(meas["q"]), d(meas["J_q"]), d(meas["J_b"]),
                           d(meas["J_a"]), d(meas["H_b"]), d(meas["H_a"]), d(meas["O_b"]), d(meas["O_a"]), d(lin), d(qlin), d(xi), d(xj),
                           d(Rm), flag, d(werr), d(chi2)) == 0
        got[name] = (werr, chi2)
    werr, chi2 = got["dense"]
    assert np.array_equal(got["tri"][0], werr) and np.array_equal(got["tri"][1], chi2)
    g = {1: 1.0e-12, 2: 2.1e-12}[model]                                       # the whitened REG gates of profiles/factor_edges.md
    e = fc.rel_err(werr, want)
    print("hostsim cost model %d: werr vs longdouble %.1e (gate %.1e)" % (model, e.max(), g))
    assert e.max() <= g
    assert np.array_equal(chi2, tc.chi2_documented(werr))                     # the documented summation, bit for bit
    chi2_ref = np.asarray((want * want).sum(axis=1), dtype=np.float64)
    assert (np.abs(chi2 - chi2_ref) <= tc.chi2_gate(g, want)).all()
