"""CPU: cpi_state_fix_batch without a GPU -- declarations, contract, and the arithmetic.

1. cpi_state_fix_batch and its _host form are declared in include/cpi_amd.h between cpi_chain_accept_batch and the device sets, listed
   among the additions within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_fix has a resource report of its own with exactly its
   four kernels, scratch 0, and no other report names them.
2. Every refusal and every forbidden overlap, through ctypes with a NULL context: the refusals come before the context is looked at,
   the _host form's validation of mfirst too.
3. The host twin (tests/hostsim/hostsim_fix.cpp over chn::state_fix of cpi_math.hpp, compiled with -ffp-contract=off): bit for bit
   against the float64 restatement of tests/fix_cases.py, within the gates of the longdouble reference, for all four kinds.
4. Mutations of the twin, built in tmp_path, that must fail: a dropped sign flip, sel of the pose kind shifted by one block, the
   entries of the second round of sixteen lanes skipped.
5. The end-to-end problem of tests/test_gpu_fix.py has positive definite undamped systems.
6. The edges of the contract on the twin: the builders of fx.edge_case against the reference (the honesty condition of
   tests/test_gpu_fix_edges.py), and the checks of tests/fix_edge_checks.py -- an exactly zero residual, a broken mfirst on padded
   arrays, one NaN in every place -- each of which fails on a twin with the defect it is there for: no clamp, a position residual that
   reads x.v, chi2 multiplied by the weight.
The figures are printed before anything is asserted (pytest -s shows them; profiles/state_fix.md records them)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fix_cases as fx
from tests import fix_edge_checks as fe
from tests import test_marginals_cpu as tm
from tests.test_lm_cpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_fix.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_fix.so")
_MATH = os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")
KERNELS = ["cpi_fix_kernel<%d>" % k for k in range(4)]
_ARGS = ("cpi_ctx *ctx, int64_t S, int64_t M, int32_t kind, const int64_t *mfirst, const double *states, const double *z, const double *R, "
         "const double *weight, const double *base, const double *pcost_base, double *out, double *pcost, double *chi2")
ENTRIES = ("cpi_state_fix_batch", "cpi_state_fix_batch_host")


@pytest.fixture(scope="module")
def lib():
    from cpi_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- declarations
def test_symbols_are_declared_bound_and_exported(lib):
    from cpi_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cpi_amd.h")).read())
    for s in ENTRIES:
        assert re.search(r" T %s$" % s, dyn, re.M), s
        assert getattr(lib, s).restype is C.c_int and len(getattr(lib, s).argtypes) == _ARGS.count(",") + 1, s
        assert flat.split("int %s(" % s, 1)[1].split(");", 1)[0] == _ARGS, s
        assert s in flat.split("typedef struct cpi_ctx")[0].split("additions within 3", 1)[1], s
    assert lib.cpi_abi_version() == 3
    assert flat.index("int cpi_chain_accept_batch(") < flat.index("int cpi_state_fix_batch(") < flat.index("/* ---- Device sets")
    assert "enum { CPI_FIX_POSITION = 0, CPI_FIX_VELOCITY = 1, CPI_FIX_ORIENTATION = 2, CPI_FIX_POSE = 3 };" in flat
    doc = flat.split("int cpi_chain_accept_batch(")[1].split("int cpi_state_fix_batch(")[0]
    for text in ("PARITY UNPINNED", "12 13 14", "6 7 8", "0 1 2 12 13 14", "negated when qd.w < 0", "i + k (k + 1) / 2", "fma(0.5 w_m, chi2, pcost)",
                 "entry 135 is written as 0.0", "WITHOUT the weight", "never in place", "clamped into [0, M]", "allocates nothing",
                 "without parallel branches", "overlaps", "before the context is looked at", "robust kernels", "between-state", "mixed kinds",
                 "right Jacobian"):
        assert text in doc, text
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## 3q." in integ
    sec = integ.split("\n## 3q.", 1)[1].split("\n## ", 1)[0]
    for text in ("state_fix", "fix_offsets", "chain_lm", "fixes=", "chi2=", "weight", "base="):
        assert text in sec, text
    for name, text in (("DESIGN.md", "3.5f"), ("README.md", "state_fix"), (os.path.join("profiles", "README.md"), "state_fix.md")):
        assert text in open(os.path.join(ROOT, name)).read(), name


def test_kernels_have_a_unit_and_a_report_of_their_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_fix"][-2:] == ["cpi_fix.hip", "cpi_fix_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_fix"]
    assert os.path.basename(own) == "resource_usage_fix.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == KERNELS
    for k in KERNELS:
        regs, scratch, occ, lds = rows[k]
        print("%s: %d registers, scratch %d, occupancy %d, LDS %d" % (k, regs, scratch, occ, lds))
        assert scratch == 0 and regs <= 128 and occ >= 4 and lds == 4 * 137 * 8
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_fix_kernel" in open(path).read()) == (unit == "cpi_fix"), path
    body = open(_MATH).read().split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    for sig in ("CPI_HD void fix_residual(const NavState &x, const double *z, double *e)", "CPI_HD double fix_vectors(const double *R, const double *e, double *wh, double *u)",
                "CPI_HD double fix_term(const double *R, const double *u, int t)", "THE ORDER OF EVERY SUM"):
        assert sig in body, sig
    assert body.index("CPI_HD double prior_eta_row(") < body.index("struct Fix {")
    kern = open(os.path.join(build.CSRC, "cpi_fix_kernels.hpp")).read()
    for call in ("chn::fix_residual<K>(", "chn::fix_vectors<T::D>(", "chn::fix_term<T::D>(", "st16_nt(", "template <int K>"):
        assert call in kern, call
    twin = open(_SRC).read()
    assert "chn::state_fix<K>(" in twin and "chn::fix_residual<" in twin


def test_engine_module_and_facade_have_the_entry():
    import torch
    import cpi_amd
    E = cpi_amd.Engine
    assert "self.lib.cpi_state_fix_batch," in inspect.getsource(E.state_fix) and "self.lib.cpi_state_fix_batch_host," in inspect.getsource(E.state_fix_host)
    p = inspect.signature(E.state_fix).parameters
    assert list(p)[1:6] == ["states", "kind", "z", "R", "mfirst"]
    assert [(n, p[n].default) for n in list(p)[6:]] == [("weight", None), ("base", None), ("pcost_base", None), ("out", None), ("pcost", None),
                                                        ("chi2", None), ("want_rows", True), ("want_cost", True)]
    assert inspect.signature(E.chain_lm).parameters["fixes"].default is None
    src = inspect.getsource(E.chain_lm)
    src = src[src.index("for it in range(iterations)"):]
    order = [src.index(s) for s in ("self.prior_relinearize(states", "self._lm_fixes(states", "self.factor_hessian(", "self.chain_solve(",
                                    "self.prior_relinearize(b[\"trial\"]", "self._lm_fixes(b[\"trial\"]", "self.chain_accept(")]
    assert order == sorted(order)
    for word in (".item()", ".cpu()", ".tolist()", "synchronize"):
        assert word not in src and word not in inspect.getsource(E._lm_fixes) and word not in inspect.getsource(E.fix_offsets), word
    for name in ("state_fix", "state_fix_host", "fix_offsets"):
        assert callable(getattr(cpi_amd, name)), name
    assert E.FIX_KINDS == {k: i for i, k in enumerate(fx.KINDS)}
    # fix_offsets: the CSR offsets of a non-decreasing index, trailing and leading states without fixes included
    idx = torch.tensor([1, 1, 2, 5, 5, 5], dtype=torch.int64)
    assert cpi_amd.fix_offsets(idx, 8).tolist() == [0, 0, 2, 3, 3, 3, 6, 6, 6]
    assert cpi_amd.fix_offsets(idx.to(torch.int32), 6).dtype == torch.int64
    assert cpi_amd.fix_offsets(idx[:0], 2).tolist() == [0, 0, 0]
    host = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_state_fix_batch_host(" in host and re.search(r"inline FixRows state_fix\(const Context &ctx", host)
    prog = open(os.path.join(ROOT, "tests", "cpp", "test_fix.cpp")).read()
    assert "state_fix(ctx, CPI_FIX_POSITION, states, z, R, mfirst)" in prog and "pos.rows, pos.pcost)" in prog


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


def _ptr(x, off=0):
    return None if x is None else x.ctypes.data + off


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", [0, 3])
def test_refusals_come_before_the_context(lib, entry, kind):
    f = getattr(lib, entry)
    S, M = 4, 6
    a = {"mfirst": np.array([0, 2, 2, 5, 6], dtype=np.int64), "states": np.zeros(S * 16), "z": np.zeros(M * fx.ZN[kind]), "R": np.zeros(M * fx.RN[kind]),
         "weight": np.ones(M), "base": np.zeros(S * 136), "pcost_base": np.zeros(S), "out": np.zeros(S * 136), "pcost": np.zeros(S), "chi2": np.zeros(M)}
    names = list(a)

    def call(S_=S, M_=M, kind_=kind, **kw):
        v = {k: _ptr(x) for k, x in a.items()}
        v.update(kw)
        return f(None, S_, M_, kind_, *[v[n] for n in names]), _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")                                       # a valid call gets as far as the context
    for k in ("weight", "base", "pcost_base", "out", "pcost", "chi2"):
        assert call(**{k: None}) == (1, "ctx is NULL"), k
    assert call(out=None, pcost=None) == (1, "ctx is NULL") and call(out=None, chi2=None) == (1, "ctx is NULL")
    refused("negative size", S_=-1)
    refused("negative size", M_=-1)
    refused("unknown kind", kind_=4)
    refused("unknown kind", kind_=-1)
    refused("mfirst or states is NULL", mfirst=None)
    refused("mfirst or states is NULL", states=None)
    refused("z or R is NULL", z=None)
    refused("z or R is NULL", R=None)
    zero = np.zeros(S + 1, dtype=np.int64)
    assert call(M_=0, z=None, R=None, weight=None, chi2=None, mfirst=_ptr(zero)) == (1, "ctx is NULL")   # M == 0: a copy of the base
    refused("all NULL", out=None, pcost=None, chi2=None)
    for o in ("out", "pcost", "chi2"):
        for i in ("mfirst", "states", "z", "R", "weight", "base", "pcost_base"):
            refused("overlaps", **{o: _ptr(a[i], a[i].nbytes - 8)})      # (the arrays may be neighbours on the heap: which output is named varies)
            refused("overlaps", **{i: _ptr(a[o], 0)})
    refused("out overlaps", pcost=_ptr(a["out"], 8))
    if entry.endswith("_host"):                                               # mfirst is validated first, and the text names the state
        for bad, s in (([0, 2, 1, 5, 6], 1), ([-1, 2, 2, 5, 6], 0), ([0, 2, 2, 5, 7], 3)):
            refused("the fixes of state %d " % s, mfirst=_ptr(np.array(bad, dtype=np.int64)))
        assert call(S_=0) == (1, "ctx is NULL")


# ---------------------------------------------------------------- the twin
def _bind(path):
    lib = C.CDLL(path)
    vp, ll = C.c_void_p, C.c_longlong
    lib.hsf_state_fix.argtypes = [ll, ll, C.c_int] + [vp] * 10
    lib.hsf_residual.argtypes = [ll, ll, C.c_int] + [vp] * 4
    return lib


@pytest.fixture(scope="module")
def hf():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in (_SRC, _MATH)):
        tm._build(_SRC, _LIB)
    return _bind(_LIB)


def _mutant(tmp_path, old, new, twin=False):
    """The twin with old replaced by new in cpi_math.hpp -- or, with twin=True, in hostsim_fix.cpp itself (its range handling)."""
    text, src = open(_MATH).read(), open(_SRC).read()
    assert (src if twin else text).count(old) == 1, old
    os.makedirs(tmp_path / "cpi_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "hostsim")
    (tmp_path / "cpi_amd" / "csrc" / "cpi_math.hpp").write_text(text if twin else text.replace(old, new))
    (tmp_path / "tests" / "hostsim" / "hostsim_fix.cpp").write_text(src.replace(old, new) if twin else src)
    out = str(tmp_path / "libmutant.so")
    tm._build(str(tmp_path / "tests" / "hostsim" / "hostsim_fix.cpp"), out)
    return _bind(out)


def twin(h, c, weight=True, base=True, rows=True, cost=True, mfirst=None, z=None, states=None):
    """hsf_state_fix on case c -> (out [S, 136], pcost [S], chi2 [M]) with sentinels behind every array (None where not asked for)."""
    out = np.full((c.S + 1, 136), fx.SENTINEL) if rows else None
    pcost = np.full(c.S + 1, fx.SENTINEL) if cost else None
    chi2 = np.full(c.M + 1, fx.SENTINEL)
    z = np.ascontiguousarray(c.z if z is None else z)
    st = np.ascontiguousarray(c.states if states is None else states)
    mf = np.ascontiguousarray(c.mfirst if mfirst is None else mfirst, dtype=np.int64)
    assert h.hsf_state_fix(c.S, c.M, c.kind, _ptr(mf), _ptr(st), _ptr(z), _ptr(c.R), _ptr(c.weight) if weight else None, _ptr(c.base) if base else None,
                           _ptr(c.pcost_base) if base else None, _ptr(out), _ptr(pcost), _ptr(chi2)) == 0
    assert chi2[c.M] == fx.SENTINEL and (out is None or (out[c.S] == fx.SENTINEL).all()) and (pcost is None or pcost[c.S] == fx.SENTINEL)
    return (None if out is None else out[:c.S]), (None if pcost is None else pcost[:c.S]), chi2[:c.M]


def twin_residual(h, c):
    e = np.zeros((c.M, fx.D[c.kind]))
    assert h.hsf_residual(c.S, c.M, c.kind, _ptr(c.mfirst), _ptr(c.states), _ptr(c.z), _ptr(e)) == 0
    return e


def test_the_inputs_are_honest():
    """Every case of the full size holds states with 0, 1, 2 and 17 fixes, every wavefront of four mixes them, the last states have none;
    the rotation cases reach qd.w < 0 before the flip, and residual rotations of 1e-9, 1 and 3.1 rad."""
    assert max(fx.SIZES) == len(fx.COUNTS) and fx.COUNTS[-2:] == (0, 0)
    for w in range(0, len(fx.COUNTS), 4):
        assert len(set(fx.COUNTS[w:w + 4])) >= min(3, len(fx.COUNTS[w:w + 4]))
    for kind in range(4):
        c = fx.case(kind, 9)
        assert set(c.counts.tolist()) == {0, 1, 2, 17} and c.M == sum(fx.COUNTS) and c.mfirst[-1] == c.M
        assert sorted({len(set(fx.case(kind, S).counts.tolist())) for S in fx.SIZES}) == [1, 3, 4]
        if kind >= 2:
            own = c.owner()
            w = np.array([(fx.quat_mul_ld(c.z[m, :4], np.concatenate([-c.states[own[m], :3], c.states[own[m], 3:4]]))[0][3]) for m in range(c.M)], dtype=np.float64)
            ang = 2 * np.arccos(np.minimum(np.abs(w), 1.0))
            assert (w < 0).sum() >= 5 and (w > 0).sum() >= 5
            for a in (1.0, 3.1):
                assert (np.abs(ang - a) < 1e-6).any(), a
            e = np.array([np.asarray(fx.residual_ld(kind, c.states[own[m]], c.z[m])[0][:3], dtype=np.float64) for m in range(c.M)])
            assert (np.abs(np.linalg.norm(e, axis=1) - 1e-9) < 1e-12).any()


@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_twin_against_the_reference_and_the_documented_order(hf, kind):
    worst = {}
    for S in fx.SIZES:
        c = fx.case(kind, S)
        for weight, base in ((True, True), (False, False)):
            out, pcost, chi2 = twin(hf, c, weight, base)
            d_out, d_pc, d_chi2 = fx.documented(c, twin_residual(hf, c), weight, base)
            assert same_bits(out, d_out) and same_bits(pcost, d_pc) and same_bits(chi2, d_chi2), (S, weight, base)    # bit for bit
            m = fx.metrics(out, pcost, chi2, fx.reference(c, weight, base))
            for k, v in m.items():
                worst[k] = max(worst.get(k, 0.0), v)
            none, pc_only, chi_only = twin(hf, c, weight, base, rows=False)
            assert none is None and same_bits(pc_only, pcost) and same_bits(chi_only, chi2)
    print("twin, %s: %s (gates %s)" % (fx.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), fx.GATE_HOST))
    for k, v in worst.items():
        assert v <= fx.GATE_HOST[k], (k, v)


@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_twin_exact_properties(hf, kind):
    c = fx.case(kind, 9)
    out, pcost, chi2 = twin(hf, c)
    none = c.counts == 0
    assert same_bits(out[none, :135], c.base[none, :135]) and same_bits(pcost[none], c.pcost_base[none]) and (out[:, 135] == 0.0).all()
    z_out, z_pc, _ = twin(hf, c, base=False)
    assert (z_out[none] == 0.0).all() and (z_pc[none] == 0.0).all()
    w0 = fx.Case(kind, fx.COUNTS)                                             # weight 0: the base as numbers, chi2 still the unweighted value
    w0.weight = np.zeros(w0.M)
    o0, p0, c0 = twin(hf, w0)
    assert np.array_equal(o0[:, :135], w0.base[:, :135]) and np.array_equal(p0, w0.pcost_base) and same_bits(c0, chi2)
    for S in (1, 3, 4, 5):                                                    # a state's bits: its own data only
        o, p, x2 = twin(hf, fx.case(kind, S))
        assert same_bits(o, out[:S]) and same_bits(p, pcost[:S]) and same_bits(x2, chi2[:len(x2)])
    if kind >= 2:                                                             # z and -z: one attitude, equal as numbers
        z = c.z.copy()
        z[:, :4] = -z[:, :4]
        o, p, x2 = twin(hf, c, z=z)
        assert np.array_equal(o, out) and np.array_equal(p, pcost) and np.array_equal(x2, chi2)
        st = c.states.copy()
        st[:, :4] = -st[:, :4]
        o, p, x2 = twin(hf, c, states=st)
        assert np.array_equal(o, out) and np.array_equal(p, pcost) and np.array_equal(x2, chi2)
    bad = c.z.copy()                                                          # a NaN measurement: that state alone
    m = int(c.mfirst[5]) + 3
    bad[m, 0] = np.nan
    o, p, x2 = twin(hf, c, z=bad)
    keep = np.arange(c.S) != 5
    assert same_bits(o[keep], out[keep]) and same_bits(p[keep], pcost[keep]) and np.isnan(p[5]) and np.isnan(o[5]).any() and np.isnan(x2[m])
    broken = np.array([-3, 40, 2, 1000, -1, 5, 0, 7, 100, -100], dtype=np.int64)   # clamped into [0, M]: nothing outside is touched
    twin(hf, c, mfirst=broken)


MUTATIONS = {
    "a dropped sign flip": ("    if (r.w < 0) { r.x = -r.x; r.y = -r.y; r.z = -r.z; r.w = -r.w; }\n", "\n", "orientation"),
    "sel of the pose kind shifted by one block": ("(a < 3 ? a : 9 + a)", "(a < 3 ? a : 6 + a)", "pose"),
    "the entries of the second round of sixteen lanes skipped": ("for (int t = 0; t < T::NT; t++) acc[t] = fma(w,", "for (int t = 0; t < T::NT && t < 16; t++) acc[t] = fma(w,",
                                                                "pose"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_wrong_term_fails_its_gate(hf, tmp_path, what):
    """The twin with one term wrong, built in tmp_path: test_twin_against_the_reference_and_the_documented_order of the named kind leaves
    its gates by orders of magnitude (and, for the sign flip, test_twin_exact_properties no longer finds z and -z equal)."""
    old, new, name = MUTATIONS[what]
    mutant = _mutant(tmp_path, old, new)
    c = fx.case(fx.KINDS.index(name), 9)
    ref = fx.reference(c)
    res = {}
    for who, h in (("twin", hf), ("mutant", mutant)):
        try:
            res[who] = fx.metrics(*twin(h, c), ref)
        except AssertionError:                                                # an entry that no fix touches was written
            res[who] = dict(Lam=np.inf, eta=np.inf, pcost=np.inf, chi2=np.inf)
        print("%s, %s: %s" % (what, who, ", ".join("%s %.3g" % kv for kv in sorted(res[who].items()))))
    assert all(res["twin"][k] <= fx.GATE_HOST[k] for k in res["twin"])
    assert max(res["mutant"]["Lam"], res["mutant"]["eta"]) > 1e3 * max(fx.GATE_HOST.values()), res["mutant"]
    if what == "a dropped sign flip":
        z = c.z.copy()
        z[:, :4] = -z[:, :4]
        assert not np.array_equal(twin(mutant, c, z=z)[0], twin(mutant, c)[0])


def test_the_stand_alone_twin_program(tmp_path):
    exe = str(tmp_path / "hostsim_fix_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-ffp-contract=off", "-DHOSTSIM_FIX_MAIN", "-o", exe, _SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout


# ---------------------------------------------------------------- the edges of the contract, on the twin
EDGE_CASES = [(name, kind) for name, kinds in fx.EDGE_BUILDERS for kind in kinds]


@pytest.mark.parametrize("name,kind", EDGE_CASES, ids=["%s-%s" % (n, fx.KINDS[k]) for n, k in EDGE_CASES])
def test_twin_on_the_edge_builders(hf, name, kind):
    """The honesty condition of the builders of tests/fix_cases.py: the reference and the twin agree within GATE_HOST on each of them
    before any number from the device is believed; the documented order bit for bit (the nine-state builders)."""
    c = fx.edge_case(name, kind)
    worst = {}
    for weight, base in ((True, True), (False, False)):
        out, pcost, chi2 = twin(hf, c, weight, base)
        if name != "many":
            d_out, d_pc, d_chi2 = fx.documented(c, twin_residual(hf, c), weight, base)
            assert same_bits(out, d_out) and same_bits(pcost, d_pc) and same_bits(chi2, d_chi2), (weight, base)
        for k, v in fx.metrics(out, pcost, chi2, fx.reference(c, weight, base)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("twin, %s, %s: %s (gates %s)" % (name, fx.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), fx.GATE_HOST))
    for k, v in worst.items():
        assert v <= fx.GATE_HOST[k], (k, v)
    if name == "many":                                                        # a state's bits: not S, nor where it sits
        assert c.S == fx.MANY and set(c.counts.tolist()) == {0, 1, 2, 17}
        out, pcost, chi2 = twin(hf, c)
        o, p, x2 = twin(hf, c.head(9))
        assert same_bits(o, out[:9]) and same_bits(p, pcost[:9]) and same_bits(x2, chi2[:len(x2)])
        mv, order, fixes = fx.reversed_case(c)
        o, p, x2 = twin(hf, mv)
        assert same_bits(o, np.ascontiguousarray(out[order])) and same_bits(p, np.ascontiguousarray(pcost[order])) and same_bits(x2, np.ascontiguousarray(chi2[fixes]))
    if name == "identity":                                                    # the premise: a rotation residual of exactly 0, both signs
        e = twin_residual(hf, c)[:, :3]
        assert (e == 0.0).all() and np.signbit(e).any() and not np.signbit(e).all()
    if name == "earth":                                                       # z - p is exact: the residuals of the nine-state case to 1e-9
        e, e0 = twin_residual(hf, c)[:, -3:], twin_residual(hf, fx.case(kind, 9))[:, -3:]
        assert np.abs(e - e0).max() < 2e-9 and np.abs(e).max() < 1.0


@pytest.mark.parametrize("kind", [2, 3], ids=fx.KINDS[2:])
def test_twin_exact_zero_residual(hf, kind):
    m = fe.check_exact_zero(lambda c: twin(hf, c), kind)
    for k, v in m.items():
        assert v <= fx.GATE_HOST[k], (k, v)


def twin_padded(h, p, mfirst):
    """hsf_state_fix on the interiors of the padded arrays of fe.Padded -> the whole buffers (out, pcost, chi2)."""
    c, P = p.c, fe.PAD
    out, pcost = np.full((c.S + 2, 136), np.nan), np.full(c.S + 2, np.nan)
    out[[0, -1]], pcost[[0, -1]] = fe.GUARD, fe.GUARD
    chi2 = p.big["chi2"].copy()
    mf = np.ascontiguousarray(mfirst, dtype=np.int64)
    z, R, w = p.big["z"], p.big["R"], p.big["weight"]
    assert h.hsf_state_fix(c.S, c.M, c.kind, _ptr(mf), _ptr(c.states), _ptr(z, P * z.strides[0]), _ptr(R, P * R.strides[0]), _ptr(w, P * 8),
                           _ptr(c.base), _ptr(c.pcost_base), _ptr(out, 136 * 8), _ptr(pcost, 8), _ptr(chi2, P * 8)) == 0
    return out, pcost, chi2


@pytest.mark.parametrize("kind", [0, 3], ids=["position", "pose"])
def test_twin_broken_mfirst_stays_inside(hf, lib, kind):
    fe.check_broken_mfirst(lambda p, mf: twin_padded(hf, p, mf), kind)
    c = fx.case(kind, 9)                                                      # the host form refuses each of them, naming a state
    for what, mf, _ in fe.broken_mfirsts(c):
        a = [np.ascontiguousarray(x) for x in (mf, c.states, c.z, c.R, c.weight, c.base, c.pcost_base, np.zeros((c.S, 136)), np.zeros(c.S), np.zeros(c.M))]
        rc = lib.cpi_state_fix_batch_host(None, c.S, c.M, kind, *[_ptr(x) for x in a])
        print("%s: %s" % (what, _err(lib)))
        assert rc == 1 and re.search(r"the fixes of state \d+ ", _err(lib)), what


@pytest.mark.parametrize("kind", range(4), ids=fx.KINDS)
def test_twin_nan_stays_where_it_is(hf, kind):
    assert fe.check_nan_locality(lambda c: twin(hf, c), kind) >= 24


EDGE_MUTATIONS = {
    "a missing mfirst clamp": ("{ return v < 0 ? 0 : (v > M ? M : v); }", "{ return v; }", True, "mfirst"),
    "a position residual that reads x.v": ("e[0] = z[0] - x.p.x; e[1] = z[1] - x.p.y; e[2] = z[2] - x.p.z; }\n    if (K == FIX_VELOCITY)",
                                           "e[0] = z[0] - x.v.x; e[1] = z[1] - x.v.y; e[2] = z[2] - x.v.z; }\n    if (K == FIX_VELOCITY)", False, "nan"),
    "chi2 multiplied by the weight": ("if (chi2) chi2[m] = c2;", "if (chi2) chi2[m] = w * c2;", False, "nan"),
}


@pytest.mark.parametrize("what", list(EDGE_MUTATIONS))
def test_the_edge_checks_fail_when_they_should(hf, tmp_path, what):
    """The twin with one defect, built in tmp_path: the check of the edge family named in EDGE_MUTATIONS passes on the twin and fails on
    the mutant.  (The padded arrays keep a twin without the clamp inside its allocations: it reads a NaN pad or writes over a guard.)"""
    old, new, in_twin, family = EDGE_MUTATIONS[what]
    mutant = _mutant(tmp_path, old, new, twin=in_twin)
    check = {"mfirst": lambda h: fe.check_broken_mfirst(lambda p, mf: twin_padded(h, p, mf), 0),
             "nan": lambda h: fe.check_nan_locality(lambda c: twin(h, c), 0)}[family]
    check(hf)
    with pytest.raises(AssertionError):
        check(mutant)
    if family == "nan":                                                       # ... and the reference comparison of the builders sees it too
        c = fx.edge_case("earth", 0)
        m = fx.metrics(*twin(mutant, c), fx.reference(c))
        print("%s, earth: %s" % (what, m))
        assert max(m.values()) > 1e3 * max(fx.GATE_HOST.values())


# ---------------------------------------------------------------- the end-to-end problem
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "dense"])
def test_the_end_to_end_systems_are_positive_definite(ragged):
    """The undamped systems of the end-to-end cases at their starting states, with the prior and the fixes: a finite Cholesky and a
    bounded condition number for every chain (cc.Reference.check_inputs).  The ragged case is the issue's: eight chains of 2 to 6
    states, first / count / ffirst all different from chain to chain, mfirst indexing states and not chains."""
    pred, states, anchor, prior0 = fx.e2e_cpu()
    L = fx.layout(ragged)
    fixes = fx.e2e_fixes(pred, L["member"])
    n = L["count"]
    assert len(n) == 8 and n.min() == (2 if ragged else 6) and n.max() == 6 and (not ragged or sorted(set(n.tolist())) == [2, 3, 4, 5, 6])
    assert np.array_equal(np.diff(fixes[0]["mfirst"]), L["member"].astype(np.int64)) and fixes[0]["mfirst"][-1] == n.sum() == len(fixes[0]["z"])
    per_chain = np.diff(fixes[1]["mfirst"]).reshape(8, 6)
    assert (per_chain[:, 0] == 1).all() and np.array_equal(per_chain[:, 3], (n >= 4).astype(np.int64)) and per_chain.sum() == 8 + (n >= 4).sum()
    assert np.array_equal(L["ffirst"], np.concatenate([[0], np.cumsum(n - 1)[:-1]])) and len(L["keep"]) == (n - 1).sum()
    loop = fx.FixLoop(anchor, prior0, fixes, L)
    sol = loop.system(states)
    sol.check_inputs()
    print("condition numbers with the fixes: %s" % np.array2string(sol.cond, precision=3))
    assert (np.abs(loop.rows[L["member"], 120:135]).max(1) > 0).all() and (loop.rows[~L["member"]] == 0).all()
