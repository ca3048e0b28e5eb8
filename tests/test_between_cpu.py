"""CPU: cpi_state_between_batch without a GPU -- declarations, contract, and the arithmetic.

1. cpi_state_between_batch and its _host form are declared in include/cpi_amd.h behind cpi_state_fix_batch, listed among the additions
   within ABI 3 and bound in cpi_amd/_lib.py; the unit cpi_between has a resource report of its own with exactly its three kernels,
   scratch 0, and no other report names them.
2. Every refusal and every forbidden overlap, through ctypes with a NULL context: the refusals come before the context is looked at,
   the _host form's validation of mfirst and of the state indices too; the exact in-place forms are let through.
3. The host twin (tests/hostsim/hostsim_between.cpp over chn::factor_between of cpi_math.hpp, compiled with -ffp-contract=off): bit for
   bit against the float64 restatement of tests/between_cases.py from e and J for all three kinds, and for the position kind from the
   inputs (no quaternion normalisation separates the two there; the orientation and pose kinds go through quat_multiply); within the
   gates of the longdouble reference; in place bit for bit the out-of-place call.
4. The Jacobian of the contract's table against central differences of the longdouble residual through a longdouble retract, the
   rotation blocks where e_th = 0, the position blocks anywhere; and g = minus the gradient of 0.5 w chi2 for every kind (the
   orientation kind 1e-4 rad from e_th = 0, within the first-order bound of the flat right Jacobian).
5. Mutations of the twin, built in tmp_path, that must fail: a dropped term, R_ij with i and j swapped, a transposed R_i.
6. The end-to-end problem of tests/test_gpu_between.py has positive definite undamped systems.
The figures are printed before anything is asserted (pytest -s shows them; profiles/state_between.md records them)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import between_cases as bc
from tests import fix_cases as fx
from tests import lm_cases as lc
from tests import test_marginals_cpu as tm
from tests.test_lm_cpu import same_bits

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_between.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_between.so")
_MATH = os.path.join(ROOT, "cpi_amd", "csrc", "cpi_math.hpp")
KERNELS = ["cpi_between_kernel<%d>" % k for k in range(3)]
_ARGS = ("cpi_ctx *ctx, int64_t F, int64_t M, int32_t kind, const int64_t *mfirst, const double *states, int64_t S, const int32_t *idx_i, "
         "const int32_t *idx_j, const double *z, const double *R, const double *weight, const double *hess_base, const double *chi2_base, "
         "double *hess, double *chi2, double *chi2_m")
ENTRIES = ("cpi_state_between_batch", "cpi_state_between_batch_host")


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
    assert flat.index("int cpi_state_fix_batch(") < flat.index("int cpi_state_between_batch(") < flat.index("/* ---- Device sets")
    assert "enum { CPI_BETWEEN_POSITION = 0, CPI_BETWEEN_ORIENTATION = 1, CPI_BETWEEN_POSE = 2 };" in flat
    doc = flat.split("int cpi_state_fix_batch(")[1].split("int cpi_state_between_batch(")[0]
    for text in ("PARITY UNPINNED", "0 1 2 12 13 14 27 28 29 30", "0 1 2 15 16 17 30", "0 1 2 12 13 14 15 16 17 27 28 29 30", "negated when qd.w < 0",
                 "r + k (k + 1) / 2", "fma(w_m, P_ab, hess[f][(a, b)])", "fma(w_m, chi2_m, chi2[f])", "WITHOUT the weight", "IN PLACE", "EXACTLY",
                 "clamped into [0, M]", "clamped into [0, S)", "allocates nothing", "without parallel branches", "overlaps",
                 "before the context is looked at", "robust kernels", "non-adjacent states", "mixed kinds", "right Jacobian", "central differences",
                 "-[y x]", "d e_th / d theta_j = -I", "minus the gradient"):
        assert text in doc, text
    for name in ("README.md", "INTEGRATION.md"):                              # "relative measurements" left the out-of-scope sentences
        assert "relative measurements" not in open(os.path.join(ROOT, name)).read().replace("\n", " "), name
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## 3r." in integ
    sec = integ.split("\n## 3r.", 1)[1].split("\n## ", 1)[0]
    for text in ("state_between", "fix_offsets", "chain_lm", "betweens=", "chi2_m", "weight", "hess_base", "in place"):
        assert text in sec, text
    for name, text in (("DESIGN.md", "3.5g"), ("README.md", "state_between"), (os.path.join("profiles", "README.md"), "state_between.md")):
        assert text in open(os.path.join(ROOT, name)).read(), name
    assert os.path.exists(os.path.join(ROOT, "profiles", "state_between.md"))


def test_kernels_have_a_unit_and_a_report_of_their_own(lib):
    from cpi_amd import build
    assert build.UNITS["cpi_between"] == build.DEVICE + ["cpi_between.hip", "cpi_between_kernels.hpp"]
    own = build.UNIT_REPORTS["cpi_between"]
    assert os.path.basename(own) == "resource_usage_between.txt"
    rows = {}
    for ln in open(own).read().splitlines()[1:]:
        name, sgpr, vgpr, agpr, scratch, occ, lds = ln.rsplit(None, 6)
        rows[name.strip()] = (int(vgpr) + int(agpr), int(scratch), int(occ), int(lds))
    assert sorted(rows) == KERNELS
    for k, d in zip(KERNELS, bc.D):
        regs, scratch, occ, lds = rows[k]
        print("%s: %d registers, scratch %d, occupancy %d, LDS %d" % (k, regs, scratch, occ, lds))
        assert scratch == 0 and regs <= 256 and occ >= 2 and lds == 4 * 497 * 8 + 4 * d * 16 * 8
    for unit, path in list(build.UNIT_REPORTS.items()) + [(None, build.REPORT)]:
        assert ("cpi_between_kernel" in open(path).read()) == (unit == "cpi_between"), path
    body = open(_MATH).read().split("namespace chn {", 1)[1].split("}  // namespace chn", 1)[0]
    for sig in ("CPI_HD BetweenGeo between_geometry(const NavState &xi, const NavState &xj)", "CPI_HD void between_residual(const BetweenGeo &g, const double *z, double *e)",
                "CPI_HD void between_jcol(const BetweenGeo &g, int c, double *Jc)", "CPI_HD void between_acol(const double *R, const double *Jc, double *Ac)",
                "CPI_HD double between_term(const double *Aa, const double *Ab, int pitch)"):
        assert sig in body, sig
    assert body.index("CPI_HD double fix_term(") < body.index("struct Between {")
    kern = open(os.path.join(build.CSRC, "cpi_between_kernels.hpp")).read()
    for call in ("chn::between_geometry<K>(", "chn::between_residual<K>(", "chn::between_jcol<K>(", "chn::between_acol<T::D>(", "chn::between_term<T::D>(",
                 "chn::fix_vectors<T::D>(", "st16_nt(", "template <int K>"):
        assert call in kern, call
    twin = open(_SRC).read()
    assert "chn::factor_between<K>(" in twin and "chn::between_jcol<K>(" in twin


def test_engine_module_and_facade_have_the_entry():
    import cpi_amd
    E = cpi_amd.Engine
    assert "self.lib.cpi_state_between_batch," in inspect.getsource(E.state_between)
    assert "self.lib.cpi_state_between_batch_host," in inspect.getsource(E.state_between_host)
    p = inspect.signature(E.state_between).parameters
    assert list(p)[1:6] == ["states", "kind", "z", "R", "mfirst"]
    assert [(n, p[n].default) for n in list(p)[6:]] == [("idx_i", None), ("idx_j", None), ("weight", None), ("hess_base", None), ("chi2_base", None),
                                                        ("out", None), ("chi2", None), ("chi2_m", None), ("want_rows", True), ("want_cost", True)]
    assert inspect.signature(E.chain_lm).parameters["betweens"].default is None
    src = inspect.getsource(E.chain_lm)
    head, loop = src[:src.index("for it in range(iterations)")], src[src.index("for it in range(iterations)"):]
    order = [head.index(s) for s in ("self.factor_cost(", "self._lm_betweens(states", "self.chain_cost(")]
    assert order == sorted(order)
    order = [loop.index(s) for s in ("self.factor_hessian(", "self._lm_betweens(states", "self.chain_solve(", "self.factor_cost(",
                                     "self._lm_betweens(b[\"trial\"]", "self.chain_accept(")]
    assert order == sorted(order)
    # a call without betweens is launch for launch what it was: the three call sites pass `betweens or ()`, and the helper is one loop
    # over that list whose body is the only place an entry is issued -- nothing runs for an empty list
    assert src.count("self._lm_betweens(") == 3 and src.count("betweens or ()") == 3
    helper = inspect.getsource(E._lm_betweens)
    body = helper.split('"""')[2]
    assert body.lstrip().startswith("for b in betweens:") and all(ln.startswith("            ") for ln in body.splitlines()[2:] if ln.strip())
    assert "hess_base=hess, out=hess" in helper and "chi2_base=chi2, chi2=chi2" in helper          # in place: no buffer of their own
    for word in (".item()", ".cpu()", ".tolist()", "synchronize", "torch.zeros", "torch.empty"):
        assert word not in helper, word
    for name in ("state_between", "state_between_host"):
        assert callable(getattr(cpi_amd, name)), name
    assert E.BETWEEN_KINDS == {k: i for i, k in enumerate(bc.KINDS)}
    host = open(os.path.join(ROOT, "cpi_amd", "csrc", "cpi_host.hpp")).read()
    assert "cpi_state_between_batch_host(" in host and re.search(r"inline BetweenRows state_between\(const Context &ctx", host)


# ---------------------------------------------------------------- contract
def _err(lib):
    return (lib.cpi_last_error(None) or b"").decode()


def _ptr(x, off=0):
    return None if x is None else x.ctypes.data + off


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", [0, 2])
def test_refusals_come_before_the_context(lib, entry, kind):
    f = getattr(lib, entry)
    F, M, S = 4, 6, 5
    a = {"mfirst": np.array([0, 2, 2, 5, 6], dtype=np.int64), "states": np.zeros(S * 16), "idx_i": np.arange(F, dtype=np.int32),
         "idx_j": np.arange(1, F + 1, dtype=np.int32), "z": np.zeros(M * bc.ZN[kind]), "R": np.zeros(M * bc.RN[kind]), "weight": np.ones(M),
         "hess_base": np.zeros(F * 496), "chi2_base": np.zeros(F), "hess": np.zeros(F * 496), "chi2": np.zeros(F), "chi2_m": np.zeros(M)}
    order = ["mfirst", "states", "S", "idx_i", "idx_j", "z", "R", "weight", "hess_base", "chi2_base", "hess", "chi2", "chi2_m"]

    def call(F_=F, M_=M, kind_=kind, S_=S, **kw):
        v = {k: _ptr(x) for k, x in a.items()}
        v.update(kw)
        v["S"] = S_
        return f(None, F_, M_, kind_, *[v[n] for n in order]), _err(lib)

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(entry + ": ") and text in msg, (kw, rc, msg)

    assert call() == (1, "ctx is NULL")                                       # a valid call gets as far as the context
    for k in ("idx_i", "idx_j", "weight", "hess_base", "chi2_base", "hess", "chi2", "chi2_m"):
        assert call(**{k: None}) == (1, "ctx is NULL"), k
    assert call(hess=None, chi2=None) == (1, "ctx is NULL") and call(hess=None, chi2_m=None) == (1, "ctx is NULL")
    # exact aliasing is the in-place form
    assert call(hess=_ptr(a["hess_base"])) == (1, "ctx is NULL") and call(chi2=_ptr(a["chi2_base"])) == (1, "ctx is NULL")
    assert call(hess=_ptr(a["hess_base"]), chi2=_ptr(a["chi2_base"])) == (1, "ctx is NULL")
    refused("hess overlaps", hess=_ptr(a["hess_base"], 8))                    # ... and nothing but exact aliasing
    refused("chi2 overlaps", chi2=_ptr(a["chi2_base"], 8))
    refused("hess overlaps", hess=_ptr(a["hess_base"], 496 * 8))
    refused("negative size", F_=-1)
    refused("negative size", M_=-1)
    refused("negative size", S_=-1)
    refused("unknown kind", kind_=3)
    refused("unknown kind", kind_=-1)
    refused("mfirst or states is NULL", mfirst=None)
    refused("mfirst or states is NULL", states=None)
    refused("z or R is NULL", z=None)
    refused("z or R is NULL", R=None)
    refused("too few states", S_=0)
    refused("too few states", idx_j=None, S_=F)                               # NULL idx_j: f + 1 needs S >= F + 1
    refused("too few states", idx_i=None, idx_j=None, S_=F)
    assert call(idx_i=None, idx_j=_ptr(a["idx_i"]), S_=F) == (1, "ctx is NULL")
    zero = np.zeros(F + 1, dtype=np.int64)
    assert call(M_=0, z=None, R=None, weight=None, chi2_m=None, mfirst=_ptr(zero)) == (1, "ctx is NULL")   # M == 0: a copy of the base
    refused("all NULL", hess=None, chi2=None, chi2_m=None)
    for o in ("hess", "chi2", "chi2_m"):
        for i in ("mfirst", "states", "idx_i", "idx_j", "z", "R", "weight", "hess_base", "chi2_base"):
            refused("overlaps", **{o: _ptr(a[i], a[i].nbytes - 4)})       # (the arrays may be neighbours on the heap: which output is named varies)
            if not (o, i) in (("hess", "hess_base"), ("chi2", "chi2_base")):
                refused("overlaps", **{i: _ptr(a[o], 0)})
    refused("hess overlaps", chi2=_ptr(a["hess"], 8))
    refused("hess overlaps", chi2_m=_ptr(a["hess"], 8))
    if entry.endswith("_host"):                                               # mfirst and the indices are validated first, and the text names the factor
        for bad, k in (([0, 2, 1, 5, 6], 1), ([-1, 2, 2, 5, 6], 0), ([0, 2, 2, 5, 7], 3)):
            refused("the measurements of factor %d " % k, mfirst=_ptr(np.array(bad, dtype=np.int64)))
        refused("state index out of range at factor 2", idx_i=_ptr(np.array([0, 1, 5, 3], dtype=np.int32)))
        refused("state index out of range at factor 0", idx_j=_ptr(np.array([-1, 1, 2, 3], dtype=np.int32)))
        assert call(F_=0) == (1, "ctx is NULL")


# ---------------------------------------------------------------- the twin
def _bind(path):
    lib = C.CDLL(path)
    vp, ll = C.c_void_p, C.c_longlong
    lib.hsb_state_between.argtypes = [ll, ll, C.c_int, vp, vp, ll] + [vp] * 10
    lib.hsb_jacobian.argtypes = [C.c_int] + [vp] * 5
    return lib


@pytest.fixture(scope="module")
def hb():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in (_SRC, _MATH)):
        tm._build(_SRC, _LIB)
    return _bind(_LIB)


def _mutant(tmp_path, old, new, twin=False):
    """The twin with old replaced by new in cpi_math.hpp -- or, with twin=True, in hostsim_between.cpp itself (its ranges and pointers)."""
    text, src = open(_MATH).read(), open(_SRC).read()
    assert (src if twin else text).count(old) == 1, old
    os.makedirs(tmp_path / "cpi_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "hostsim")
    (tmp_path / "cpi_amd" / "csrc" / "cpi_math.hpp").write_text(text if twin else text.replace(old, new))
    (tmp_path / "tests" / "hostsim" / "hostsim_between.cpp").write_text(src.replace(old, new) if twin else src)
    out = str(tmp_path / "libmutant.so")
    tm._build(str(tmp_path / "tests" / "hostsim" / "hostsim_between.cpp"), out)
    return _bind(out)


def twin(h, c, weight=True, base=True, rows=True, cost=True, inplace=False, z=None, mfirst=None, alias=None, bases=None, padded=None):
    """hsb_state_between on case c -> (hess [F, 496], chi2 [F], chi2_m [M]) with sentinels behind every array (None where not asked for).
    alias = (hess in place, chi2 in place) and bases = (hess_base given, chi2_base given) where the two arrays differ (inplace and base
    set both).  padded: a between_edge_checks.Padded of the case -- z, R, weight, the states and chi2_m are the interiors of its arrays,
    the inputs are compared with what they were, and chi2_m comes back as the WHOLE buffer [M + 2 PAD]."""
    hess = np.full((c.F + 1, 496), bc.SENTINEL) if rows else None
    chi2 = np.full(c.F + 1, bc.SENTINEL) if cost else None
    chi2_m = np.full(c.M + 1, bc.SENTINEL)
    a_h, a_c = (inplace, inplace) if alias is None else alias
    b_h, b_c = (base, base) if bases is None else bases
    hb_, cb_ = (c.base if b_h else None), (c.chi2_base if b_c else None)
    if a_h and rows:
        assert b_h
        hess[:c.F] = c.base
        hb_ = hess
    if a_c and cost:
        assert b_c
        chi2[:c.F] = c.chi2_base
        cb_ = chi2
    z = np.ascontiguousarray(c.z if z is None else z)
    mf = np.ascontiguousarray(c.mfirst if mfirst is None else mfirst, dtype=np.int64)
    if padded is not None:
        p, big = padded, padded.big
        was = {k: v.copy() for k, v in big.items()}
        x2 = big["chi2_m"].copy()
        inner = lambda a, n: _ptr(a, n * a.strides[0])
        assert h.hsb_state_between(c.F, c.M, c.kind, _ptr(mf), inner(big["states"], p.PADS), c.S, _ptr(c.idx_i), _ptr(c.idx_j), inner(big["z"], p.PAD),
                                   inner(big["R"], p.PAD), inner(big["weight"], p.PAD) if weight else None, _ptr(hb_), _ptr(cb_), _ptr(hess), _ptr(chi2),
                                   inner(x2, p.PAD)) == 0
        assert all(same_bits(big[k], was[k]) for k in big), "an input was written"
        chi2_m = np.concatenate([x2, [bc.SENTINEL]])
    else:
        assert h.hsb_state_between(c.F, c.M, c.kind, _ptr(mf), _ptr(c.states), c.S, _ptr(c.idx_i), _ptr(c.idx_j), _ptr(z), _ptr(c.R),
                                   _ptr(c.weight) if weight else None, _ptr(hb_), _ptr(cb_), _ptr(hess), _ptr(chi2), _ptr(chi2_m)) == 0
    assert chi2_m[-1] == bc.SENTINEL and (hess is None or (hess[c.F] == bc.SENTINEL).all()) and (chi2 is None or chi2[c.F] == bc.SENTINEL)
    return (None if hess is None else hess[:c.F]), (None if chi2 is None else chi2[:c.F]), chi2_m[:-1]


def twin_e_J(h, kind, xi, xj, z):
    e, J = np.zeros(bc.D[kind]), np.zeros((bc.D[kind], 30))
    xi, xj, z = (np.ascontiguousarray(a, dtype=np.float64) for a in (xi, xj, z))
    assert h.hsb_jacobian(kind, _ptr(xi), _ptr(xj), _ptr(z), _ptr(e), _ptr(J)) == 0
    return e, J


def twin_all_e_J(h, c):
    fi, fj = c.pairs()
    own = c.owner()
    pairs = [twin_e_J(h, c.kind, c.states[fi[own[m]]], c.states[fj[own[m]]], c.z[m]) for m in range(c.M)]
    d = bc.D[c.kind]
    return (np.stack([p[0] for p in pairs]) if c.M else np.zeros((0, d))), (np.stack([p[1] for p in pairs]) if c.M else np.zeros((0, d, 30)))


def test_the_inputs_are_honest():
    """Every case of the full size holds factors with 0, 1, 2 and 17 measurements, every wavefront of four mixes them, the last factors
    have none; explicit indices with a repeated pair; the rotation cases reach qd.w < 0 before the flip and residual rotations of 1e-9,
    1, 3.1 rad and pi - 1e-6; positions of 5e6 m; float32-rounded quaternions."""
    assert bc.SIZES == (1, 3, 4, 5, 9) and bc.COUNTS == (17, 0, 1, 2, 2, 17, 1, 0, 0)
    for w in range(0, len(bc.COUNTS), 4):
        assert len(set(bc.COUNTS[w:w + 4])) >= min(3, len(bc.COUNTS[w:w + 4]))
    assert (bc.IDX_I[2], bc.IDX_J[2]) == (bc.IDX_I[5], bc.IDX_J[5]) and bc.COUNTS[2] and bc.COUNTS[5]
    for kind in range(3):
        names = [n for n, _ in bc.all_cases(kind)]
        assert "explicit" in names and "earth" in names and ("float32" in names) == bc.ROT[kind]
        c = bc.case(kind, 9)
        assert c.idx_i is None and c.S == 10 and set(c.counts.tolist()) == {0, 1, 2, 17} and c.M == sum(bc.COUNTS)
        x = bc.case(kind, 9, "explicit")
        assert x.idx_i is not None and x.S == 12 and max(x.idx_j) == 11
        assert np.abs(bc.case(kind, 9, "earth").states[:, 13:16]).max() >= 5e6
        if bc.ROT[kind]:
            n = np.linalg.norm(bc.case(kind, 9, "float32").states[:, :4], axis=1)
            assert (np.abs(n - 1) < 1e-7).all() and (n != 1.0).any()
            fi, fj = c.pairs()
            own = c.owner()
            w = []
            for m in range(c.M):
                xi, xj = c.states[fi[own[m]]], c.states[fj[own[m]]]
                rin = bc._unit_flip(*fx.quat_mul_ld(xj[:4], bc._inv(np.asarray(xi[:4], dtype=LD))))[0]
                w.append(float(fx.quat_mul_ld(c.z[m, :4], bc._inv(rin))[0][3]))
            w = np.array(w)
            ang = 2 * np.arccos(np.minimum(np.abs(w), 1.0))
            assert (w < 0).sum() >= 5 and (w > 0).sum() >= 5
            for a in (1.0, 3.1, np.pi - 1e-6):
                assert (np.abs(ang - a) < 1e-7).any(), a
            assert ang.max() > 3.14159 and (w[ang > 3.14159] < 0).any() and (w[ang > 3.14159] > 0).any()      # up to pi, on both sides of the flip
            assert (np.abs(ang - 1e-9) < 1e-6).any()


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_against_the_reference_and_the_documented_order(hb, kind):
    worst = {}
    for name, c in bc.all_cases(kind):
        e, J = twin_all_e_J(hb, c)
        if kind == 0:                                                         # no quaternion normalisation in it: e and J from the inputs, bit for bit
            fi, fj = c.pairs()
            own = c.owner()
            for m in range(c.M):
                e64, J64 = bc.position_e_J(c.states[fi[own[m]]], c.states[fj[own[m]]], c.z[m])
                assert same_bits(e[m], e64) and same_bits(np.ascontiguousarray(J[m]) + 0.0, J64 + 0.0), (name, m)
        for weight, base in ((True, True), (False, False)):
            hess, chi2, chi2_m = twin(hb, c, weight, base)
            d_hess, d_chi2, d_chi2_m = bc.documented(c, e, J, weight, base)
            assert same_bits(hess, d_hess) and same_bits(chi2, d_chi2) and same_bits(chi2_m, d_chi2_m), (name, weight, base)    # bit for bit
            for k, v in bc.metrics(hess, chi2, chi2_m, bc.reference(c, weight, base)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            none, c_only, m_only = twin(hb, c, weight, base, rows=False)      # the cost-only call
            assert none is None and same_bits(c_only, chi2) and same_bits(m_only, chi2_m)
            if base:                                                          # in place: the out-of-place call's bits
                i_hess, i_chi2, _ = twin(hb, c, weight, True, inplace=True)
                assert same_bits(i_hess, hess) and same_bits(i_chi2, chi2), name
    print("twin, %s: %s (gates %s)" % (bc.KINDS[kind], ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), bc.GATE_HOST))
    for k, v in worst.items():
        assert v <= bc.GATE_HOST[k], (k, v)


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_twin_exact_properties(hb, kind):
    c = bc.case(kind, 9)
    hess, chi2, chi2_m = twin(hb, c)
    none = c.counts == 0
    assert same_bits(hess[none], c.base[none]) and same_bits(chi2[none], c.chi2_base[none])
    rest = np.setdiff1d(np.arange(496), bc.touched(kind))                    # entries outside the touched set: the base bits
    assert len(bc.touched(kind)) == bc.NT[kind] and same_bits(np.ascontiguousarray(hess[:, rest]), np.ascontiguousarray(c.base[:, rest]))
    assert (hess[~none][:, bc.touched(kind)] != c.base[~none][:, bc.touched(kind)]).all()
    z_hess, z_chi2, _ = twin(hb, c, base=False)
    assert (z_hess[none] == 0.0).all() and (z_chi2[none] == 0.0).all() and (z_hess[:, rest] == 0.0).all()
    for F in (1, 3, 4, 5):                                                    # a factor's bits: its own data only
        o, p, x2 = twin(hb, bc.case(kind, F))
        assert same_bits(o, hess[:F]) and same_bits(p, chi2[:F]) and same_bits(x2, chi2_m[:len(x2)])
    x = bc.case(kind, 9, "explicit")                                          # a repeated pair: the same J, each factor its own measurements
    xh = twin(hb, x)[0]
    assert not np.array_equal(xh[2], xh[5])
    if bc.ROT[kind]:                                                          # z and -z: one rotation, equal as numbers
        z = c.z.copy()
        z[:, :4] = -z[:, :4]
        o, p, x2 = twin(hb, c, z=z)
        assert np.array_equal(o, hess) and np.array_equal(p, chi2) and np.array_equal(x2, chi2_m)
    bad = c.z.copy()                                                          # a NaN measurement: that factor alone
    m = int(c.mfirst[5]) + 3
    bad[m, 0] = np.nan
    o, p, x2 = twin(hb, c, z=bad)
    keep = np.arange(c.F) != 5
    assert same_bits(o[keep], hess[keep]) and same_bits(p[keep], chi2[keep]) and np.isnan(p[5]) and np.isnan(o[5]).any() and np.isnan(x2[m])
    assert same_bits(np.ascontiguousarray(o[5, rest]), np.ascontiguousarray(c.base[5, rest]))
    broken = np.array([-3, 40, 2, 1000, -1, 5, 0, 7, 100, -100], dtype=np.int64)   # clamped into [0, M]: nothing outside is touched
    twin(hb, c, mfirst=broken)


# ---------------------------------------------------------------- the Jacobian against central differences
def _fd_states(kind, n, seed=41):
    rng = np.random.default_rng(seed + kind)
    out = []
    for k in range(n):
        xi, xj = np.zeros(16), np.zeros(16)
        for x in (xi, xj):
            x[:4] = fx._unit_quat(rng)
            x[4:] = rng.standard_normal(12) * np.repeat([1e-2, 1.0, 1e-1, 5.0], 3)
        out.append((xi, xj))
    return out


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_jacobian_against_central_differences(hb, kind):
    """The table of the contract, in longdouble and as the twin computes it, against central differences of residual_ld through
    retract_ld.  The rotation blocks at e_th = 0 (z = q_j (x) inv(q_i) in longdouble), the position blocks anywhere (z_p off by 0.1 m
    and more)."""
    worst = {"table": 0.0, "twin": 0.0}
    rng = np.random.default_rng(43)
    for xi, xj in _fd_states(kind, 6):
        z = bc.exact_z(kind, xi, xj)
        if bc.POS[kind]:
            z[bc.ZN[kind] - 3:] = rng.standard_normal(3) * 3.0               # anywhere
        e, _, J, _ = bc.residual_ld(kind, xi, xj, z)
        if bc.ROT[kind]:
            assert np.abs(np.asarray(e[:3], dtype=np.float64)).max() < 1e-17
        fd = bc.fd_jacobian(kind, xi, xj, z)
        scale = 1 + np.abs(fd).max()
        worst["table"] = max(worst["table"], float(np.abs(fd - J).max() / scale))
        _, Jt = twin_e_J(hb, kind, xi, xj, np.asarray(z, dtype=np.float64))
        worst["twin"] = max(worst["twin"], float(np.abs(fd - np.asarray(Jt, dtype=LD)).max() / scale))
        for blk in (slice(3, 12), slice(18, 27)):                             # bg v ba of either state: structurally zero
            assert (Jt[:, blk] == 0).all() and (np.asarray(fd[:, blk], dtype=np.float64) == 0).all()
    print("%s: Jacobian against central differences (h %g): table %.3g, twin %.3g (gate %.3g)" % (bc.KINDS[kind], bc.FD_STEP, worst["table"], worst["twin"], bc.GATE_FD))
    assert worst["table"] <= bc.GATE_FD and worst["twin"] <= bc.GATE_FD


ROT_OFFSET = 1e-4   # rad: the residual rotation of the orientation kind's gradient check


@pytest.mark.parametrize("kind", range(3), ids=bc.KINDS)
def test_g_is_minus_the_gradient_of_the_cost(hb, kind):
    """g (column 30 of the row) = -d (0.5 w |R e|^2) / d delta along the retract, by central differences of the longdouble cost: the sign
    cpi_chain_solve_batch expects.  One measurement on a zero base; the pose at e_th = 0 (where its Jacobian is exact), position anywhere.
    The orientation kind alone has g = 0 at e_th = 0, so it is checked ROT_OFFSET = 1e-4 rad away from it: the flat right Jacobian then
    leaves out (1/2) [e x] + O(e^2) of the rotation blocks, a relative 5e-5 of J, which R^T R (condition number below 10 for the R of the
    cases) and the step from the 2-norm to the largest entry carry into g as less than 10 |e_th| = 1e-3; a wrong sign is 2."""
    rng = np.random.default_rng(47)
    worst = 0.0
    gate = bc.GATE_FD if bc.POS[kind] else 10 * ROT_OFFSET
    for xi, xj in _fd_states(kind, 3, seed=53):
        zl = bc.exact_z(kind, xi, xj)
        if bc.POS[kind]:
            zl[bc.ZN[kind] - 3:] = rng.standard_normal(3) * 3.0
        z = np.asarray(zl, dtype=np.float64)
        if not bc.POS[kind]:
            z = lc._quat_mul(lc._quat_of(rng.standard_normal(3), ROT_OFFSET), z)
        c = bc.Case.__new__(bc.Case)
        c.kind, c.F, c.S, c.M, c.counts, c.mfirst = kind, 1, 2, 1, np.array([1]), np.array([0, 1], dtype=np.int64)
        c.states, c.idx_i, c.idx_j, c.z = np.stack([xi, xj]), None, None, z[None]
        full = bc.case(kind, 1)
        c.R, c.weight, c.base, c.chi2_base = full.R[:1], full.weight[:1], np.zeros((1, 496)), np.zeros(1)
        hess, chi2, _ = twin(hb, c, base=False)
        g = hess[0, [bc.hslot(a, 30) for a in range(30)]]
        R, w, h = bc.unpack_R(c.R[0], bc.D[kind]), LD(c.weight[0]), LD(bc.FD_STEP)

        def cost(di, dj):
            e = bc.residual_ld(kind, bc.retract_ld(xi, di), bc.retract_ld(xj, dj), z)[0]
            wh = R @ e
            return LD(0.5) * w * (wh * wh).sum()

        grad = np.zeros(30, dtype=LD)
        for a in range(30):
            dl, zero = np.zeros(15, dtype=LD), np.zeros(15, dtype=LD)
            dl[a % 15] = h
            grad[a] = ((cost(dl, zero) - cost(-dl, zero)) if a < 15 else (cost(zero, dl) - cost(zero, -dl))) / (2 * h)
        assert np.abs(grad).max() > (1.0 if bc.POS[kind] else 0.01)          # a gradient to speak of
        worst = max(worst, float(np.abs(np.asarray(g, dtype=LD) + grad).max() / np.abs(grad).max()))
        assert abs(float(chi2[0] / (2 * cost(np.zeros(15, dtype=LD), np.zeros(15, dtype=LD)))) - 1) < (1e-12 if bc.POS[kind] else 8 * 2.0 ** -53 / ROT_OFFSET)
        # chi2 = w |R e|^2 on a zero base; a rotation component of 1e-4 carries the rounding of products of size 1 (four of them, twice in the square)
    print("%s: g + gradient, relative to the largest entry: %.3g (gate %.3g)" % (bc.KINDS[kind], worst, gate))
    assert worst <= gate


# ---------------------------------------------------------------- mutations
MUTATIONS = {
    "a dropped term (d e_p / d p_j)": ("((kind == 3) ? -p_i : 0.0));", "((kind == 3) ? 0.0 : 0.0));", "position"),
    "R_ij with i and j swapped": ("acc = fma(Rj.m[a][k], g.Ri.m[b][k], acc);", "acc = fma(g.Ri.m[a][k], Rj.m[b][k], acc);", "orientation"),
    "a transposed R_i": ("acc = fma(g.Ri.m[r][k], d[k], acc);", "acc = fma(g.Ri.m[k][r], d[k], acc);", "pose"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_wrong_term_fails_its_gate(hb, tmp_path, what):
    """The twin with one term wrong, built in tmp_path: the comparison with the reference leaves its gates by orders of magnitude, and
    the comparison with central differences shows O(1)."""
    old, new, name = MUTATIONS[what]
    mutant = _mutant(tmp_path, old, new)
    kind = bc.KINDS.index(name)
    c = bc.case(kind, 9)
    ref = bc.reference(c)
    res = {}
    for who, h in (("twin", hb), ("mutant", mutant)):
        try:
            res[who] = bc.metrics(*twin(h, c), ref)
        except AssertionError:                                                # an entry that no measurement touches was written
            res[who] = dict(G=np.inf, g=np.inf, f=np.inf, chi2=np.inf, chi2_m=np.inf)
        print("%s, %s: %s" % (what, who, ", ".join("%s %.3g" % kv for kv in sorted(res[who].items()))))
    assert all(res["twin"][k] <= bc.GATE_HOST[k] for k in res["twin"])
    assert max(res["mutant"]["G"], res["mutant"]["g"]) > 1e3 * max(bc.GATE_HOST.values()), res["mutant"]
    xi, xj = _fd_states(kind, 1)[0]
    z = bc.exact_z(kind, xi, xj)
    fd = bc.fd_jacobian(kind, xi, xj, z)
    off = float(np.abs(fd - np.asarray(twin_e_J(mutant, kind, xi, xj, np.asarray(z, dtype=np.float64))[1], dtype=LD)).max())
    print("%s: the mutant's Jacobian is %.3g from the central differences" % (what, off))
    assert off > 0.1


def test_the_stand_alone_twin_program(tmp_path):
    exe = str(tmp_path / "hostsim_between_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-ffp-contract=off", "-DHOSTSIM_BETWEEN_MAIN", "-o", exe, _SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout


# ---------------------------------------------------------------- the end-to-end problem
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "dense"])
def test_the_end_to_end_systems_are_positive_definite(ragged):
    """The undamped systems of the end-to-end cases at their starting states, with the prior and the betweens: a finite Cholesky and a
    bounded condition number for every chain (cc.Reference.check_inputs)."""
    pred, states, anchor, prior0 = fx.e2e_cpu()
    L = fx.layout(ragged)
    betweens = bc.e2e_betweens(pred, L)
    F = len(L["fi"])
    assert betweens[0]["mfirst"][-1] == F == len(betweens[0]["z"]) and betweens[1]["mfirst"][-1] == (F + 1) // 2 == len(betweens[1]["z"])
    loop = bc.BetweenLoop(anchor, prior0, betweens, L)
    sol = loop.system(states)
    sol.check_inputs()
    print("condition numbers with the betweens: %s" % np.array2string(sol.cond, precision=3))
    assert (np.abs(np.asarray(loop.brows, dtype=np.float64)[:, 495]) > 0).all()
