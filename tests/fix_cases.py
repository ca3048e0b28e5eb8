"""Inputs, references and metrics of cpi_state_fix_batch (tests/test_fix_cpu.py on the host twin, tests/test_gpu_fix.py on the device).
TEST INFRASTRUCTURE ONLY.  Built on tests/lm_cases.py (fma, CpuLoop) and tests/chain_cases.py (the packing).

Three kinds of statement:
  * the FIXED summation order of include/cpi_amd.h restated in float64 numpy (documented), from the residual e: bit for bit;
  * the same quantities in numpy.longdouble by the table of the contract (reference): within a gate;
  * a CPU loop with fixes, FixLoop over lm_cases.CpuLoop, for the end-to-end case.

Metrics, in the natural unit of each quantity (printed by the tests before anything is asserted).  The unit of an entry is 2^-53 times
the sum of the absolute values of its terms, the terms followed down to the inputs: |e|_b below is |e_b| plus, for a rotation
component, 2 x the four absolute products of the quaternion product behind it (the rounding of a component of size 1e-9 is that of
products of size 1, not of 1e-9):
    Lam    |Lam_ab - ref| / ((|base_ab| + sum_m w (|R|^T |R|)_ab) 2^-53)
    eta    |eta_a - ref|  / ((|base_a| + sum_m w (|R|^T |R| |e|)_a) 2^-53)
    pcost  |pcost - ref|  / ((|pcost_base| + sum_m 0.5 w ||R| |e||^2) 2^-53)
    chi2   |chi2_m - ref| / (||R| |e||^2 2^-53)
    final  max |local(final state, the CPU loop's)_i| / sigma_i, sigma from chain_marginals at the final states
Gates = 100 x the floor, the rule of tests/tol.py and tests/lm_cases.py; a floor is the largest value measured over every case of the
tests and never below one unit.  Measured (profiles/state_fix.md):
    host twin (tests/hostsim/hostsim_fix.cpp, x86-64)    Lam 7.0   eta 6.3   pcost 4.3   chi2 4.7
    device (MI355X)                                      Lam 7.0   eta 6.3   pcost 4.3   chi2 4.7   final 4.3e-13 sigma (dense; ragged 1.8e-13)
All four are set by the 1027 states of edge_case("many", .) -- the largest of 4560 fixes, where the nine states of case() gave 3.5, 3.0,
1.7, 3.3 on the host and 4.5, 3.0, 2.4, 3.3 on the device; the builders at GPS-sized positions and with float32-rounded, scaled or
axis-aligned quaternions stay below those.  A wrong term shows as 1e13 units and more (the mutation checks of tests/test_fix_cpu.py)."""
import functools

import numpy as np

from tests import chain_cases as cc
from tests import lm_cases as lc

LD = np.longdouble
EPS_HALF = cc.EPS_HALF
SENTINEL = lc.SENTINEL
KINDS = ("position", "velocity", "orientation", "pose")
D = (3, 3, 3, 6)
ZN = (3, 3, 4, 7)
RN = (6, 6, 6, 21)
SEL = ((12, 13, 14), (6, 7, 8), (0, 1, 2), (0, 1, 2, 12, 13, 14))

FLOOR_HOST = dict(Lam=7.0, eta=6.3, pcost=4.3, chi2=4.7)
FLOOR_DEVICE = dict(Lam=7.0, eta=6.3, pcost=4.3, chi2=4.7)
FLOOR_FINAL_DEVICE = 4.3e-13  # sigma: both loops reach the minimum itself, what is left is rounding (as lm_cases.FLOOR_FINAL_DEVICE)
GATE_HOST = {k: 100 * max(v, 1.0) for k, v in FLOOR_HOST.items()}
GATE_DEVICE = {k: 100 * max(v, 1.0) for k, v in FLOOR_DEVICE.items()}
GATE_FINAL_DEVICE = 100 * FLOOR_FINAL_DEVICE

# fixes per state: 0, 1, 2 and 17 dealt so that every wavefront of four states mixes them; the last two states have none
COUNTS = (17, 0, 1, 2, 2, 17, 1, 0, 0)
SIZES = (1, 3, 4, 5, 9)


def tri(d):
    return d * (d + 1) // 2


def slot(a, b):
    """Where entry (a, b) of the 16 x 16 symmetric row sits in its 136 doubles."""
    return tri(max(a, b)) + min(a, b)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def unpack_R(Rp, d, dtype=LD):
    R = np.zeros(Rp.shape[:-1] + (d, d), dtype=dtype)
    for k in range(d):
        for i in range(k + 1):
            R[..., i, k] = Rp[..., tri(k) + i]
    return R


def _unit_quat(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def quat_mul_ld(q, p):
    """quat_multiply of cpi_math.hpp in longdouble WITHOUT the normalisation and the sign: (product [4], |terms| [4])."""
    q, p = np.asarray(q, dtype=LD), np.asarray(p, dtype=LD)
    qv, pv = q[:3], p[:3]
    r = np.concatenate([q[3] * pv - np.cross(qv, pv) + qv * p[3], [q[3] * p[3] - qv @ pv]])
    aq, ap = np.abs(q), np.abs(p)
    cr = np.array([aq[1] * ap[2] + aq[2] * ap[1], aq[2] * ap[0] + aq[0] * ap[2], aq[0] * ap[1] + aq[1] * ap[0]], dtype=LD)
    t = np.concatenate([aq[3] * ap[:3] + cr + aq[:3] * ap[3], [aq[3] * ap[3] + aq[:3] @ ap[:3]]])
    return r, t


def residual_ld(kind, x, z):
    """(e [d], |e| [d]) of one fix by the table of the contract, in longdouble; |e| as the module docstring defines it."""
    x, z = np.asarray(x, dtype=LD), np.asarray(z, dtype=LD)
    if kind == 0:
        e = z - x[13:16]
        return e, np.abs(e)
    if kind == 1:
        e = z - x[7:10]
        return e, np.abs(e)
    qinv = np.concatenate([-x[:3], x[3:4]])
    r, t = quat_mul_ld(z[:4], qinv)
    n = np.sqrt((r * r).sum())
    r, t = r / n, t / n
    if r[3] < 0:
        r = -r
    e, u = 2 * r[:3], 2 * t[:3] + np.abs(2 * r[:3])
    if kind == 3:
        ep = z[4:7] - x[13:16]
        e, u = np.concatenate([e, ep]), np.concatenate([u, np.abs(ep)])
    return e, u


class Case:
    """One call: states [S, 16], mfirst [S + 1], z [M, ZN], R [M, RN], weight [M], base [S, 136], pcost_base [S]."""

    def __init__(self, kind, counts, seed=3, angle=None):
        rng = np.random.default_rng(seed + 17 * kind)
        self.kind, self.counts = kind, np.asarray(counts, dtype=np.int64)
        S, d = len(counts), D[kind]
        self.S, self.mfirst = S, offsets(counts)
        M = self.M = int(self.mfirst[-1])
        self.states = np.zeros((S, 16))
        for s in range(S):
            self.states[s, :4] = _unit_quat(rng)
            self.states[s, 4:] = rng.standard_normal(12) * np.repeat([1e-2, 1.0, 1e-1, 5.0], 3)
        self.z = np.zeros((M, ZN[kind]))
        owner = np.repeat(np.arange(S), self.counts)
        for m in range(M):
            x = self.states[owner[m]]
            if kind == 0:
                self.z[m] = x[13:16] + 0.1 * rng.standard_normal(3)
            elif kind == 1:
                self.z[m] = x[7:10] + 0.05 * rng.standard_normal(3)
            else:
                a = angle if angle is not None else (1e-9, 0.03, 1.0, 3.1)[m % 4]
                self.z[m, :4] = lc._quat_mul(lc._quat_of(rng.standard_normal(3), a), x[:4])
                if m % 3 == 1:
                    self.z[m, :4] = -self.z[m, :4]                             # the same attitude: qd.w < 0 before the flip
                if kind == 3:
                    self.z[m, 4:7] = x[13:16] + 0.1 * rng.standard_normal(3)
        scale = {0: 10.0, 1: 20.0, 2: 50.0, 3: np.array([50.0] * 3 + [10.0] * 3)}[kind]
        Rd = np.triu(np.eye(d) + 0.3 * rng.standard_normal((M, d, d))) * np.asarray(scale)[..., None] if M else np.zeros((0, d, d))
        self.R = np.zeros((M, RN[kind]))
        for k in range(d):
            for i in range(k + 1):
                self.R[:, tri(k) + i] = Rd[:, i, k]
        self.weight = rng.uniform(0.25, 2.0, M)
        B = np.zeros((S, 16, 16))
        for s in range(S):
            A = cc.SCALES[:, None] * np.triu(np.eye(15) + 0.1 * rng.standard_normal((15, 15)))
            B[s, :15, :15] = A.T @ A
            B[s, :15, 15] = B[s, 15, :15] = np.diag(B[s])[:15] * 0.01 * rng.standard_normal(15)
        self.base = cc.pack_upper(B)
        self.pcost_base = rng.standard_normal(S) * 3.0

    def owner(self):
        return np.repeat(np.arange(self.S), self.counts)


    def head(self, S):
        """The first S states with their fixes: the same data at another S."""
        c = Case.__new__(Case)
        M = int(self.mfirst[S])
        c.kind, c.counts, c.S, c.M, c.mfirst = self.kind, self.counts[:S], S, M, self.mfirst[:S + 1].copy()
        c.states, c.base, c.pcost_base = (np.ascontiguousarray(a[:S]) for a in (self.states, self.base, self.pcost_base))
        c.z, c.R, c.weight = (np.ascontiguousarray(a[:M]) for a in (self.z, self.R, self.weight))
        return c


@functools.lru_cache(maxsize=None)
def case(kind, S, seed=3):
    """The first S states of the nine of COUNTS: a state's data does not depend on S."""
    full = Case(kind, COUNTS, seed) if S == len(COUNTS) else case(kind, len(COUNTS), seed)
    return full if S == len(COUNTS) else full.head(S)


# --------------------------------------------------------------------------------------------- the cases at the edges of the contract
# Variations of the nine-state Case(kind, COUNTS): the mix of 0 / 1 / 2 / 17 fixes per wavefront stays (tests/test_fix_cpu.py holds the
# host twin to the reference on each of them, tests/test_gpu_fix_edges.py the device).
EARTH = np.array([4.2e6, 1.7e5, 4.8e6])      # an ECEF position: a GPS fix is 6e6 m from the origin
MANY, MANY_SEED = 1027, 101                  # 257 workgroups of four states, the last one short
Z_SCALES, X_SCALES = (0.5, 2.0, 1e-3, 1e3, 1.0 + 1e-7), (1.0, 3.0, 0.25)
EDGE_BUILDERS = (("earth", (0, 3)), ("float32", (2, 3)), ("scaled", (2, 3)), ("identity", (2, 3)), ("many", (0, 1, 2, 3)))


def _zp(kind):
    """The columns of z that hold a position."""
    return slice(0, 3) if kind == 0 else slice(4, 7)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def edge_case(name, kind):
    """One of EDGE_BUILDERS:
      earth     kinds 0, 3: EARTH added to the states' positions and to the position part of z (z - p stays exact in double)
      float32   kinds 2, 3: the state and z quaternions rounded to float32 and back: unit to 1e-8 only
      scaled    kinds 2, 3: z scaled by Z_SCALES[m % 5], the state quaternion by X_SCALES[s % 3] (residual_ld normalises the product)
      identity  kinds 2, 3: the state quaternions np.eye(4)[(s + 3) % 4], z the owner's quaternion, negated for odd m: the product has
                no rounding and the rotation residual is exactly +-0.0
      many      every kind: MANY states (COUNTS tiled), a problem of its own seed"""
    assert kind in dict(EDGE_BUILDERS)[name], (name, kind)
    if name == "many":
        c = Case(kind, np.tile(COUNTS, 115)[:MANY], seed=MANY_SEED)
        nine = case(kind, len(COUNTS))
        for a, b in ((c.states[:9], nine.states), (c.z[:int(c.mfirst[9])], nine.z), (c.R[:int(c.mfirst[9])], nine.R)):
            assert not np.isin(a, b).any(), "the first nine states repeat the nine-state case"
        return c
    c = Case(kind, COUNTS)
    own = c.owner()
    if name == "earth":
        c.states[:, 13:16] += EARTH
        c.z[:, _zp(kind)] += EARTH
        assert np.abs(c.states[:, 13:16]).max() > 4e6
    elif name == "float32":
        c.states[:, :4], c.z[:, :4] = _f32(c.states[:, :4]), _f32(c.z[:, :4])
        n = np.linalg.norm(c.states[:, :4], axis=1)
        assert (np.abs(n - 1) < 1e-7).all() and (n != 1.0).any()
    elif name == "scaled":
        c.z[:, :4] *= np.asarray(Z_SCALES)[np.arange(c.M) % 5][:, None]
        c.states[:, :4] *= np.asarray(X_SCALES)[np.arange(c.S) % 3][:, None]
    elif name == "identity":
        c.states[:, :4] = np.eye(4)[(np.arange(c.S) + 3) % 4]
        c.z[:, :4] = c.states[own, :4] * np.where(np.arange(c.M) % 2, -1.0, 1.0)[:, None]
    return c


def reversed_case(c):
    """(the case with its states in reverse order, order [S], fixes [M]: where every state and fix of it sits in c)."""
    order = np.arange(c.S - 1, -1, -1)
    fixes = np.concatenate([np.arange(c.mfirst[s], c.mfirst[s + 1]) for s in order]).astype(np.int64)
    mv = c.head(c.S)
    mv.counts = c.counts[order]
    mv.mfirst = offsets(mv.counts)
    mv.states, mv.base, mv.pcost_base = c.states[order], c.base[order], c.pcost_base[order]
    mv.z, mv.R, mv.weight = c.z[fixes], c.R[fixes], c.weight[fixes]
    return mv, order, fixes


def touched(kind):
    """The entries of a row [136] that a kind writes: (Lam slots, eta slots)."""
    d, sel = D[kind], SEL[kind]
    return [slot(sel[a], sel[b]) for a in range(d) for b in range(a, d)], [slot(sel[a], 15) for a in range(d)]


def reference(c, weight=True, base=True):
    """By the table of the contract in longdouble -> dict(out [S, 136], pcost [S], chi2 [M]) and the units u_out, u_pcost, u_chi2
    (without the 2^-53).  Entries of out that no fix touches are the base's (or 0) with unit 0: they must be exact."""
    kind, d, sel = c.kind, D[c.kind], SEL[c.kind]
    out = np.array(c.base if base else np.zeros((c.S, 136)), dtype=LD)
    out[:, 135] = 0
    u_out = np.zeros((c.S, 136), dtype=LD)
    pcost = np.array(c.pcost_base if base else np.zeros(c.S), dtype=LD)
    u_pc = np.abs(pcost)
    chi2, u_chi2 = np.zeros(c.M, dtype=LD), np.zeros(c.M, dtype=LD)
    R = unpack_R(c.R, d)
    touched = [slot(sel[a], sel[b]) for a in range(d) for b in range(a, d)] + [slot(sel[a], 15) for a in range(d)]
    for s in range(c.S):
        if c.counts[s]:
            u_out[s, touched] = np.abs(out[s, touched])
        for m in range(c.mfirst[s], c.mfirst[s + 1]):
            w = LD(c.weight[m]) if weight else LD(1)
            e, ue = residual_ld(kind, c.states[s], c.z[m])
            wh, uwh = R[m] @ e, np.abs(R[m]) @ ue
            chi2[m], u_chi2[m] = (wh * wh).sum(), (uwh * uwh).sum()
            G, uG = R[m].T @ R[m], np.abs(R[m]).T @ np.abs(R[m])
            u, uu = R[m].T @ wh, np.abs(R[m]).T @ uwh
            for a in range(d):
                for b in range(a, d):
                    out[s, slot(sel[a], sel[b])] += w * G[a, b]
                    u_out[s, slot(sel[a], sel[b])] += abs(w) * uG[a, b]
                out[s, slot(sel[a], 15)] += w * u[a]
                u_out[s, slot(sel[a], 15)] += abs(w) * uu[a]
            pcost[s] += LD(0.5) * w * chi2[m]
            u_pc[s] += LD(0.5) * abs(w) * u_chi2[m]
    return dict(out=out, pcost=pcost, chi2=chi2, u_out=u_out, u_pcost=u_pc, u_chi2=u_chi2)


def metrics(out, pcost, chi2, ref):
    """dict(Lam, eta, pcost, chi2) in units; entries with unit 0 must be exact (asserted here: they are copies)."""
    tiny = np.finfo(np.float64).tiny
    m = {}
    if out is not None:
        err = np.abs(np.asarray(out, dtype=LD) - ref["out"])
        exact = ref["u_out"] == 0
        assert (err[exact] == 0).all(), "an entry that no fix touches differs from the base"
        r = np.where(exact, 0, err / np.maximum(ref["u_out"] * EPS_HALF, tiny))
        m["Lam"], m["eta"] = float(r[:, :120].max(initial=0)), float(r[:, 120:135].max(initial=0))
    if pcost is not None:
        err = np.abs(np.asarray(pcost, dtype=LD) - ref["pcost"])
        m["pcost"] = float(np.where(ref["u_pcost"] == 0, err, err / np.maximum(ref["u_pcost"] * EPS_HALF, tiny)).max(initial=0))
    if chi2 is not None and len(chi2):
        m["chi2"] = float((np.abs(np.asarray(chi2, dtype=LD) - ref["chi2"]) / np.maximum(ref["u_chi2"] * EPS_HALF, tiny)).max())
    return m


def documented(c, e, weight=True, base=True):
    """The summation orders of include/cpi_amd.h in float64, from the residuals e [M, d] -> (out [S, 136], pcost [S], chi2 [M])."""
    fma = lc.fma
    kind, d, sel = c.kind, D[c.kind], SEL[c.kind]
    out = np.array(c.base if base else np.zeros((c.S, 136)), dtype=np.float64)
    out[:, 135] = 0.0
    pcost = np.array(c.pcost_base if base else np.zeros(c.S), dtype=np.float64)
    chi2 = np.zeros(c.M)
    Rat = lambda m, i, k: float(c.R[m, tri(k) + i])
    for s in range(c.S):
        for m in range(c.mfirst[s], c.mfirst[s + 1]):
            w = float(c.weight[m]) if weight else 1.0
            wh = []
            for i in range(d):
                acc = 0.0
                for k in range(i, d):
                    acc = fma(Rat(m, i, k), e[m, k], acc)
                wh.append(acc)
            x2 = np.float64(wh[0]) * np.float64(wh[0])
            for i in range(1, d):
                x2 = x2 + np.float64(wh[i]) * np.float64(wh[i])
            chi2[m] = x2
            pcost[s] = fma(0.5 * w, float(x2), pcost[s])
            for a in range(d):
                acc = 0.0
                for i in range(a + 1):
                    acc = fma(Rat(m, i, a), wh[i], acc)
                out[s, slot(sel[a], 15)] = fma(w, acc, out[s, slot(sel[a], 15)])
                for b in range(a, d):
                    acc = 0.0
                    for i in range(a + 1):
                        acc = fma(Rat(m, i, a), Rat(m, i, b), acc)
                    out[s, slot(sel[a], sel[b])] = fma(w, acc, out[s, slot(sel[a], sel[b])])
    return out, pcost, chi2


def gaussian_record(c, m):
    """The old route for fix m of case c: (anchor [16], prior0 [136]) with Lam = S^T R^T R S, eta0 = 0 and the anchor equal to the fix's
    state with z put in -- what cpi_prior_relinearize_batch takes."""
    kind, d, sel = c.kind, D[c.kind], SEL[c.kind]
    s = int(np.searchsorted(c.mfirst, m, side="right") - 1)
    anchor = c.states[s].copy()
    if kind == 0:
        anchor[13:16] = c.z[m]
    elif kind == 1:
        anchor[7:10] = c.z[m]
    else:
        anchor[:4] = c.z[m, :4]
        if kind == 3:
            anchor[13:16] = c.z[m, 4:7]
    R = unpack_R(c.R[m], d, np.float64)
    P = np.zeros((16, 16))
    P[np.ix_(sel, sel)] = R.T @ R
    return s, anchor, cc.pack_upper(P[None])[0]


# --------------------------------------------------------------------------------------------- the end-to-end cases on the CPU
# states per chain of the RAGGED end-to-end case: eight chains with G between 2 and 6.  Chain c keeps the first n_c states of its block
# of six in tests/chain_pipeline.py, so first = 6 c is explicit, the other states of a block belong to no chain, and the factor rows
# are compacted (ffirst = the running sum of n_c - 1): first / count / ffirst all differ from chain to chain.
RAGGED_COUNTS = (2, 3, 4, 5, 6, 6, 3, 2)


def layout(ragged):
    """dict(count [C] int32, first [C] int64, ffirst [C] int64, keep: the rows of the pipeline's 40 factors the chains use, in chain
    order, fi / fj: the states each of them joins, member [S] bool) of the ragged or of the dense (eight times six) end-to-end case."""
    from tests import chain_pipeline as cp
    n = np.array(RAGGED_COUNTS if ragged else [cp.G] * cp.C, dtype=np.int64)
    first = np.arange(cp.C, dtype=np.int64) * cp.G
    keep = np.concatenate([c * (cp.G - 1) + np.arange(n[c] - 1) for c in range(cp.C)])
    fi = np.concatenate([first[c] + np.arange(n[c] - 1) for c in range(cp.C)])
    member = np.zeros(cp.S, dtype=bool)
    for c in range(cp.C):
        member[first[c]:first[c] + n[c]] = True
    return dict(count=n.astype(np.int32), first=first, ffirst=offsets(n - 1)[:-1], keep=keep, fi=fi, fj=fi + 1, member=member)


def e2e_fixes(pred, member=None, seed=23):
    """The fixes of an end-to-end case from the UNPERTURBED states pred [S, 16] of tests/chain_pipeline.py: a position fix on every
    state of a chain (sigma 0.05 m), a pose fix on the first and -- where the chain has one -- the fourth state of every chain
    (0.01 rad, 0.02 m), so the first state carries its Gaussian prior, a position and a pose fix; every z is moved by a seeded draw of
    its noise.  member [S] bool: the states that belong to a chain (None: all); the others get no fix, so mfirst, which indexes STATES,
    is no arange.  A list of dicts of numpy arrays as Engine.chain_lm takes tensors: kind, z, R, mfirst."""
    from tests import chain_pipeline as cp
    rng = np.random.default_rng(seed)
    S = cp.S
    member = np.ones(S, dtype=bool) if member is None else member
    zp = pred[:, 13:16] + 0.05 * rng.standard_normal((S, 3))
    pos = dict(kind="position", z=np.ascontiguousarray(zp[member]), R=np.tile(np.array([20.0, 0, 20.0, 0, 0, 20.0]), (int(member.sum()), 1)),
               mfirst=offsets(member.astype(np.int64)))
    has = ((np.arange(S) % cp.G == 0) | (np.arange(S) % cp.G == 3)) & member
    rows = np.flatnonzero(has)
    z = np.zeros((len(rows), 7))
    for k, s in enumerate(rows):
        z[k, :4] = lc._quat_mul(lc._quat_of(rng.standard_normal(3), 0.01 * abs(rng.standard_normal()) + 1e-4), pred[s, :4])
        z[k, 4:] = pred[s, 13:16] + 0.02 * rng.standard_normal(3)
    Rp = np.zeros((len(rows), 21))
    for a in range(6):
        Rp[:, tri(a) + a] = 100.0 if a < 3 else 50.0
    Rp[:, tri(4) + 1] = 5.0                                                  # an off-diagonal entry: rotation against position
    pose = dict(kind="pose", z=z, R=Rp, mfirst=offsets(has.astype(np.int64)))
    return [pos, pose]


def fix_rows_ld(fixes, st):
    """(rows [S, 136], pcost [S]) of the fixes at the states st, in longdouble, on a zero base."""
    rows, pc = np.zeros((len(st), 136), dtype=LD), np.zeros(len(st), dtype=LD)
    for f in fixes:
        c = Case.__new__(Case)
        c.kind = KINDS.index(f["kind"])
        c.S, c.mfirst, c.counts = len(st), f["mfirst"], np.diff(f["mfirst"])
        c.M, c.states, c.z, c.R = len(f["z"]), st, f["z"], f["R"]
        c.weight = f.get("weight", np.ones(c.M))
        c.base, c.pcost_base = np.zeros((c.S, 136)), np.zeros(c.S)
        r = reference(c)
        rows, pc = rows + r["out"], pc + r["pcost"]
    return rows, pc


class FixLoop(lc.CpuLoop):
    """lm_cases.CpuLoop (its longdouble pieces: the oracle's preintegration, R, retract / local) with absolute measurements and over
    the chains of a layout(), ragged or dense: the fixes' cost joins every chain's cost, their rows join the prior rows of the solve.
    anchor / prior0 [C, ...]: one Gaussian record per chain, on its first state.  States of no chain are never moved."""

    def __init__(self, anchor, prior0, fixes, lay=None):
        super().__init__(anchor, prior0)
        self.fixes, self.lay = fixes, lay if lay is not None else layout(False)

    def costs(self, st):
        L, cp = self.lay, self.cp
        ref = self.fc.evaluate_error_longdouble(1, self.rec[L["keep"]], st[L["fi"]], st[L["fj"]])
        w = self.fc.whitened_longdouble(ref, self.R[L["keep"]])[0]
        chi2 = (w * w).sum(1)
        eta, pcost, _, _ = lc.prior_reference(lc.oracle_local(st[L["first"]], self.anchor), self.prior0)
        self.rows, pc = fix_rows_ld(self.fixes, st)                           # of the states costs() was last called with
        cost = [LD(0.5) * chi2[ff:ff + n - 1].sum() + pcost[c] + pc[f:f + n].sum() for c, (f, n, ff) in enumerate(zip(L["first"], L["count"], L["ffirst"]))]
        return ref, eta, np.asarray(cost, dtype=np.float64)

    def prior_rows(self, eta):
        prior = np.zeros((self.cp.S, 136))
        prior[self.lay["first"]] = self.prior0
        prior[self.lay["first"], 120:135] = np.asarray(eta, dtype=np.float64)
        prior = np.asarray(np.asarray(prior, dtype=LD) + self.rows, dtype=np.float64)
        prior[:, 135] = 0.0
        return prior

    def batch(self, ref, prior):
        L = self.lay
        hess = np.asarray(self.fc.hessian_longdouble(ref, self.R[L["keep"]]), dtype=np.float64)
        return cc.Batch.from_arrays(L["count"], L["first"], L["ffirst"], hess, prior)

    def system(self, st):
        """The undamped systems at st as a cc.Reference (its check_inputs: a finite Cholesky of every chain's matrix)."""
        ref, eta, _ = self.costs(st)
        return cc.Reference(self.batch(ref, self.prior_rows(eta)))

    def run(self, states, lam, iterations, params=None):
        L, C = self.lay, self.cp.C
        p = dict(lc.DEFAULTS, **(params or {}))
        st, lam = np.array(states, dtype=np.float64), np.full(C, lam, dtype=np.float64)
        phase = np.zeros(C, dtype=np.int32)
        ref, eta, cost = self.costs(st)
        prior = self.prior_rows(eta)
        history = [cost.copy()]
        for _ in range(iterations):
            delta = cc.Reference(self.batch(ref, prior), lam, True).delta    # NaN in the rows of no chain
            trial = st.copy()
            for s in np.flatnonzero(L["member"]):
                trial[s] = self.orc.retract(st[s], delta[s])
            _, _, new = self.costs(trial)
            for c in range(C):
                if phase[c] != 0:
                    continue
                acc, cost[c], lam[c], ph = lc.lm_rule(cost[c], new[c], lam[c], p)
                if ph:
                    phase[c] = ph
                if acc:
                    rows = slice(L["first"][c], L["first"][c] + L["count"][c])
                    st[rows] = trial[rows]
            ref, eta, _ = self.costs(st)
            prior = self.prior_rows(eta)
            history.append(cost.copy())
        return st, cost, lam, phase, np.stack(history)


@functools.lru_cache(maxsize=None)
def e2e_cpu():
    """(pred [S, 16], states [S, 16], anchor [C, 16], prior0 [C, 136]) of tests/chain_pipeline.py on the CPU, as its cpu_case() forms them:
    a Gaussian prior 0.1 diag(scales)^2 on every chain's first state, centred on the unperturbed state."""
    from oracle import oracle_py as op
    from tests import chain_pipeline as cp
    from tests import factor_cases as fc
    x = cp.inputs()
    kn, lin = x["knots"].numpy(), x["lin"].numpy()
    orc = op.oracle()
    rec = op.factor_records(orc.run(op.make_params(1, 0, 1), kn, lin, x["q"].numpy()), lin, None)
    pred = np.zeros((cp.S, 16))
    pred[0::cp.G] = x["x0"].numpy()
    for k in range(cp.G - 1):
        rows = np.arange(cp.C) * (cp.G - 1) + k
        pred[k + 1::cp.G] = np.asarray(fc.predict_longdouble(1, rec[rows], pred[k::cp.G]), dtype=np.float64)
    states = np.stack([orc.retract(pred[s], x["step"].numpy()[s]) for s in range(cp.S)])
    P0 = np.zeros((cp.C, 16, 16))
    P0[:, np.arange(15), np.arange(15)] = 0.1 * cc.SCALES ** 2
    return pred, states, pred[0::cp.G].copy(), cc.pack_upper(P0)
