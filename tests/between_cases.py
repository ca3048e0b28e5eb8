"""Inputs, references and metrics of cpi_state_between_batch (tests/test_between_cpu.py on the host twin, tests/test_gpu_between.py on the
device).  TEST INFRASTRUCTURE ONLY.  Built on tests/fix_cases.py (the packing of R, the quaternion product with its units, FixLoop),
tests/lm_cases.py (fma) and tests/chain_cases.py.

Five kinds of statement:
  * the FIXED summation order of include/cpi_amd.h restated in float64 numpy (documented), from the residual e and the Jacobian J of
    every measurement: bit for bit;
  * the position kind's e and J restated in float64 numpy from the inputs (position_e_J): bit for bit on the host twin -- no quaternion
    normalisation separates the two (quat_2_Rot is products and sums; the twin is compiled without contraction).  The orientation and
    pose kinds go through quat_multiply, whose normalisation the restatement does not fix, so their e and J come from the twin;
  * the same quantities in numpy.longdouble by the table of the contract (reference): within a gate;
  * central differences of the longdouble residual through a longdouble retract (fd_jacobian), which decide the signs of the table;
  * a CPU loop with between measurements, BetweenLoop over fix_cases.FixLoop (a lm_cases.CpuLoop), for the end-to-end case.

Metrics, in the natural unit of each quantity (printed by the tests before anything is asserted): 2^-53 times the sum of the absolute
values of the terms of an entry, the terms followed down to the inputs (the metric of tests/fix_cases.py extended to the 31 x 31 row):
    G      |hess_ab - ref| / ((|base_ab| + sum_m w (|A|^T |A|)_ab) 2^-53), a <= b < 30, |A| = |R| |J|
    g      the same for column 30, rows < 30, with |b| = |R| |e|
    f      the same for entry (30, 30)
    chi2   |chi2_f - ref| / ((|chi2_base| + sum_m w ||R| |e||^2) 2^-53);    chi2_m  |chi2_m - ref| / (||R| |e||^2 2^-53)
    final  max |local(final state, the CPU loop's)_i| / sigma_i, sigma from chain_marginals at the final states
Gates = 100 x the floor, the rule of tests/tol.py and tests/fix_cases.py; a floor is the largest value measured over every case of the
tests and never below one unit.  Measured (profiles/state_between.md):
    host twin (tests/hostsim/hostsim_between.cpp, x86-64)   G 5.9   g 0.46   f 0.11   chi2 0.098   chi2_m 0.25
    device (MI355X)                                         G 5.9   g 0.60   f 0.11   chi2 0.12    chi2_m 0.22
                                                            final 2.1e-13 sigma (dense; ragged 2.0e-13): FLOOR_FINAL_DEVICE
G is set by the pose kind on the chained nine factors (position 3.9, orientation 4.5); every other figure stays below one unit, so its
gate is the 100 units of the rule.  A wrong term shows as 1e13 units and more (the mutation checks of tests/test_between_cpu.py).
Central differences: step FD_STEP = 1e-6 on every tangent entry, in longdouble.  The truncation of a central difference is h^2 / 6 times
the third derivative (1e-12 x the size of the entry for a rotation, 0 for the linear position entries), the rounding 2^-64 / h x the
size of the residual's terms (5e-14 x).  Measured over every case, relative to 1 + the largest entry: the Jacobian 2.5e-13 (position),
6.1e-14 (orientation), 2.4e-13 (pose); g against the gradient of the cost 6.7e-13 (position), 1.0e-12 (pose): FLOOR_FD is the largest.
A wrong sign or a transposed block shows as O(1) (0.9 to 16 in the mutation checks).
The edge builders (edge_case; tests/between_edge_checks.py) have floors of their own, FLOOR_EDGE_HOST / FLOOR_EDGE_DEVICE, the largest
value over the kinds of a builder against the same longdouble reference, and gates by the same rule, 100 x max(floor, 1).  Measured on
the host twin (x86-64) / on the MI355X:
    identity   G 4.41 / 4.41   g, f, chi2, chi2_m 0 / 0: every residual is exactly zero
    pi         G 4.62 / 4.62   g 0.393 / 0.393   f 0.147 / 0.147   chi2 0.181 / 0.181   chi2_m 0.147 / 0.147   (exact products: the same bits)
    scaled     G 4.96 / 4.96   g 0.337 / 0.67    f 0.108 / 0.129   chi2 0.072 / 0.144   chi2_m 0.102 / 0.582
    long       G 10.9 / 10.8   g 0.176 / 0.16    f 0.0847 / 0.0847 chi2 0.0847 / 0.0847 chi2_m 0.381 / 0.381
Only the fold of 300 (long) leaves the range of FLOOR_HOST / FLOOR_DEVICE by more than a fraction of a unit: G 10.9 against 5.9, the
rounding of 300 fma steps onto one entry; its G gate is 1090 (host) / 1080 (device), every other gate of the builders is the 100 units of
the rule or, for G, below GATE_HOST's 590."""
import functools

import numpy as np

from tests import chain_cases as cc
from tests import fix_cases as fx
from tests import lm_cases as lc

LD = np.longdouble
EPS_HALF = cc.EPS_HALF
SENTINEL = lc.SENTINEL
KINDS = ("position", "orientation", "pose")
D = (3, 3, 6)
ZN = (3, 4, 7)
RN = (6, 6, 21)
COLS = ((0, 1, 2, 12, 13, 14, 27, 28, 29, 30), (0, 1, 2, 15, 16, 17, 30), (0, 1, 2, 12, 13, 14, 15, 16, 17, 27, 28, 29, 30))
NT = (55, 28, 91)
ROT = (False, True, True)
POS = (True, False, True)

FLOOR_HOST = dict(G=5.9, g=0.46, f=0.11, chi2=0.098, chi2_m=0.25)
FLOOR_DEVICE = dict(G=5.9, g=0.60, f=0.11, chi2=0.12, chi2_m=0.22)
GATE_HOST = {k: 100 * max(v, 1.0) for k, v in FLOOR_HOST.items()}
GATE_DEVICE = {k: 100 * max(v, 1.0) for k, v in FLOOR_DEVICE.items()}
# the edge builders (edge_case), each with a floor of its own: the largest value over its kinds, measured against the longdouble reference
FLOOR_EDGE_HOST = dict(identity=dict(G=4.41, g=0.0, f=0.0, chi2=0.0, chi2_m=0.0), pi=dict(G=4.62, g=0.393, f=0.147, chi2=0.181, chi2_m=0.147),
                       scaled=dict(G=4.96, g=0.337, f=0.108, chi2=0.072, chi2_m=0.102), long=dict(G=10.9, g=0.176, f=0.0847, chi2=0.0847, chi2_m=0.381))
FLOOR_EDGE_DEVICE = dict(identity=dict(G=4.41, g=0.0, f=0.0, chi2=0.0, chi2_m=0.0), pi=dict(G=4.62, g=0.393, f=0.147, chi2=0.181, chi2_m=0.147),
                         scaled=dict(G=4.96, g=0.67, f=0.129, chi2=0.144, chi2_m=0.582), long=dict(G=10.8, g=0.16, f=0.0847, chi2=0.0847, chi2_m=0.381))
GATE_EDGE_HOST = {n: {k: 100 * max(v, 1.0) for k, v in fl.items()} for n, fl in FLOOR_EDGE_HOST.items()}
GATE_EDGE_DEVICE = {n: {k: 100 * max(v, 1.0) for k, v in fl.items()} for n, fl in FLOOR_EDGE_DEVICE.items()}
FD_STEP = 1e-6
FLOOR_FD = 1.1e-12
GATE_FD = 100 * FLOOR_FD
FLOOR_FINAL_DEVICE = 2.1e-13   # sigma, measured (dense; ragged 2.0e-13): both loops reach the minimum itself, what is left is rounding
GATE_FINAL_DEVICE = 100 * FLOOR_FINAL_DEVICE

# measurements per factor: 0, 1, 2 and 17 dealt so that every wavefront of four factors mixes them; the last two factors have none
COUNTS = fx.COUNTS
SIZES = fx.SIZES
# explicit state indices of the nine factors over twelve states: factors 2 and 5 join the same pair (7, 2), state 7 is state i of three factors
IDX_I = (3, 0, 7, 7, 1, 7, 9, 4, 10)
IDX_J = (4, 5, 2, 8, 6, 2, 1, 11, 0)
EARTH = np.array([4.2e6, 1.7e5, 4.8e6]) * (5e6 / 4.8e6)      # positions of 5e6 m
# residual rotations; the last one is pi less 1e-6: qd.w = 5e-7, so its sign is the data's and not a rounding's (at pi itself e = 2 vec(qd)
# is discontinuous: the flip makes +axis and -axis the same rotation)
ANGLES = (1e-9, 0.03, 1.0, 3.1, np.pi - 1e-6)
VARIANTS = ("chain", "explicit", "earth", "float32")

tri, offsets, unpack_R = fx.tri, fx.offsets, fx.unpack_R


def hslot(a, b):
    """Where entry (a, b) of the 31 x 31 symmetric row sits in its 496 doubles."""
    return tri(max(a, b)) + min(a, b)


def touched(kind):
    c = COLS[kind]
    return [hslot(c[a], c[b]) for b in range(len(c)) for a in range(b + 1)]


def unpack_row(row):
    """[..., 496] -> the symmetric [..., 31, 31]."""
    H = np.zeros(row.shape[:-1] + (31, 31), dtype=row.dtype)
    for b in range(31):
        for a in range(b + 1):
            H[..., a, b] = H[..., b, a] = row[..., tri(b) + a]
    return H


# --------------------------------------------------------------------------------------------- longdouble geometry
def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=LD)


def rot_ld(q):
    """(quat_2_Rot(q), |terms|) of cpi_math.hpp in longdouble: (2 w^2 - 1) I - 2 w [v x] + 2 v v^T, q as it is (not normalised)."""
    q = np.asarray(q, dtype=LD)
    v, w = q[:3], q[3]
    R = (2 * w * w - 1) * np.eye(3, dtype=LD) - 2 * w * skew(v) + 2 * np.outer(v, v)
    u = (2 * w * w + 1) * np.eye(3, dtype=LD) + 2 * abs(w) * np.abs(skew(v)) + 2 * np.outer(np.abs(v), np.abs(v))
    return R, u


def _unit_flip(r, t):
    n = np.sqrt((r * r).sum())
    r, t = r / n, t / n
    return (-r, t) if r[3] < 0 else (r, t)


def _inv(q):
    return np.concatenate([-q[:3], q[3:4]])


def residual_ld(kind, xi, xj, z):
    """(e [d], |e| [d], J [d, 30], |J| [d, 30]) of one measurement by the table of the contract, in longdouble."""
    xi, xj, z = (np.asarray(a, dtype=LD) for a in (xi, xj, z))
    d = D[kind]
    e, ue, J, uJ = (np.zeros(s, dtype=LD) for s in (d, d, (d, 30), (d, 30)))
    Ri, uRi = rot_ld(xi[:4])
    if ROT[kind]:
        Rj, uRj = rot_ld(xj[:4])
        r_in, t_in = _unit_flip(*fx.quat_mul_ld(xj[:4], _inv(xi[:4])))
        r, t = fx.quat_mul_ld(z[:4], _inv(r_in))
        t = t + fx.quat_mul_ld(z[:4], t_in)[1]                                # the rounding of the inner product, carried through the outer one
        r, t = _unit_flip(r, t)
        e[:3], ue[:3] = 2 * r[:3], 2 * t[:3] + np.abs(2 * r[:3])
        J[:3, 0:3], uJ[:3, 0:3] = Rj @ Ri.T, uRj @ uRi.T
        J[:3, 15:18], uJ[:3, 15:18] = -np.eye(3, dtype=LD), np.eye(3, dtype=LD)
    if POS[kind]:
        pr, zp = (3, 4) if ROT[kind] else (0, 0)
        dp = xj[13:16] - xi[13:16]
        y, uy = Ri @ dp, uRi @ np.abs(dp)
        e[pr:pr + 3], ue[pr:pr + 3] = z[zp:zp + 3] - y, np.abs(z[zp:zp + 3]) + uy
        J[pr:pr + 3, 0:3], uJ[pr:pr + 3, 0:3] = -skew(y), np.abs(skew(uy))
        J[pr:pr + 3, 12:15], uJ[pr:pr + 3, 12:15] = Ri, uRi
        J[pr:pr + 3, 27:30], uJ[pr:pr + 3, 27:30] = -Ri, uRi
    return e, ue, J, uJ


def retract_ld(x, delta):
    """cpi_retract_batch's map in longdouble: q' = [sin(n/2)/n dtheta, cos(n/2)] (x) q, normalised; the other twelve x + delta."""
    x, delta = np.asarray(x, dtype=LD), np.asarray(delta, dtype=LD)
    th = delta[:3]
    n = np.sqrt((th * th).sum())
    dq = np.concatenate([np.sin(n / 2) / n * th, [np.cos(n / 2)]]) if n > 0 else np.array([0, 0, 0, 1], dtype=LD)
    q = fx.quat_mul_ld(dq, x[:4])[0]
    return np.concatenate([q / np.sqrt((q * q).sum()), x[4:] + delta[3:]])


def fd_jacobian(kind, xi, xj, z, h=FD_STEP):
    """Central differences of residual_ld through retract_ld: [d, 30]."""
    J = np.zeros((D[kind], 30), dtype=LD)
    for c in range(30):
        dl = np.zeros(15, dtype=LD)
        dl[c % 15] = h
        plus = residual_ld(kind, retract_ld(xi, dl), xj, z)[0] if c < 15 else residual_ld(kind, xi, retract_ld(xj, dl), z)[0]
        minus = residual_ld(kind, retract_ld(xi, -dl), xj, z)[0] if c < 15 else residual_ld(kind, xi, retract_ld(xj, -dl), z)[0]
        J[:, c] = (plus - minus) / (2 * LD(h))
    return J


def exact_z(kind, xi, xj):
    """z [ZN] in longdouble at which the rotation residual is zero (to 2^-64): q_j (x) inv(q_i); the position part stays 0."""
    z = np.zeros(ZN[kind], dtype=LD)
    if ROT[kind]:
        z[:4] = _unit_flip(*fx.quat_mul_ld(np.asarray(xj[:4], dtype=LD), _inv(np.asarray(xi[:4], dtype=LD))))[0]
    return z


# --------------------------------------------------------------------------------------------- the cases
class Case:
    """One call: states [S, 16], idx_i / idx_j [F] or None, mfirst [F + 1], z [M, ZN], R [M, RN], weight [M], base [F, 496], chi2_base [F]."""

    def __init__(self, kind, counts, variant="chain", seed=5, idx=None, S=12):
        """idx: (idx_i, idx_j) of the explicit variant over S states where the nine pairs of IDX_I / IDX_J do not reach (edge_case("many"))."""
        assert variant in VARIANTS
        rng = np.random.default_rng(seed + 17 * kind + 101 * VARIANTS.index(variant))
        self.kind, self.variant, self.counts = kind, variant, np.asarray(counts, dtype=np.int64)
        F, d = len(counts), D[kind]
        self.F, self.mfirst = F, offsets(counts)
        M = self.M = int(self.mfirst[-1])
        explicit = variant == "explicit"
        S = self.S = S if explicit else F + 1
        self.idx_i = np.array(IDX_I[:F] if idx is None else idx[0], dtype=np.int32) if explicit else None
        self.idx_j = np.array(IDX_J[:F] if idx is None else idx[1], dtype=np.int32) if explicit else None
        self.states = np.zeros((S, 16))
        for s in range(S):
            self.states[s, :4] = fx._unit_quat(rng)
            self.states[s, 4:] = rng.standard_normal(12) * np.repeat([1e-2, 1.0, 1e-1, 5.0], 3)
        if variant == "earth":
            self.states[:, 13:16] += EARTH
            assert np.abs(self.states[:, 13:16]).max() >= 5e6
        if variant == "float32":
            self.states[:, :4] = fx._f32(self.states[:, :4])
        self.z = np.zeros((M, ZN[kind]))
        fi, fj = self.pairs()
        owner = self.owner()
        for m in range(M):
            xi, xj = self.states[fi[owner[m]]], self.states[fj[owner[m]]]
            if ROT[kind]:
                rel = lc._quat_mul(xj[:4], _inv(xi[:4]))
                self.z[m, :4] = lc._quat_mul(lc._quat_of(rng.standard_normal(3), ANGLES[m % 5]), rel)
                if m % 3 == 1:
                    self.z[m, :4] = -self.z[m, :4]                             # the same rotation: qd.w < 0 before the flip
            if POS[kind]:
                y = np.asarray(rot_ld(xi[:4])[0] @ np.asarray(xj[13:16] - xi[13:16], dtype=LD), dtype=np.float64)
                self.z[m, ZN[kind] - 3:] = y + 0.1 * rng.standard_normal(3)
        if variant == "float32" and ROT[kind]:
            self.z[:, :4] = fx._f32(self.z[:, :4])
        scale = {0: 10.0, 1: 50.0, 2: np.array([50.0] * 3 + [10.0] * 3)}[kind]
        Rd = np.triu(np.eye(d) + 0.3 * rng.standard_normal((M, d, d))) * np.asarray(scale)[..., None] if M else np.zeros((0, d, d))
        self.R = np.zeros((M, RN[kind]))
        for k in range(d):
            for i in range(k + 1):
                self.R[:, tri(k) + i] = Rd[:, i, k]
        self.weight = rng.uniform(0.25, 2.0, M)
        B = np.zeros((F, 31, 31))
        sc = np.concatenate([cc.SCALES, cc.SCALES])
        for f in range(F):
            A = np.triu(np.eye(31) + 0.1 * rng.standard_normal((31, 31)))
            A[:30, :30] *= sc[:, None]
            B[f] = A.T @ A
        self.base = np.stack([[B[f][a, b] for b in range(31) for a in range(b + 1)] for f in range(F)]) if F else np.zeros((0, 496))
        self.chi2_base = np.abs(rng.standard_normal(F)) * 3.0

    def pairs(self):
        if self.idx_i is None:
            return np.arange(self.F), np.arange(self.F) + 1
        return self.idx_i.astype(np.int64), self.idx_j.astype(np.int64)

    def owner(self):
        return np.repeat(np.arange(self.F), self.counts)

    def head(self, F):
        """The first F factors with their measurements: the same data at another F."""
        c = Case.__new__(Case)
        M = int(self.mfirst[F])
        c.kind, c.variant, c.counts, c.F, c.M, c.mfirst = self.kind, self.variant, self.counts[:F], F, M, self.mfirst[:F + 1].copy()
        if self.idx_i is None:
            c.S, c.states, c.idx_i, c.idx_j = F + 1, np.ascontiguousarray(self.states[:F + 1]), None, None
        else:
            c.S, c.states, c.idx_i, c.idx_j = self.S, self.states, self.idx_i[:F].copy(), self.idx_j[:F].copy()
        c.base, c.chi2_base = np.ascontiguousarray(self.base[:F]), np.ascontiguousarray(self.chi2_base[:F])
        c.z, c.R, c.weight = (np.ascontiguousarray(a[:M]) for a in (self.z, self.R, self.weight))
        return c


@functools.lru_cache(maxsize=None)
def case(kind, F, variant="chain"):
    """The first F factors of the nine of COUNTS: a factor's data does not depend on F."""
    if F == len(COUNTS):
        return Case(kind, COUNTS, variant)
    return case(kind, len(COUNTS), variant).head(F)


def all_cases(kind):
    """Every (name, case) the comparisons run over: the chained form at every size, the other variants at nine factors."""
    out = [("chain-%d" % F, case(kind, F)) for F in SIZES]
    out += [(v, case(kind, 9, v)) for v in VARIANTS[1:] if not (v == "float32" and not ROT[kind])]
    return out


# --------------------------------------------------------------------------------------------- the edge builders
PI_Z = tuple(tuple(s * v for v in np.eye(4)[a]) for a in range(3) for s in (1.0, -1.0))     # +x -x +y -y +z -z: qd.w == 0 exactly
Z_SCALES = (0.5, 3.0, 1e-150)
LONG_COUNTS = (0, 300, 1, 33, 0)
MANY, MANY_SEED, MANY_S = 1027, 61, 40      # 257 workgroups of four factors, the last one with three live factors
EDGE_BUILDERS = (("identity", (0, 1, 2)), ("pi", (1, 2)), ("scaled", (1, 2)), ("long", (0, 1, 2)), ("many", (0, 1, 2)))


def _on_the_grid(c, rng):
    """Identity quaternions and positions that are multiples of 0.25: R_i = I, y = p_j - p_i and every product of quaternions exact."""
    c.states[:, :4] = [0.0, 0.0, 0.0, 1.0]
    c.states[:, 13:16] = 0.25 * rng.integers(-40, 41, (c.S, 3))
    fi, fj = c.pairs()
    own = c.owner()
    return c.states[fj[own], 13:16] - c.states[fi[own], 13:16]


@functools.lru_cache(maxsize=None)
def edge_case(name, kind):
    """One of EDGE_BUILDERS (the tests leave what comes back unchanged):
      identity  every kind: the nine chained factors, state quaternions [0, 0, 0, 1], positions multiples of 0.25, z quaternion
                [0, 0, 0, 1], z_p = p_j - p_i: every residual is exactly +-0.0
      pi        kinds 1, 2: the same states, z quaternion PI_Z[m % 6] (+-1 on one axis): qd.w == 0 exactly, a rotation of exactly pi, where
                "negated when qd.w < 0" leaves e_th = 2 vec(qd) as it is; z_p off the exact value by multiples of 0.25; the pose kind with
                a diagonal R, so that the rotation and the position rows of [A | b] do not mix
      scaled    kinds 1, 2: the nine chained factors, z quaternion times Z_SCALES[m % 3] (residual_ld normalises the product)
      long      every kind: LONG_COUNTS measurements per factor, a fold of 300
      many      every kind: MANY factors over MANY_S states, the pairs of IDX_I / IDX_J continued by a seeded draw (i != j), COUNTS tiled"""
    assert kind in dict(EDGE_BUILDERS)[name], (name, kind)
    rng = np.random.default_rng(1000 + 10 * [n for n, _ in EDGE_BUILDERS].index(name) + kind)
    if name == "long":
        return Case(kind, LONG_COUNTS, seed=MANY_SEED + 1)
    if name == "many":
        i = rng.integers(0, MANY_S, MANY)
        j = (i + 1 + rng.integers(0, MANY_S - 1, MANY)) % MANY_S
        i[:9], j[:9] = IDX_I, IDX_J
        assert (i != j).all()
        return Case(kind, np.tile(COUNTS, MANY // len(COUNTS) + 1)[:MANY], "explicit", seed=MANY_SEED, idx=(i, j), S=MANY_S)
    c = Case(kind, COUNTS)
    if name == "scaled":
        c.z[:, :4] *= np.asarray(Z_SCALES)[np.arange(c.M) % 3][:, None]
        return c
    dp = _on_the_grid(c, rng)
    if ROT[kind]:
        c.z[:, :4] = [0.0, 0.0, 0.0, 1.0] if name == "identity" else np.asarray(PI_Z)[np.arange(c.M) % 6]
    if POS[kind]:
        c.z[:, ZN[kind] - 3:] = dp if name == "identity" else dp + 0.25 * rng.integers(1, 9, (c.M, 3))
    if name == "pi" and kind == 2:
        for k in range(6):
            c.R[:, tri(k):tri(k) + k] = 0.0
    return c


def reversed_case(c):
    """(the case with its factors in reverse order, order [F], meas [M]: where every factor and measurement of it sits in c); the states
    stay where they are, so the case has explicit indices."""
    assert c.idx_i is not None
    order = np.arange(c.F - 1, -1, -1)
    meas = np.concatenate([np.arange(c.mfirst[f], c.mfirst[f + 1]) for f in order]).astype(np.int64)
    mv = c.head(c.F)
    mv.counts = c.counts[order]
    mv.mfirst = offsets(mv.counts)
    mv.base, mv.chi2_base = c.base[order], c.chi2_base[order]
    mv.idx_i, mv.idx_j = c.idx_i[order].copy(), c.idx_j[order].copy()
    mv.z, mv.R, mv.weight = c.z[meas], c.R[meas], c.weight[meas]
    return mv, order, meas


def without(c, drop):
    """The case with the measurements drop [M] bool deleted."""
    v = c.head(c.F)
    own = c.owner()
    v.counts = np.bincount(own[~drop], minlength=c.F).astype(np.int64)
    v.mfirst = offsets(v.counts)
    v.M = int(v.mfirst[-1])
    v.z, v.R, v.weight = (np.ascontiguousarray(a[~drop]) for a in (c.z, c.R, c.weight))
    return v


# --------------------------------------------------------------------------------------------- reference and metrics
def reference(c, weight=True, base=True):
    """By the table of the contract in longdouble -> dict(hess [F, 496], chi2 [F], chi2_m [M]) and the units u_hess, u_chi2, u_chi2_m
    (without the 2^-53).  Entries of hess that no measurement touches are the base's (or 0) with unit 0: they must be exact."""
    kind, d = c.kind, D[c.kind]
    hess = np.array(c.base if base else np.zeros((c.F, 496)), dtype=LD)
    u_hess = np.zeros((c.F, 496), dtype=LD)
    chi2 = np.array(c.chi2_base if base else np.zeros(c.F), dtype=LD)
    u_chi2 = np.abs(chi2)
    chi2_m, u_chi2_m = np.zeros(c.M, dtype=LD), np.zeros(c.M, dtype=LD)
    R = unpack_R(c.R, d)
    tch = touched(kind)
    ia, ib = np.array([a for b in range(31) for a in range(b + 1)]), np.array([b for b in range(31) for a in range(b + 1)])
    fi, fj = c.pairs()
    for f in range(c.F):
        if c.counts[f]:
            u_hess[f, tch] = np.abs(hess[f, tch])
        for m in range(c.mfirst[f], c.mfirst[f + 1]):
            w = LD(c.weight[m]) if weight else LD(1)
            e, ue, J, uJ = residual_ld(kind, c.states[fi[f]], c.states[fj[f]], c.z[m])
            A = np.concatenate([R[m] @ J, -(R[m] @ e)[:, None]], axis=1)
            uA = np.concatenate([np.abs(R[m]) @ uJ, (np.abs(R[m]) @ ue)[:, None]], axis=1)
            chi2_m[m], u_chi2_m[m] = (A[:, 30] ** 2).sum(), (uA[:, 30] ** 2).sum()
            H, uH = A.T @ A, uA.T @ uA
            hess[f] += w * H[ia, ib]
            u_hess[f] += abs(w) * uH[ia, ib]
            chi2[f] += w * chi2_m[m]
            u_chi2[f] += abs(w) * u_chi2_m[m]
    return dict(hess=hess, chi2=chi2, chi2_m=chi2_m, u_hess=u_hess, u_chi2=u_chi2, u_chi2_m=u_chi2_m)


@functools.lru_cache(maxsize=None)
def edge_reference(name, kind, weight=True, base=True):
    """reference() of an edge builder, computed once and shared (the tests leave it unchanged)."""
    return reference(edge_case(name, kind), weight, base)


_IB = np.array([b for b in range(31) for a in range(b + 1)])
_IA = np.array([a for b in range(31) for a in range(b + 1)])


def metrics(hess, chi2, chi2_m, ref):
    """dict(G, g, f, chi2, chi2_m) in units; entries with unit 0 must be exact (asserted here: they are copies)."""
    tiny = np.finfo(np.float64).tiny
    m = {}
    if hess is not None:
        err = np.abs(np.asarray(hess, dtype=LD) - ref["hess"])
        exact = ref["u_hess"] == 0
        assert (err[exact] == 0).all(), "an entry that no measurement touches differs from the base"
        r = np.where(exact, 0, err / np.maximum(ref["u_hess"] * EPS_HALF, tiny))
        m["G"] = float(r[:, _IB < 30].max(initial=0))
        m["g"] = float(r[:, (_IB == 30) & (_IA < 30)].max(initial=0))
        m["f"] = float(r[:, 495].max(initial=0))
    if chi2 is not None:
        err = np.abs(np.asarray(chi2, dtype=LD) - ref["chi2"])
        m["chi2"] = float(np.where(ref["u_chi2"] == 0, err, err / np.maximum(ref["u_chi2"] * EPS_HALF, tiny)).max(initial=0))
    if chi2_m is not None and len(chi2_m):
        m["chi2_m"] = float((np.abs(np.asarray(chi2_m, dtype=LD) - ref["chi2_m"]) / np.maximum(ref["u_chi2_m"] * EPS_HALF, tiny)).max())
    return m


def documented(c, e, J, weight=True, base=True):
    """The summation orders of include/cpi_amd.h in float64, from the residuals e [M, d] and the Jacobians J [M, d, 30] ->
    (hess [F, 496], chi2 [F], chi2_m [M])."""
    fma = lc.fma
    kind, d, cols = c.kind, D[c.kind], COLS[c.kind]
    nc = len(cols)
    hess = np.array(c.base if base else np.zeros((c.F, 496)), dtype=np.float64)
    chi2 = np.array(c.chi2_base if base else np.zeros(c.F), dtype=np.float64)
    chi2_m = np.zeros(c.M)
    Rat = lambda m, i, k: float(c.R[m, tri(k) + i])
    for f in range(c.F):
        for m in range(c.mfirst[f], c.mfirst[f + 1]):
            w = float(c.weight[m]) if weight else 1.0
            A = np.zeros((d, nc))
            for r in range(d):
                acc = 0.0
                for k in range(r, d):
                    acc = fma(Rat(m, r, k), e[m, k], acc)
                A[r, nc - 1] = -acc
                for ci in range(nc - 1):
                    acc = 0.0
                    for k in range(r, d):
                        acc = fma(Rat(m, r, k), J[m, k, cols[ci]], acc)
                    A[r, ci] = acc
            x2 = np.float64(A[0, nc - 1]) * np.float64(A[0, nc - 1])
            for r in range(1, d):
                x2 = x2 + np.float64(A[r, nc - 1]) * np.float64(A[r, nc - 1])
            chi2_m[m] = x2
            chi2[f] = fma(w, float(x2), chi2[f])
            for b in range(nc):
                for a in range(b + 1):
                    acc = 0.0
                    for r in range(d):
                        acc = fma(A[r, a], A[r, b], acc)
                    s = hslot(cols[a], cols[b])
                    hess[f, s] = fma(w, acc, hess[f, s])
    return hess, chi2, chi2_m


def _rot64(q):
    """quat_2_Rot of cpi_math.hpp in float64, operation for operation (no contraction)."""
    v, w = [np.float64(a) for a in q[:3]], np.float64(q[3])
    two = np.float64(2)
    c = two * w * w - np.float64(1)
    S = [[np.float64(0), -v[2], v[1]], [v[2], np.float64(0), -v[0]], [-v[1], v[0], np.float64(0)]]
    return [[c * np.float64(1.0 if i == j else 0.0) - two * w * S[i][j] + two * v[i] * v[j] for j in range(3)] for i in range(3)]


def position_e_J(xi, xj, z):
    """e [3] and J [3, 30] of one POSITION measurement in float64 in the documented order: d_p = p_j - p_i, y_r the fma chain over k,
    e = z - y, J = [-[y x] | R_i at p_i | -R_i at p_j]."""
    Ri = _rot64(xi[:4])
    dp = [np.float64(xj[13 + k]) - np.float64(xi[13 + k]) for k in range(3)]
    y = []
    for r in range(3):
        acc = 0.0
        for k in range(3):
            acc = lc.fma(Ri[r][k], dp[k], acc)
        y.append(np.float64(acc))
    e = np.array([np.float64(z[k]) - y[k] for k in range(3)])
    J = np.zeros((3, 30))
    J[:, 0:3] = [[0.0, y[2], -y[1]], [-y[2], 0.0, y[0]], [y[1], -y[0], 0.0]]
    J[:, 12:15] = Ri
    J[:, 27:30] = -np.array(Ri)
    return e, J


# --------------------------------------------------------------------------------------------- the end-to-end cases on the CPU
def e2e_betweens(pred, lay, seed=29):
    """The between measurements of an end-to-end case from the UNPERTURBED states pred [S, 16] of tests/chain_pipeline.py and a
    fx.layout(): a relative pose on every factor of every chain (0.01 rad, 0.02 m), and a body-frame displacement on every second
    factor (0.05 m), every z moved by a seeded draw of its noise.  mfirst indexes the chains' factors in their compacted order.  A list
    of dicts of numpy arrays as Engine.chain_lm takes tensors: kind, z, R, mfirst."""
    rng = np.random.default_rng(seed)
    fi, fj = lay["fi"], lay["fj"]
    F = len(fi)
    z = np.zeros((F, 7))
    for f in range(F):
        xi, xj = pred[fi[f]], pred[fj[f]]
        rel = lc._quat_mul(xj[:4], _inv(xi[:4]))
        z[f, :4] = lc._quat_mul(lc._quat_of(rng.standard_normal(3), 0.01 * abs(rng.standard_normal()) + 1e-4), rel)
        z[f, 4:] = np.asarray(rot_ld(xi[:4])[0] @ np.asarray(xj[13:16] - xi[13:16], dtype=LD), dtype=np.float64) + 0.02 * rng.standard_normal(3)
    Rp = np.zeros((F, 21))
    for a in range(6):
        Rp[:, tri(a) + a] = 100.0 if a < 3 else 50.0
    Rp[:, tri(4) + 1] = 5.0                                                  # an off-diagonal entry: rotation against position
    pose = dict(kind="pose", z=z, R=Rp, mfirst=np.arange(F + 1, dtype=np.int64))
    has = (np.arange(F) % 2 == 0)
    rows = np.flatnonzero(has)
    zp = np.stack([np.asarray(rot_ld(pred[fi[f], :4])[0] @ np.asarray(pred[fj[f], 13:16] - pred[fi[f], 13:16], dtype=LD), dtype=np.float64) for f in rows])
    zp = zp + 0.05 * rng.standard_normal(zp.shape)
    pos = dict(kind="position", z=zp, R=np.tile(np.array([20.0, 0, 20.0, 0, 0, 20.0]), (len(rows), 1)), mfirst=offsets(has.astype(np.int64)))
    return [pose, pos]


def between_rows_ld(betweens, st, fi, fj):
    """(rows [F, 496], chi2 [F]) of the betweens at the states st, in longdouble, on a zero base."""
    F = len(fi)
    rows, chi2 = np.zeros((F, 496), dtype=LD), np.zeros(F, dtype=LD)
    for b in betweens:
        c = Case.__new__(Case)
        c.kind = KINDS.index(b["kind"])
        c.F, c.S, c.mfirst, c.counts = F, len(st), b["mfirst"], np.diff(b["mfirst"])
        c.M, c.states, c.z, c.R = len(b["z"]), st, b["z"], b["R"]
        c.idx_i, c.idx_j = np.asarray(fi, dtype=np.int32), np.asarray(fj, dtype=np.int32)
        c.weight = b.get("weight", np.ones(c.M))
        c.base, c.chi2_base = np.zeros((F, 496)), np.zeros(F)
        r = reference(c)
        rows, chi2 = rows + r["hess"], chi2 + r["chi2"]
    return rows, chi2


class BetweenLoop(fx.FixLoop):
    """fix_cases.FixLoop -- lm_cases.CpuLoop over the chains of a layout() -- with measurements between consecutive states: their chi2
    joins the factors' chi2 in every chain's cost, their rows join the factors' rows of the solve.  evaluate=False leaves them out of the
    solve and of the accept rule (the loop without the betweens) while objective() still evaluates the whole objective."""

    def __init__(self, anchor, prior0, betweens, lay=None, fixes=(), evaluate=True):
        super().__init__(anchor, prior0, list(fixes), lay)
        self.betweens, self.evaluate = betweens, evaluate

    def costs(self, st, force=False):
        L = self.lay
        ref, eta, cost = super().costs(st)
        if self.evaluate or force:
            self.brows, chi2 = between_rows_ld(self.betweens, st, L["fi"], L["fj"])
            extra = [LD(0.5) * chi2[ff:ff + n - 1].sum() for n, ff in zip(L["count"], L["ffirst"])]
            cost = np.asarray(np.asarray(cost, dtype=LD) + np.asarray(extra, dtype=LD), dtype=np.float64)
        else:
            self.brows = np.zeros((len(L["fi"]), 496), dtype=LD)
        return ref, eta, cost

    def objective(self, st):
        """The whole objective per chain at st, betweens included whatever `evaluate` says."""
        return self.costs(st, force=True)[2]

    def batch(self, ref, prior):
        L = self.lay
        hess = np.asarray(self.fc.hessian_longdouble(ref, self.R[L["keep"]]) + self.brows, dtype=np.float64)
        return cc.Batch.from_arrays(L["count"], L["first"], L["ffirst"], hess, prior)
