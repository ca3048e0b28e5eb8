"""Inputs, references and metrics of the Levenberg-Marquardt step per chain (cpi_prior_relinearize_batch, cpi_chain_cost_batch,
cpi_chain_accept_batch; tests/test_lm_cpu.py on the host twin, tests/test_gpu_lm.py on the device).  TEST INFRASTRUCTURE ONLY.
Built on tests/chain_cases.py (RAGGED, Batch, pack_upper) and tests/chain_pipeline.py (the end-to-end chains).

Three kinds of statement:
  * the two FIXED summation orders restated in float64 numpy (prior_documented, chain_cost_documented) and the rule of the decision
    (accept_expected): compared bit for bit, no tolerance;
  * the same quantities in numpy.longdouble by their definitions (prior_reference, chain_cost_reference), xi from the oracle's
    localCoordinates: compared within a gate;
  * a CPU loop of the same rules over the longdouble pieces of tests/chain_pipeline.py: cpu_case() (CpuLoop), for the end-to-end case.

Metrics, in the natural unit of each quantity (printed by the tests before anything is asserted):
    eta    max_i |eta_i - ref_i| / (((|Lam| |xi|)_i + |eta0_i|) 2^-53)
    pcost  |pcost - ref| / ((0.5 |xi|^T |Lam| |xi| + |eta0|^T |xi|) 2^-53)
    cost   |cost - ref| / ((0.5 sum |chi2| + sum |pcost|) 2^-53)
    final  max |local(final state, the CPU loop's)_i| / sigma_i, sigma from chain_marginals at the final states
Gates = 100 x the floor, the rule of tests/tol.py; a floor is the largest value measured over every case of the tests and never below
one unit.  Measured (profiles/chain_lm.md):
    host twin (tests/hostsim/hostsim_lm.cpp, x86-64)    eta 79   pcost 6.1   cost 2.0
    device (MI355X)                                      eta 86   pcost 13    cost 2.0   final 1.93e-13 sigma
hard_prior_case (GPS-sized positions, float32-rounded and scaled quaternions) stays below them: eta 5.6 / pcost 4.1 on the host twin,
10.6 / 5.8 on the device.  A wrong term shows as 1e13 units and more (the mutation checks of tests/test_lm_cpu.py)."""
import functools
from fractions import Fraction

import numpy as np

from tests import chain_cases as cc

LD = np.longdouble
EPS_HALF = cc.EPS_HALF
SENTINEL = -7.0
RUNNING, CONVERGED, GAVE_UP = 0, 1, 2
DEFAULTS = dict(lam_down=0.1, lam_up=10.0, lam_min=0.0, lam_max=1e5, abs_tol=1e-5, rel_tol=1e-5)
PARAM_NAMES = ("lam_down", "lam_up", "lam_min", "lam_max", "abs_tol", "rel_tol")

FLOOR_ETA_HOST, FLOOR_PCOST_HOST, FLOOR_COST_HOST = 79.0, 6.1, 2.0
FLOOR_ETA_DEVICE, FLOOR_PCOST_DEVICE, FLOOR_COST_DEVICE = 86.0, 13.0, 2.0
FLOOR_FINAL_DEVICE = 2e-13  # sigma: both loops reach the minimum itself (the last accepted step is quadratic), so what is left is rounding
GATE_ETA_HOST, GATE_PCOST_HOST, GATE_COST_HOST = (100 * max(f, 1.0) for f in (FLOOR_ETA_HOST, FLOOR_PCOST_HOST, FLOOR_COST_HOST))
GATE_ETA_DEVICE, GATE_PCOST_DEVICE, GATE_COST_DEVICE = (100 * max(f, 1.0) for f in (FLOOR_ETA_DEVICE, FLOOR_PCOST_DEVICE, FLOOR_COST_DEVICE))
GATE_FINAL_DEVICE = 100 * FLOOR_FINAL_DEVICE


def fma(a, b, c):
    """round(a b + c) with ONE rounding (exact rational arithmetic, then the correctly rounded conversion); NaN / inf as IEEE has them."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return float(np.float64(a) * np.float64(b) + np.float64(c))
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return float(np.float64(a) * np.float64(b) + np.float64(c))          # the sign of an exact zero: as the rounded operations give it
    return float(r)


def sym_at(row, i, d):
    return row[cc.tri(d) + i] if i <= d else row[cc.tri(i) + d]


# --------------------------------------------------------------------------------------------- prior_relinearize
def prior_documented(xi, prior0):
    """The summation orders of include/cpi_amd.h in float64: xi [P, 15], prior0 [P, 136] -> (rows [P, 136], pcost [P])."""
    xi, prior0 = np.asarray(xi, dtype=np.float64), np.asarray(prior0, dtype=np.float64)
    rows, pcost = prior0.copy(), np.zeros(len(xi))
    for p in range(len(xi)):
        t = np.zeros(15)
        for i in range(15):
            acc = prior0[p, 120 + i]
            for k in range(15):
                acc = fma(sym_at(prior0[p], i, k), xi[p, k], acc)
            rows[p, 120 + i] = acc
            t[i] = np.float64(acc) + prior0[p, 120 + i]
        rows[p, 135] = 0.0
        acc = 0.0
        for i in range(15):
            acc = fma(xi[p, i], t[i], acc)
        pcost[p] = 0.5 * acc
    return rows, pcost


def oracle_local(x, other):
    from oracle import oracle_py as op
    orc = op.oracle()
    return np.stack([orc.local(x[k], other[k]) for k in range(len(x))]) if len(x) else np.zeros((0, 15))


def prior_reference(xi, prior0):
    """By the definition in longdouble: (eta [P, 15], pcost [P], unit_eta [P, 15], unit_pcost [P]), the units without the 2^-53."""
    xi = np.asarray(xi, dtype=LD)
    Lam = cc.unpack_sym(np.where(np.arange(136) == 135, 0.0, prior0), 16)[:, :15, :15]
    eta0 = np.asarray(prior0[:, 120:135], dtype=LD)
    eta = eta0 + np.einsum("pik,pk->pi", Lam, xi)
    pcost = LD(0.5) * np.einsum("pi,pik,pk->p", xi, Lam, xi) + (eta0 * xi).sum(1)
    u_eta = np.einsum("pik,pk->pi", np.abs(Lam), np.abs(xi)) + np.abs(eta0)
    u_pc = LD(0.5) * np.einsum("pi,pik,pk->p", np.abs(xi), np.abs(Lam), np.abs(xi)) + (np.abs(eta0) * np.abs(xi)).sum(1)
    return eta, pcost, u_eta, u_pc


def prior_metrics(rows, pcost, xi_ref, prior0, skip=None):
    """(eta, pcost) metrics of rows [P, 136] / pcost [P] against the longdouble reference at xi_ref.  Left out: records with NaN, and
    the records of skip -- those AT their anchor, where xi is zero by construction and the oracle's own rounding of the quaternion
    product (1e-17 absolute) is all the reference would hold: the tests hold these records to exact equality instead."""
    eta, pc, u_eta, u_pc = prior_reference(xi_ref, prior0)
    ok = np.isfinite(np.asarray(eta, dtype=np.float64)).all(1) & np.isfinite(prior0[:, :135]).all(1)
    if skip is not None:
        ok &= ~np.asarray(skip, dtype=bool)
    tiny = np.finfo(np.float64).tiny
    m_eta = (np.abs(np.asarray(rows[:, 120:135], dtype=LD) - eta) / np.maximum(u_eta * EPS_HALF, tiny))[ok]
    m_pc = (np.abs(np.asarray(pcost, dtype=LD) - pc) / np.maximum(u_pc * EPS_HALF, tiny))[ok]
    return float(m_eta.max()) if m_eta.size else 0.0, float(m_pc.max()) if m_pc.size else 0.0


def _quat_of(axis, angle):
    axis = axis / np.linalg.norm(axis)
    q = np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])
    return -q if q[3] < 0 else q


def _quat_mul(q, p):
    qv, pv = q[:3], p[:3]
    r = np.concatenate([q[3] * pv + p[3] * qv - np.cross(qv, pv), [q[3] * p[3] - qv @ pv]])
    r = r / np.linalg.norm(r)
    return -r if r[3] < 0 else r


@functools.lru_cache(maxsize=None)
def prior_case(S, seed=11):
    """states [S, 16], anchor [S, 16], prior0 [S, 136] for S records in state order.  Record p: p % 4 == 0 sits AT its anchor; the
    others are rotated away from it by up to pi (p % 4 == 3: within 1e-3 of pi, where localCoordinates flips the sign) and moved in
    the additive entries; eta0 is zero for even p (a Gaussian prior) and non-zero for odd p (a marginalised one); Lam = R^T R with the
    row scales of tests/chain_cases.py.  Entry 135 holds NaN: it is never read."""
    rng = np.random.default_rng(seed)
    states, anchor, prior0 = np.zeros((S, 16)), np.zeros((S, 16)), np.zeros((S, 136))
    for p in range(S):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        states[p, :4] = -q if q[3] < 0 else q
        states[p, 4:] = rng.standard_normal(12) * np.repeat([1e-2, 1.0, 1e-1, 5.0], 3)
        anchor[p] = states[p]
        if p % 4:
            angle = {1: rng.uniform(0.01, 0.1), 2: rng.uniform(0.1, 3.0), 3: np.pi - 1e-3 * rng.uniform()}[p % 4]
            anchor[p, :4] = _quat_mul(_quat_of(rng.standard_normal(3), angle), states[p, :4])
            anchor[p, 4:] += rng.standard_normal(12) * np.repeat([1e-4, 1e-2, 1e-3, 1e-2], 3)
        R = cc.SCALES[:, None] * np.triu(np.eye(15) + 0.1 * rng.standard_normal((15, 15)))
        P = np.zeros((16, 16))
        P[:15, :15] = R.T @ R
        if p % 2:
            P[:15, 15] = P[15, :15] = np.diag(P)[:15] * 0.01 * rng.standard_normal(15)
        P[15, 15] = np.nan
        prior0[p] = cc.pack_upper(P)
    return states, anchor, prior0


HARD_OFFSET = np.array([4.2e6, -1.7e5, 4.8e6])


@functools.lru_cache(maxsize=None)
def hard_prior_case(S, seed=11):
    """prior_case(S) away from its comfortable range: the positions of state and anchor moved by the same HARD_OFFSET (a GPS position),
    the quaternions of odd records rounded to float32 (unit to 1e-8 only), those of every third record scaled -- the state's by 0.5 and
    the anchor's by 2 where p % 6 == 0, the other way round where p % 6 == 3.  localCoordinates normalises the product, so the
    reference (xi from the oracle) is the contract's."""
    states, anchor, prior0 = (a.copy() for a in prior_case(S, seed))
    p = np.arange(S)
    for a in (states, anchor):
        a[:, 13:16] += HARD_OFFSET
        a[p % 2 == 1, :4] = a[p % 2 == 1, :4].astype(np.float32).astype(np.float64)
    for a, (s0, s3) in ((states, (0.5, 2.0)), (anchor, (2.0, 0.5))):
        a[p % 6 == 0, :4] *= s0
        a[p % 6 == 3, :4] *= s3
    return states, anchor, prior0


# --------------------------------------------------------------------------------------------- chain_cost
def chain_cost_documented(chi2, pcost):
    """The fixed shape of include/cpi_amd.h in float64: the chain's chi2 rows [n - 1] and pcost rows [n] (either may be empty)."""
    v = np.zeros(16)
    for q in range(16):
        a = b = np.float64(0.0)
        for x in np.asarray(chi2, dtype=np.float64)[q::16]:
            a = a + x
        for x in np.asarray(pcost, dtype=np.float64)[q::16]:
            b = b + x
        v[q] = np.float64(0.5) * a + b
    with np.errstate(invalid="ignore"):
        for s in (8, 4, 2, 1):
            v = v + v[np.arange(16) ^ s]
    return float(v[0])


def chain_ranges(call):
    """[(first state, states, first factor row, refused)] of a cc.Call, clamped as the entries clamp them."""
    out = []
    for c in range(call.C):
        f, n = call.states(c)
        ff = int(call.ffirst[c]) if call.ffirst is not None else f - c
        out.append((f, n, ff, n > 1 and (ff < 0 or ff > call.b.F - (n - 1))))
    return out


def chain_costs(call, chi2, pcost, documented=True):
    """cost [C] of a cc.Call over chi2 [F] / pcost [S] or None: the documented float64 shape, or (documented=False) the longdouble sums
    with their units (cost, unit)."""
    cost, unit = np.zeros(call.C), np.zeros(call.C)
    for c, (f, n, ff, bad) in enumerate(chain_ranges(call)):
        x2 = chi2[ff:ff + n - 1] if (n > 1 and not bad and chi2 is not None) else np.zeros(0)
        pc = pcost[f:f + n] if (pcost is not None and not bad) else np.zeros(0)
        if bad:
            cost[c] = unit[c] = np.nan
        elif documented:
            cost[c] = chain_cost_documented(x2, pc)
        else:
            cost[c] = float(LD(0.5) * np.asarray(x2, dtype=LD).sum() + np.asarray(pc, dtype=LD).sum())
            unit[c] = float(LD(0.5) * np.abs(np.asarray(x2, dtype=LD)).sum() + np.abs(np.asarray(pc, dtype=LD)).sum())
    return cost if documented else (cost, unit)


# every layout of the cost tests: dense C x G, and the ragged chains on and beside the 16-slot stride, with an empty chain and an empty wavefront
COST_LAYOUTS = [("dense %dx%d" % (Cn, G), [G] * Cn, "tile") for Cn in (1, 3, 4, 5, 9) for G in (1, 2, 16, 17, 33)] + \
               [("ragged", cc.RAGGED, "tile"), ("gaps", cc.RAGGED, "gaps"), ("reverse", cc.RAGGED, "reverse"), ("empty wave", cc.EMPTY_WAVE, "tile")]


def cost_call(b):
    """The call of a batch as the entries take it: all three arrays when the layout is explicit, count alone when the chains tile the
    states but differ in length, nothing when they tile them exactly."""
    return cc.Call.explicit(b) if b.explicit else (cc.Call(b, count=b.count) if (b.count != b.G).any() else cc.Call(b))


def cost_metric(cost, call, chi2, pcost):
    ref, unit = chain_costs(call, chi2, pcost, documented=False)
    ok = np.isfinite(ref) & (unit > 0)
    return float((np.abs(cost[ok] - ref[ok]) / (unit[ok] * EPS_HALF)).max()) if ok.any() else 0.0


def cost_terms(b, seed=5, negative=False):
    """chi2 [F] >= 0 and pcost [S] for a cc.Batch, NaN in the rows of no chain; negative: pcost large and negative (a negative cost)."""
    rng = np.random.default_rng(seed)
    chi2, pcost = np.full(max(b.F, 0), np.nan), np.full(b.S, np.nan)
    for c in range(b.C):
        n = int(b.count[c])
        if n > 1:
            chi2[b.ffirst[c]:b.ffirst[c] + n - 1] = rng.chisquare(15, n - 1)
        pcost[b.first[c]:b.first[c] + n] = rng.standard_normal(n) * 3.0 - (40.0 * n if negative else 0.0)
    return chi2, pcost


# --------------------------------------------------------------------------------------------- chain_accept
def lm_rule(cur, new, lam, p):
    """The rule of include/cpi_amd.h for one running chain with states -> (accepted, cost, lambda, phase)."""
    with np.errstate(invalid="ignore"):
        cur, new, lam = np.float64(cur), np.float64(new), np.float64(lam)
        if new < cur:
            dec = cur - new
            conv = dec <= p["abs_tol"] or dec <= np.float64(p["rel_tol"]) * abs(cur)
            return 1, float(new), float(max(lam * np.float64(p["lam_down"]), np.float64(p["lam_min"]))), CONVERGED if conv else RUNNING
        if abs(new - cur) <= max(np.float64(p["abs_tol"]), np.float64(p["rel_tol"]) * abs(cur)):
            return 0, float(cur), float(lam), CONVERGED
        l = lam * np.float64(p["lam_up"])
        if not (l <= p["lam_max"]):
            return 0, float(cur), float(lam), GAVE_UP
        return 0, float(cur), float(l), RUNNING


def accept_expected(call, params, chi2_new, pcost_new, trial, cost, states, chi2, lam, phase):
    """What cpi_chain_accept_batch must leave: (cost, states, chi2, lam, phase, accepted), every array a copy; new is the documented cost."""
    p = dict(DEFAULTS, **(params or {}))
    cost, states, lam, phase = cost.copy(), states.copy(), lam.copy(), phase.copy()
    chi2 = None if chi2 is None else chi2.copy()
    accepted = np.zeros(call.C, dtype=np.int32)
    new = chain_costs(call, chi2_new, pcost_new)
    for c, (f, n, ff, bad) in enumerate(chain_ranges(call)):
        if phase[c] != 0:
            continue
        if n == 0:
            phase[c] = CONVERGED
            continue
        accepted[c], cost[c], lam[c], ph = lm_rule(cost[c], new[c], lam[c], p)
        if ph:
            phase[c] = ph
        if accepted[c]:
            states[f:f + n] = trial[f:f + n]
            if chi2 is not None and n > 1:
                chi2[ff:ff + n - 1] = chi2_new[ff:ff + n - 1]
    return cost, states, chi2, lam, phase, accepted


class AcceptCase:
    """The arrays of one call of cpi_chain_accept_batch over a cc.Call: sentinels in states / chi2 and in every row of no chain."""

    def __init__(self, call, chi2_new, pcost_new, cost, lam, phase, params=None, seed=9):
        rng = np.random.default_rng(seed)
        b = call.b
        self.call, self.params = call, params
        self.chi2_new, self.pcost_new = chi2_new, pcost_new
        self.trial = rng.standard_normal((b.S, 16))
        self.states = SENTINEL - np.arange(b.S * 16, dtype=np.float64).reshape(b.S, 16) / 1024.0
        self.chi2 = SENTINEL - np.arange(b.F, dtype=np.float64) / 1024.0
        self.cost, self.lam, self.phase = np.asarray(cost, dtype=np.float64), np.asarray(lam, dtype=np.float64), np.asarray(phase, dtype=np.int32)

    def expected(self, with_chi2=True):
        return accept_expected(self.call, self.params, self.chi2_new, self.pcost_new, self.trial, self.cost, self.states,
                               self.chi2 if with_chi2 else None, self.lam, self.phase)


# rule -> (states, chi2_new rows, pcost_new of the first state, cur - new (None: cur given), cur, lambda, phase, what it must give:
# (accepted, phase, lambda)); four per wavefront, every wavefront with an accept, a reject and a frozen chain
RULE_PARAMS = dict(lam_min=1e-3)
RULES = [
    ("accept",                    3, [1.0, 2.0], 0.25, 1.0, None, 1.0, 0, (1, RUNNING, 0.1)),
    ("reject",                    3, [1.0, 2.0], 0.25, -1.0, None, 1.0, 0, (0, RUNNING, 10.0)),
    ("frozen converged",          3, [1.0, 2.0], 0.25, 1.0, None, 1.0, 1, (0, CONVERGED, 1.0)),
    ("NaN new",                   3, [1.0, np.nan], 0.25, None, 5.0, 1.0, 0, (0, RUNNING, 10.0)),
    ("accept, abs_tol",           2, [4.0], 0.0, 5e-6, None, 2.0, 0, (1, CONVERGED, 0.2)),
    ("reject, stalled",           2, [4.0], 0.0, -5e-6, None, 2.0, 0, (0, CONVERGED, 2.0)),
    ("frozen gave up",            3, [1.0, 2.0], 0.25, 1.0, None, 1.0, 2, (0, GAVE_UP, 1.0)),
    ("NaN cur",                   3, [1.0, 2.0], 0.25, None, np.nan, 1.0, 0, (0, RUNNING, 10.0)),
    ("accept, rel_tol, cur < 0",  3, [1.0, 2.0], -1001.505, None, -1000.0, 1.0, 0, (1, CONVERGED, 0.1)),
    ("reject into GAVE_UP",       3, [1.0, 2.0], 0.25, -1.0, None, 5e4, 0, (0, GAVE_UP, 5e4)),
    ("frozen, other value",       3, [1.0, 2.0], 0.25, 1.0, None, 1.0, 7, (0, 7, 1.0)),
    ("no states",                 0, [], 0.0, None, 3.0, 1.0, 0, (0, CONVERGED, 1.0)),
    ("one state",                 1, [], 0.5, 1.0, None, 1.0, 0, (1, RUNNING, 0.1)),
    ("lam_min clamp",             3, [1.0, 2.0], 0.25, 1.0, None, 5e-3, 0, (1, RUNNING, 1e-3)),
    ("factor rows outside",       3, [1.0, 2.0], 0.25, None, 5.0, 1.0, 0, (0, RUNNING, 10.0)),
    ("new == cur",                3, [1.0, 2.0], 0.25, 0.0, None, 1.0, 0, (0, CONVERGED, 1.0)),
]


def rule_table(outside=True):
    """(AcceptCase, [the (accepted, phase, lambda) every rule must give]) -- one chain per rule, gap rows between the chains.
    outside=False leaves the factor rows of the "factor rows outside" chain where they belong (the host forms REFUSE such a call, naming
    the chain: they are compared with the device form on this table; the chain is then an ordinary accepted one)."""
    counts = [r[1] for r in RULES]
    b = cc.Batch(counts, seed=1, layout="gaps")
    b.G = 3
    outside = [r[0] for r in RULES].index("factor rows outside") if outside else -1
    if outside >= 0:
        b.ffirst[outside] = b.F - 1                                           # two rows from F - 1 on
    call = cc.Call.explicit(b)
    chi2_new, pcost_new = np.full(b.F, np.nan), np.full(b.S, np.nan)
    for c, r in enumerate(RULES):
        n = r[1]
        if n > 1 and c != outside:
            chi2_new[b.ffirst[c]:b.ffirst[c] + n - 1] = r[2]
        if n > 0:
            pcost_new[b.first[c]:b.first[c] + n] = 0.0
            pcost_new[b.first[c]] = r[3]
    new = chain_costs(call, chi2_new, pcost_new)
    cost = np.array([(new[c] + r[4]) if r[4] is not None else r[5] for c, r in enumerate(RULES)])
    case = AcceptCase(call, chi2_new, pcost_new, cost, [r[6] for r in RULES], [r[7] for r in RULES], params=RULE_PARAMS)
    return case, [r[8] for r in RULES]


# The equalities and infinities of the rule, and chains on both sides of the copy loop's trip of 128 sixteen-byte pieces (16 states);
# the columns of RULES, the parameters of RULE_PARAMS (lam_up 10, lam_max 1e5, abs_tol = rel_tol = 1e-5).  1e4 * 10 is 1e5 without
# rounding; 2e-5 - 1e-5 is the double 1e-5 without rounding (a binary doubling).  cur = +inf over a finite new is an accept that
# CONVERGES by the rule as written: dec = inf <= rel_tol * |cur| = inf.
INF = float("inf")
RULES_EDGE = [
    ("lambda * lam_up == lam_max",  3, [1.0, 2.0], 0.25, -1.0, None, 1e4, 0, (0, RUNNING, 1e5)),
    ("cur - new == abs_tol",        2, [0.0], 1e-5, None, 2e-5, 2.0, 0, (1, CONVERGED, 0.2)),
    ("cur +inf, new finite",        3, [1.0, 2.0], 0.25, None, INF, 1.0, 0, (1, CONVERGED, 0.1)),
    ("new -inf",                    3, [1.0, 2.0], -INF, None, 5.0, 1.0, 0, (1, RUNNING, 0.1)),
    ("cur == new == +inf",          3, [1.0, 2.0], INF, None, INF, 1.0, 0, (0, RUNNING, 10.0)),
    ("lambda 0 on a reject",        3, [1.0, 2.0], 0.25, -1.0, None, 0.0, 0, (0, RUNNING, 0.0)),
    ("16 states accepted",          16, [1.0] * 15, 0.25, 1.0, None, 1.0, 0, (1, RUNNING, 0.1)),
    ("17 states accepted",          17, [1.0] * 16, 0.25, 1.0, None, 1.0, 0, (1, RUNNING, 0.1)),
    ("32 states accepted",          32, [1.0] * 31, 0.25, 1.0, None, 1.0, 0, (1, RUNNING, 0.1)),
]


def edge_rule_table():
    """(AcceptCase, [the (accepted, phase, lambda) every rule of RULES_EDGE must give]) -- one chain per rule, gap rows between the
    chains; every expected triple is the one lm_rule gives (asserted here)."""
    b = cc.Batch([r[1] for r in RULES_EDGE], seed=2, layout="gaps")
    call = cc.Call.explicit(b)
    chi2_new, pcost_new = np.full(b.F, np.nan), np.full(b.S, np.nan)
    for c, r in enumerate(RULES_EDGE):
        chi2_new[b.ffirst[c]:b.ffirst[c] + r[1] - 1] = r[2]
        pcost_new[b.first[c]:b.first[c] + r[1]] = 0.0
        pcost_new[b.first[c]] = r[3]
    new = chain_costs(call, chi2_new, pcost_new)
    cost = np.array([(new[c] + r[4]) if r[4] is not None else r[5] for c, r in enumerate(RULES_EDGE)])
    p = dict(DEFAULTS, **RULE_PARAMS)
    for c, r in enumerate(RULES_EDGE):
        acc, _, lam, ph = lm_rule(cost[c], new[c], r[6], p)
        assert (acc, ph, lam) == r[8], (r[0], acc, ph, lam)
    assert 1e4 * p["lam_up"] == p["lam_max"] and cost[1] - new[1] == p["abs_tol"]
    case = AcceptCase(call, chi2_new, pcost_new, cost, [r[6] for r in RULES_EDGE], [r[7] for r in RULES_EDGE], params=RULE_PARAMS)
    return case, [r[8] for r in RULES_EDGE]


def ragged_accept_case(layout="tile", seed=4):
    """RAGGED chains: even chains get a cheaper trial, odd ones a dearer one, chain 5 is frozen."""
    b = cc.Batch(cc.RAGGED, seed=3, layout=layout)
    call = cc.Call.explicit(b) if b.explicit else cc.Call(b, count=b.count)
    chi2_new, pcost_new = cost_terms(b, seed=seed)
    new = chain_costs(call, chi2_new, pcost_new)
    cost = new + np.where(np.arange(b.C) % 2 == 0, 2.0, -2.0)
    phase = np.zeros(b.C, dtype=np.int32)
    phase[5] = CONVERGED
    return AcceptCase(call, chi2_new, pcost_new, cost, np.full(b.C, 0.5), phase)


# --------------------------------------------------------------------------------------------- the end-to-end case on the CPU
class CpuLoop:
    """The loop of INTEGRATION.md 3p on the CPU with the longdouble pieces tests/chain_pipeline.py: cpu_case() uses (the oracle's
    preintegration, evaluate_error_longdouble, hessian_longdouble, the dense longdouble solve of tests/chain_cases.py, the oracle's
    retract / local), for the chains of tests/chain_pipeline.py with one prior record per chain on its first state."""

    def __init__(self, anchor, prior0):
        from oracle import oracle_py as op
        from tests import chain_pipeline as cp
        from tests import factor_cases as fc
        from tests.tol import sqrt_info_longdouble
        self.cp, self.fc = cp, fc
        x = cp.inputs()
        kn, lin = x["knots"].numpy(), x["lin"].numpy()
        self.orc = op.oracle()
        out = self.orc.run(op.make_params(1, 0, 1), kn, lin, x["q"].numpy())
        self.rec = op.factor_records(out, lin, None)
        Rl = sqrt_info_longdouble(np.asarray(out["P"]).reshape(cp.F, 15, 15))
        self.R = np.ascontiguousarray(Rl.transpose(0, 2, 1).reshape(cp.F, 225))
        self.ii, self.jj = cp.indices()
        self.anchor, self.prior0 = np.asarray(anchor, dtype=np.float64), np.asarray(prior0, dtype=np.float64)

    def costs(self, st):
        cp = self.cp
        ref = self.fc.evaluate_error_longdouble(1, self.rec, st[self.ii], st[self.jj])
        w = self.fc.whitened_longdouble(ref, self.R)[0]
        chi2 = (w * w).sum(1).reshape(cp.C, cp.G - 1)
        xi = oracle_local(st[0::cp.G], self.anchor)
        eta, pcost, _, _ = prior_reference(xi, self.prior0)
        return ref, eta, np.asarray(LD(0.5) * chi2.sum(1) + pcost, dtype=np.float64)

    def run(self, states, lam, iterations, params=None):
        cp = self.cp
        p = dict(DEFAULTS, **(params or {}))
        st, lam = np.array(states, dtype=np.float64), np.full(cp.C, lam, dtype=np.float64)
        phase = np.zeros(cp.C, dtype=np.int32)
        ref, eta, cost = self.costs(st)
        history = [cost.copy()]
        for _ in range(iterations):
            hess = np.asarray(self.fc.hessian_longdouble(ref, self.R), dtype=np.float64)
            prior = np.zeros((cp.S, 136))
            prior[0::cp.G] = self.prior0
            prior[0::cp.G, 120:135] = np.asarray(eta, dtype=np.float64)
            prior[:, 135] = 0.0
            b = cc.Batch.from_arrays([cp.G] * cp.C, np.arange(cp.C) * cp.G, np.arange(cp.C) * (cp.G - 1), hess, prior)
            delta = cc.Reference(b, lam, True).delta
            trial = np.stack([self.orc.retract(st[s], delta[s]) for s in range(cp.S)])
            ref_t, eta_t, new = self.costs(trial)
            for c in range(cp.C):
                if phase[c] != 0:
                    continue
                acc, cost[c], lam[c], ph = lm_rule(cost[c], new[c], lam[c], p)
                if ph:
                    phase[c] = ph
                if acc:
                    st[c * cp.G:(c + 1) * cp.G] = trial[c * cp.G:(c + 1) * cp.G]
            ref, eta, _ = self.costs(st)
            history.append(cost.copy())
        return st, cost, lam, phase, np.stack(history)
