"""CPU: host emulation of the carry path (tests/hostsim/hostsim_carry.cpp, the kernels' arithmetic from cpi_math.hpp).

A window of the pinned traces (tests/golden/trace_v1.npz / trace_v2.npz: the state after every interval) is split at
knot s into two segments that share knot s; the first starts from the zero state, the second from the first's carry
record.  The first segment's result must match the trace snapshot at the split, the second's the final state, at the
regression gates (tests/tol.py).  Covered: the mean recursion for every lane split the kernels use (L in 1, 2, 5, 16, 64;
model 2 mean-only with several lanes composes through the gravity response, GSEG), with and without the analytic
Jacobians, and the column-lane covariance recursion.  The golden batch pre_w48 (imu_avg 0 and 1) checks the final state of
two- and three-segment chains."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.tol import check_pre

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_carry.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_carry.so")
_HDR = os.path.join(os.path.dirname(_HERE), "cpi_amd", "csrc", "cpi_math.hpp")
GRAV = np.array([0.0, 0.0, 9.8])
SIG = np.array([0.005, 4e-6, 0.01, 2e-4])
SPLITS = [0, 1, 17, 49, 50]
LANES = [1, 2, 5, 16, 64]
FIELDS = [("DT", 1), ("alpha", 3), ("beta", 3), ("q", 4), ("R", 9), ("J_q", 9), ("J_a", 9), ("J_b", 9), ("H_a", 9),
          ("H_b", 9), ("O_a", 9), ("O_b", 9), ("P", 225)]


@pytest.fixture(scope="module")
def lib():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-o", _LIB, _SRC])
    return C.CDLL(_LIB)


def _dp(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double))


def _split(raw):
    out, o = {}, 0
    for name, n in FIELDS:
        out[name] = raw[o:o + n][None]
        o += n
    return out


class _Seg:
    """Runs one segment (knots kn[n + 1]) from carry record cin (None = the zero state); returns (outputs, carry)."""

    def __init__(self, lib, model, avg, kind, L=1, jac=False):
        self.lib, self.model, self.avg, self.kind, self.L, self.jac = lib, model, avg, kind, L, jac
        self.cd = lib.hsc_carry_doubles(model)

    def __call__(self, kn, lin, q, cin):
        kn = np.ascontiguousarray(kn, dtype=np.float64)
        out, cout = np.zeros(308), np.full(self.cd, np.nan)
        n = kn.shape[0] - 1
        if self.kind == "mean":
            self.lib.hsc_mean(self.model, int(self.jac), self.avg, self.L, n, _dp(kn), _dp(lin), _dp(q), _dp(GRAV), _dp(cin),
                              _dp(cout), _dp(out))
        else:
            self.lib.hsc_cov(self.model, self.avg, n, _dp(kn), _dp(lin), _dp(q), _dp(SIG), _dp(GRAV), _dp(cin), _dp(cout),
                             _dp(out))
        return _split(out), cout


def _configs():
    cfg = []
    for model in (1, 2):
        for L in LANES:
            cfg.append((model, "mean", L, False))                     # model 2, L > 1: GSEG
            if model == 1 or L == 1:                                  # model 2 with analytic Jacobians: one lane (pick_lanes)
                cfg.append((model, "mean", L, True))
        cfg.append((model, "cov", 1, False))
    return cfg


def _what(model, kind, jac):
    if kind == "cov":
        return ("mean", "jac", "cov") if model == 2 else ("mean", "cov")
    return ("mean", "jac") if jac else ("mean",)


def _zero_state():
    z = {name: np.zeros((1, n)) for name, n in FIELDS}
    z["q"][0, 3] = 1.0
    z["R"][0, [0, 4, 8]] = 1.0
    return z


@pytest.mark.parametrize("model,kind,L,jac", _configs())
@pytest.mark.parametrize("split", SPLITS)
def test_split_vs_trace(lib, golden_dir, model, kind, L, jac, split):
    """trace_v1 / trace_v2 are mode (model, imu_avg 0, stj 1): model 2's analytic Jacobians (stj 0) are not in them, so those
    runs check the means here and the Jacobians against pre_w48 below."""
    d = dict(np.load(os.path.join(golden_dir, "trace_v%d.npz" % model)))
    kn, lin, q = d["knots"], d["lin"], d["q_k_lin"]
    seg = _Seg(lib, model, 0, kind, L, jac)
    what = _what(model, kind, jac)
    if model == 2 and kind == "mean":
        what = ("mean",)
    a, carry = seg(kn[:split + 1], lin, q, None)
    ref_a = _zero_state() if split == 0 else {k: v[split - 1:split] for k, v in d.items() if k in dict(FIELDS)}
    label = "m%d %s L=%d jac=%d split=%d" % (model, kind, L, jac, split)
    check_pre(a, ref_a, what=what, v2=(model == 2), label=label + " at the split", regression=True)
    assert np.all(np.isfinite(carry[:17]))
    b, carry = seg(kn[split:], lin, q, carry)
    ref_b = {k: v[-1:] for k, v in d.items() if k in dict(FIELDS)}
    check_pre(b, ref_b, what=what, v2=(model == 2), label=label + " final", regression=True)
    np.testing.assert_allclose(b["R"][0], ref_b["R"][0], rtol=0, atol=2e-13)


def _mode_out(d, m, w):
    key = "m%d_avg%d_stj%d__" % m
    return {k[len(key):]: v[w:w + 1] for k, v in d.items() if k.startswith(key)}


@pytest.mark.parametrize("model,kind,L,jac", _configs())
@pytest.mark.parametrize("avg", [0, 1])
def test_chains_vs_golden(lib, golden_dir, model, kind, L, jac, avg):
    d = dict(np.load(os.path.join(golden_dir, "pre_w48.npz")))
    rng = np.random.default_rng(31 + 7 * model + 3 * avg + L)
    seg = _Seg(lib, model, avg, kind, L, jac)
    stj = 0 if (model == 2 and kind == "mean" and jac) else 1
    for w in range(0, d["knots"].shape[0], 3):
        kn, lin, q = d["knots"][w], d["lin"][w], d["q_k_lin"][w]
        cuts = [0] + sorted(rng.integers(0, 51, size=2).tolist()) + [50]   # repeats = empty segments
        carry = None
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            out, carry = seg(kn[c0:c1 + 1], lin, q, carry)
        check_pre(out, _mode_out(d, (model, avg, stj), w), what=_what(model, kind, jac), v2=(model == 2),
                  label="m%d %s L=%d jac=%d avg=%d w=%d cuts=%s" % (model, kind, L, jac, avg, w, cuts), regression=True)


def test_carry_sizes_match_the_library(lib):
    """The emulation restates the record layout of cpi_args.hpp: its sizes must be the library's."""
    from cpi_amd import _lib
    dev = _lib.load()
    assert [lib.hsc_carry_doubles(m) for m in (1, 2)] == [dev.cpi_carry_doubles(m) for m in (1, 2)]
