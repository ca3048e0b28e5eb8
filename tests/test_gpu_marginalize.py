"""GPU: cpi_chain_marginalize_batch against the longdouble Schur complement of tests/marginalize_cases.py, at the smallest shapes where
the kernel changes path: different m inside one wavefront (0, 1, n - 1, a middle value, and one refused), a trip count of 63 beside
chains that stop at once, a wavefront without a single state, chains of two and three states, explicit first with gaps and in
reverse order.  Equivalence: the reduced chains' solve and marginals give the full chains' rows.  Bits: a chain does not depend on
its neighbours, its position or on what it does not eliminate; the host form and the C++ facade are the device form.  The device's own
hess: factor_hessian -> chain_marginalize -> chain_solve replays from one graph.
The metrics of a comparison are printed before anything is asserted; the gates are those of tests/marginalize_cases.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import chain_cases as cc
from tests import marginalize_cases as mz
from tests import marginals_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0
GPU_LAYOUTS = ("ragged", "gaps", "reverse", "one_2", "one_3", "long", "empty_wave")


@pytest.fixture(scope="module")
def eng():
    return cpi_amd.Engine()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ragged_kw(b, dev, first=None, count=None, ffirst=None):
    """first / count / ffirst of a batch as the entries take them: all three when the layout is explicit (or overridden), count alone
    when the chains tile the states but differ in length, nothing when they tile them exactly."""
    if b.explicit or first is not None:
        f, n, ff = (x if y is None else y for x, y in ((b.first, first), (b.count, count), (b.ffirst, ffirst)))
        return dict(first=_t(np.asarray(f, dtype=np.int64), dev), count=_t(np.asarray(n, dtype=np.int32), dev), ffirst=_t(np.asarray(ff, dtype=np.int64), dev))
    if (b.count != b.G).any():
        return dict(count=_t(b.count, dev))
    return {}


def marginalize(eng, b, drop, with_prior=True, host=False, hess=None, prior=None, first=None, count=None, ffirst=None):
    """chain_marginalize of batch b (drop: an int, or [C]) -> (out [C, 136], status [C]) as numpy; the row past out keeps its sentinel."""
    dev = "cpu" if host else eng.device
    Cn = b.C if first is None else len(first)
    buf = torch.full((Cn + 1, 136), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((Cn,), 99, dtype=torch.int32, device=dev)
    d = int(drop) if np.isscalar(drop) else _t(np.asarray(drop, dtype=np.int32), dev)
    pr = _t(b.prior if prior is None else prior, dev) if with_prior else None
    fn = eng.chain_marginalize_host if host else eng.chain_marginalize
    out = fn(_t(b.hess if hess is None else hess, dev), C=Cn, G=b.G, prior=pr, drop=d, out=buf[:Cn], status=status, **_ragged_kw(b, dev, first, count, ffirst))
    if not host:
        torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and (buf[Cn] == SENTINEL).all()
    return buf[:Cn].cpu().numpy(), status.cpu().numpy()


def solve(eng, b, first, count, ffirst, prior, marginals=False):
    """chain_solve (lambda = NULL) of the chains first / count / ffirst on b.hess and prior -> delta [S, 15] (and cov, cross), status."""
    dev = eng.device
    kw = dict(first=_t(first, dev), count=_t(count, dev))
    status = torch.full((len(first),), 99, dtype=torch.int32, device=dev)
    ws = torch.full((eng.chain_solve_workspace_doubles(b.S),), float("nan"), dtype=torch.float64, device=dev)
    delta = eng.chain_solve(_t(b.hess, dev), C=len(first), G=b.G, ffirst=_t(ffirst, dev), prior=_t(prior, dev), status=status, workspace=ws,
                            out=torch.full((b.S, 15), float("nan"), dtype=torch.float64, device=dev), **kw)
    res = [delta.cpu().numpy()]
    if marginals:
        cov, cross = eng.chain_marginals(ws, C=len(first), G=b.G, status=status, cross=True, out=torch.full((b.S, 120), float("nan"), dtype=torch.float64, device=dev), **kw)
        res += [cov.cpu().numpy(), cross.cpu().numpy()]
    torch.cuda.synchronize()
    return res + [status.cpu().numpy()]


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("layout", GPU_LAYOUTS)
def test_against_the_longdouble_schur_complement(eng, layout):
    worst = np.zeros(4)
    for prior_all in ((False, True) if layout == "ragged" else (False,)):
        for plan in mz.PLANS:
            b, drop, ref, full = mz.reference(layout, prior_all, plan)
            out, status = marginalize(eng, b, 1 if plan == "scalar1" else drop)
            m_c, m_d = ref.metrics(out)
            delta, st2 = solve(eng, b, *mz.reduced(b, drop, out, status))
            e_a, e_b = mz.equivalence(full, drop, status, delta)
            print("%s prior %s %s: cond(A_EE) max %.1e, (c) %.3e (d) %.3e, equivalence (a) %.3e (b) %.3e"
                  % (layout, "all" if prior_all else "first", plan, ref.cond.max(), m_c, m_d, e_a, e_b))
            assert np.array_equal(status, ref.status), (plan, status)
            assert (st2 == 0).all(), (plan, st2)
            assert np.isnan(out[status != 0]).all() and np.isfinite(out[status == 0]).all() and (out[status == 0, 135] == 0.0).all()
            for c in ref.lam:
                assert np.isfinite(np.linalg.cholesky(mz.unpack_out(out[c])[0])).all(), (plan, c)
            worst = np.maximum(worst, [m_c, m_d, e_a, e_b])
    print("largest (c) %.3e (floor %.3e, gate %.2e); (d) %.3e (floor %.3e, gate %.2e); equivalence (a) %.3e, (b) %.3e (gate %.2e)"
          % (worst[0], mz.FLOOR_LAM_DEVICE, mz.GATE_LAM_DEVICE, worst[1], mz.FLOOR_ETA_DEVICE, mz.GATE_ETA_DEVICE, worst[2],
             worst[3], cc.GATE_FORWARD_DEVICE))
    assert worst[0] <= mz.GATE_LAM_DEVICE and worst[1] <= mz.GATE_ETA_DEVICE
    assert worst[3] <= cc.GATE_FORWARD_DEVICE                                 # (a) is printed for the record: marginalize_cases.py says why


def test_a_chain_with_m_equal_n_is_refused_alone(eng):
    b, drop, ref, _ = mz.reference("ragged", False, "mixed1")
    good, status = marginalize(eng, b, drop)
    for c in (4, 6, 9):                                                       # 17 states, 5 states, one state: m = n
        bad = drop.copy()
        bad[c] = b.count[c]
        out, st = marginalize(eng, b, bad)
        assert st[c] == -1 and np.isnan(out[c]).all(), c
        others = np.arange(b.C) != c
        assert np.array_equal(st[others], status[others]) and np.array_equal(out[others], good[others], equal_nan=True), c
    neg = drop.copy()
    neg[5] = -1
    out, st = marginalize(eng, b, neg)
    assert st[5] == -1 and np.isnan(out[5]).all() and np.array_equal(np.delete(out, 5, 0), np.delete(good, 5, 0), equal_nan=True)
    far = b.ffirst.copy()
    far[6] = b.F - 1                                                          # chain 6 (5 states): its factor rows leave [0, F)
    out, st = marginalize(eng, b, drop, first=b.first, ffirst=far)
    assert st[6] == -1 and np.isnan(out[6]).all() and np.array_equal(np.delete(out, 6, 0), np.delete(good, 6, 0), equal_nan=True)


# ------------------------------------------------------------------------------------------ 2. bits
def test_position_layout_and_repetition_do_not_change_the_bits(eng):
    for plan in ("mixed0", "mixed3"):
        b, drop, _, _ = mz.reference("ragged", False, plan)
        base, status = marginalize(eng, b, drop)
        again, st = marginalize(eng, b, drop)
        assert np.array_equal(again, base, equal_nan=True) and np.array_equal(st, status)
        for other in ("gaps", "reverse"):
            o, d2, _, _ = mz.reference(other, False, plan)
            assert np.array_equal(d2, drop)
            out, st = marginalize(eng, o, d2)
            assert np.array_equal(out, base, equal_nan=True) and np.array_equal(st, status), (plan, other)
        for c in (4, 5, 10):                                                  # alone, C = 1: its own bits
            one, st = marginalize(eng, b, drop[[c]], first=b.first[[c]], count=b.count[[c]], ffirst=b.ffirst[[c]])
            assert st.tolist() == [0] and np.array_equal(one[0], base[c]), (plan, c)


def test_only_what_is_eliminated_is_read(eng):
    for layout, plan in (("ragged", "mixed2"), ("reverse", "mixed1"), ("long", "mixed3")):
        b, drop, _, _ = mz.reference(layout, layout != "long", plan)
        good, status = marginalize(eng, b, drop)
        hess, prior = b.hess.copy(), b.prior.copy()
        for c in range(b.C):
            n, m = int(b.count[c]), int(drop[c])
            hess[b.ffirst[c] + m:b.ffirst[c] + max(n - 1, 0)] = np.nan
            prior[b.first[c] + m + 1:b.first[c] + n] = np.nan
        out, st = marginalize(eng, b, drop, hess=hess, prior=prior)
        assert np.array_equal(st, status) and np.array_equal(out, good, equal_nan=True), layout


def test_m_zero_passes_the_prior_through(eng):
    for layout in ("ragged", "empty_wave"):                                   # empty_wave: a wavefront of chains without states
        b, _ = mz.case(layout, layout == "ragged")
        out, status = marginalize(eng, b, 0)
        has = b.count > 0
        assert status.tolist() == np.where(has, 0, -1).tolist()
        for c in np.nonzero(has)[0]:
            assert np.array_equal(out[c, :135], b.prior[b.first[c], :135]) and out[c, 135] == 0.0, c
        assert np.isnan(out[~has]).all()
        none, status = marginalize(eng, b, 0, with_prior=False)
        assert (none[has] == 0.0).all() and not np.signbit(none[has]).any() and np.isnan(none[~has]).all()
    b, _ = mz.case("one_1")                                                   # one chain of one state: nothing to eliminate, no hess
    out, status = marginalize(eng, b, np.zeros(1, dtype=np.int32))
    assert status.tolist() == [0] and np.array_equal(out[0, :135], b.prior[0, :135]) and out[0, 135] == 0.0


# ------------------------------------------------------------------------------------------ 3. failed blocks
def test_a_failed_eliminated_block_is_nan_and_alone(eng):
    good, bad, st_solve = cc.failure_plan()                                   # eight chains of four states, broken at states 0 .. 3
    clean, status = marginalize(eng, good.b, 3)
    assert (status == 0).all()
    ref = mz.Reference(good.b, np.full(good.b.C, 3))
    ref.check_inputs()
    for m in (3, 2, 1):
        out, status = marginalize(eng, bad.b, m)
        want = [s if 0 < s <= m else 0 for s in st_solve]                     # a bad block at a state >= m is not looked at
        assert status.tolist() == want, (m, status)
        assert np.isnan(out[status != 0]).all() and np.isfinite(out[status == 0]).all()
    out, status = marginalize(eng, bad.b, 3)                                  # drop above every broken state below 3: the solve's codes
    assert status.tolist() == [s if s <= 3 else 0 for s in st_solve]
    ok = [c for c in range(good.b.C) if c not in cc.FAILURES]
    assert np.array_equal(out[ok], clean[ok])
    m_c, m_d = ref.metrics(out, ok)
    print("neighbours of failed chains: (c) %.3e (d) %.3e" % (m_c, m_d))
    assert m_c <= mz.GATE_LAM_DEVICE and m_d <= mz.GATE_ETA_DEVICE


# ------------------------------------------------------------------------------------------ 4. composition, marginals
def test_composition_of_two_marginalisations(eng):
    """drop = a, then drop = b on the reduced chain with the first output as its prior, against drop = a + b at once: each is within
    its gate of the truth, so they differ by at most two gates."""
    b, _ = mz.case("ragged", True)                                            # a prior on every state: the two routes add it in different places
    long = b.count >= 15
    da, db = np.where(long, 5, 0).astype(np.int32), np.where(long, 7, 0).astype(np.int32)
    ref = mz.Reference(b, da + db)
    ref.check_inputs()
    once, st = marginalize(eng, b, da + db)
    first_out, st1 = marginalize(eng, b, da)
    f2, n2, ff2, prior2 = mz.reduced(b, da, first_out, st1)
    twice, st2 = marginalize(eng, b, db, prior=prior2, first=f2, count=n2, ffirst=ff2)
    assert np.array_equal(st, ref.status) and np.array_equal(st1, st) and np.array_equal(st2, st)
    worst_c = worst_d = 0.0
    for c in ref.lam:
        L1, e1 = mz.unpack_out(once[c])
        L2, e2 = mz.unpack_out(twice[c])
        d = np.sqrt(np.diagonal(ref.lam[c])).astype(np.float64)
        unit = ref.cond[c] * cc.EPS_HALF
        worst_c = max(worst_c, float((np.abs(L1 - L2) / (d[:, None] * d[None, :])).max() / unit))
        worst_d = max(worst_d, float((np.abs(e1 - e2) / (d * float(ref.q[c]))).max() / unit))
    print("5 then 7 against 12 at once: (c) %.3e (gate %.2e), (d) %.3e (gate %.2e)" % (worst_c, 2 * mz.GATE_LAM_DEVICE, worst_d, 2 * mz.GATE_ETA_DEVICE))
    assert len(ref.lam) == 4 and worst_c <= 2 * mz.GATE_LAM_DEVICE and worst_d <= 2 * mz.GATE_ETA_DEVICE


def test_marginals_of_the_reduced_chain_are_the_full_chains(eng):
    b, drop, _, _ = mz.reference("ragged", False, "mixed2")
    ref = mc.Reference(b)
    ref.check_inputs()
    _, cov, cross, st = solve(eng, b, b.first, b.count, b.ffirst, b.prior, marginals=True)
    out, status = marginalize(eng, b, drop)
    _, cov2, cross2, st2 = solve(eng, b, *mz.reduced(b, drop, out, status), marginals=True)
    assert (st == 0).all() and (st2 == 0).all()
    m_full = ref.metric(cov, cross)
    chains = [c for c in ref.A if status[c] == 0]
    for c in chains:                                                          # the kept states' rows from the reduced chain
        lo, hi = int(b.first[c]) + int(drop[c]), int(b.first[c]) + int(b.count[c])
        assert np.isfinite(cov2[lo:hi]).all() and np.isfinite(cross2[lo:hi - 1]).all()
        cov[lo:hi] = cov2[lo:hi]
        cross[lo:hi - 1] = cross2[lo:hi - 1]
    m = ref.metric(cov, cross, chains)
    print("marginals of the reduced chains: metric %.3e (the full chains' own: %.3e; gate %.2e)" % (m, m_full, mc.GATE_DEVICE))
    assert m <= mc.GATE_DEVICE


# ------------------------------------------------------------------------------------------ 5. the host form, the C++ facade
@pytest.mark.parametrize("layout", ["ragged", "reverse", "one_2"])
def test_the_host_form_is_the_device_form(eng, layout):
    b, drop, _, _ = mz.reference(layout, False, "mixed1")
    drop = np.where(b.count > 0, drop, 0)
    dev, sd = marginalize(eng, b, drop)
    host, sh = marginalize(eng, b, drop, host=True)
    assert np.array_equal(sd, sh) and np.array_equal(dev, host, equal_nan=True)
    if layout == "ragged":
        bad = drop.copy()
        bad[5] = b.count[5]
        with pytest.raises(cpi_amd.CpiError, match="drop of chain 5 leaves"):
            marginalize(eng, b, bad, host=True)
        g = cc.Batch(cc.RAGGED, seed=3, layout="gaps")
        g.ffirst[5] = g.F - 3
        with pytest.raises(cpi_amd.CpiError, match="the factor rows of chain 5 leave"):
            marginalize(eng, g, drop, host=True)


def test_marginalize_cpp_facade(eng):
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_marginalize")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_marginalize.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "test_marginalize ok 5 4 2", p.stdout
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[-6:-1]])
    Cn, G = 5, 4                                                              # the chains of the program, on the device form
    P = np.zeros((Cn * G, 16, 16))
    P[0::G, np.arange(15), np.arange(15)] = 1.0
    P[0::G, :15, 15] = P[0::G, 15, :15] = np.arange(1, 16)[None, :] + np.arange(Cn)[:, None]
    H = np.zeros((31, 31))
    H[:30, :30] = np.block([[np.eye(15), -np.eye(15)], [-np.eye(15), np.eye(15)]])
    hess = np.tile(cc.pack_upper(H), (Cn * (G - 1), 1))
    dev = eng.device
    out = cpi_amd.chain_marginalize(_t(hess, dev), C=Cn, G=G, prior=_t(cc.pack_upper(P), dev), drop=2)      # the module-level entry
    assert np.array_equal(out.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------ 6. the device's own hess
@pytest.fixture(scope="module")
def pipe(eng):
    from tests.test_gpu_chain import Pipeline
    return Pipeline(eng)


def test_real_factors_and_one_graph(eng, pipe):
    """The chains of tests/chain_pipeline.py: chain_marginalize(drop=2) then chain_solve on the reduced chains gives the full solve's
    delta for states 2 .. 5; factor_hessian -> chain_marginalize -> chain_solve captured into one graph and replayed gives the eager
    bits."""
    C, G, m = pipe.C, pipe.G, 2
    S, F = C * G, C * (G - 1)
    dev = eng.device
    first = torch.arange(C, dtype=torch.int64, device=dev) * G + m
    count = torch.full((C,), G - m, dtype=torch.int32, device=dev)
    ffirst = torch.arange(C, dtype=torch.int64, device=dev) * (G - 1) + m

    def run(hess, carried, st1, prior2, delta, st2, ws):
        pipe.hessian(eng, out=hess)
        eng.chain_marginalize(hess, C=C, G=G, prior=pipe.prior, drop=m, out=carried, status=st1)
        prior2.copy_(pipe.prior)
        prior2[m::G] = carried                                                # the first state that stays, of every chain
        eng.chain_solve(hess, C=C, G=G, first=first, count=count, ffirst=ffirst, prior=prior2, out=delta, status=st2, workspace=ws)

    def buffers():
        f64 = lambda *s: torch.full(s, -1.0, dtype=torch.float64, device=dev)
        i32 = lambda: torch.full((C,), 99, dtype=torch.int32, device=dev)
        return (f64(F, 496), f64(C, 136), i32(), f64(S, 136), f64(S, 15), i32(), torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev))

    eager = buffers()
    run(*eager)
    torch.cuda.synchronize()
    hess, carried, st1, prior2, delta, st2, _ = (t.cpu().numpy() for t in eager)
    assert st1.tolist() == [0] * C and st2.tolist() == [0] * C and np.isfinite(carried).all()
    b = cc.Batch.from_arrays([G] * C, np.arange(C) * G, np.arange(C) * (G - 1), hess, pipe.prior.cpu().numpy())
    full = cc.Reference(b)
    full.check_inputs()
    ref = mz.Reference(b, np.full(C, m))
    ref.check_inputs()
    m_c, m_d = ref.metrics(carried)
    e_a, e_b = mz.equivalence(full, np.full(C, m), st1, delta)
    print("device hess: cond max %.1e, (c) %.3e (d) %.3e, equivalence (a) %.3e (b) %.3e" % (full.cond.max(), m_c, m_d, e_a, e_b))
    assert (delta[np.arange(S) % G < m] == -1.0).all()                        # the rows of the states that left are not written
    assert m_c <= mz.GATE_LAM_DEVICE and m_d <= mz.GATE_ETA_DEVICE
    assert e_b <= cc.GATE_FORWARD_DEVICE
    bufs = buffers()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(*bufs)                                                            # warm-up on a side stream, as graph capture requires
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(*bufs)
    for t in bufs[:6]:
        t.fill_(-1.0 if t.dtype == torch.float64 else 99)
    graph.replay()
    torch.cuda.synchronize()
    for k in range(6):
        assert torch.equal(bufs[k], eager[k]), k
