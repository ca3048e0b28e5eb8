"""GPU: model 2's seven bias Jacobians after every interval of a window that continues from a carry record
(cpi_running_resume_stj_batch[_host], Engine.preintegrate_running_resume_stj[_host]).

References: every row of every chain against oracle_py.oracle().trace of the WHOLE window (tests/test_gpu_stj.py's _trace) at
TOL_MEAN / TOL_JAC / TOL_COV (tests/tol.py: check_pre).  The interchange rules -- first segment = cpi_running_stj_batch, mean / P rows
and carry_out = cpi_preintegrate_running_resume, row N - 1 = a zero-interval cpi_preintegrate_resume, repeat rows, host form -- are
checked for exact equality.  Segments are cut on and beside cov_body<2>'s pass length CH: CH - 1, CH, CH + 1 and 2 CH + 1."""
import numpy as np
import pytest
import torch

from tests.test_gpu_stj import ALL, CH, JAC7, MEAN, _bits, _dev, _flat, _np, _trace, _windows
from tests.tol import FieldTable, check_pre, field_gates

pytestmark = pytest.mark.gpu
NT = 3 * CH + 1        # intervals of a whole window: segments of CH - 1 | 2 CH + 2, CH | 2 CH + 1, CH + 1 | 2 CH and three-segment chains
KEYS = MEAN + JAC7 + ("P",)
# Per-field regression gates beside TOL_JAC (tests/tol.py: field_gates): 100 x the largest error against the oracle measured on an
# MI355X over test_chains_match_the_oracle_and_the_older_entries (both layouts and imu_avg settings), never below 2^-53 x max |ref|
# of the field (the table: profiles/stj_edges.md)
FLOOR_CHAIN = {"J_q": 5.55e-16, "J_a": 1.80e-16, "J_b": 1.11e-15, "H_a": 8.33e-17, "H_b": 5.55e-16, "O_a": 8.88e-16, "O_b": 8.44e-15}
CHAINS = [(CH - 1, 2 * CH + 2), (CH, 2 * CH + 1), (CH + 1, 2 * CH), (CH, CH + 1, CH), (CH + 1, CH - 1, CH + 1), (2 * CH + 1, 1, CH - 1)]


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _rec(c):
    """The parts of model 2's records these calls define: tag, means and rotation, and the covariance state with the nine columns
    (the block of the analytic Jacobians in between belongs to cpi_preintegrate_resume with state_transition_jacobians = 0)."""
    c = c.cpu().numpy() if torch.is_tensor(c) else c
    return np.concatenate([c[:, :17], c[:, 80:]], axis=1)


def _segment(eng, kn, lin, q, prm, a, b, carry, want=ALL, entry="preintegrate_running_resume_stj", layout="dense", W=None):
    """Rows [W, b - a, ...] and carry_out of the intervals [a, b) of every window, continued from carry."""
    W = kn.shape[0] if W is None else W
    fn = getattr(eng, entry)
    if layout == "dense":
        return fn(_dev(kn[:W, a:b + 1], eng), _dev(lin[:W], eng), _dev(q[:W], eng), prm, want=want, carry_in=carry)
    n1 = kn.shape[1]
    first = np.arange(W, dtype=np.int64) * n1 + a
    count = np.full(W, b - a, dtype=np.int32)
    return fn(_dev(kn.reshape(-1, 7), eng), _dev(lin[:W], eng), _dev(q[:W], eng), prm, want=want, first=_dev(first, eng), count=_dev(count, eng),
              N=b - a, carry_in=carry)


def _chain(eng, kn, lin, q, prm, lens, layout="dense", W=None, want=ALL):
    """The segments of a chain: list of (a, b, rows (numpy), carry_in, carry_out)."""
    out, a, carry = [], 0, None
    for n in lens:
        rows, co = _segment(eng, kn, lin, q, prm, a, a + n, carry, want=want, layout=layout, W=W)
        out.append((a, a + n, _np(rows), carry, co))
        a, carry = a + n, co
    return out


@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("avg", [0, 1])
def test_chains_match_the_oracle_and_the_older_entries(eng, avg, layout):
    """Chains of two and three segments over windows of 3 CH + 1 intervals, batches of 1, 2 and 3 windows (two windows per wavefront):
    every row of every field against the oracle's trace of the whole window; the first segment is cpi_running_stj_batch's bits; the
    mean and P rows and carry_out of every segment are cpi_preintegrate_running_resume's bits; asking for the Jacobians alone gives the
    same Jacobian bits; a zero-interval cpi_preintegrate_resume on carry_out returns row N - 1's seven matrices bit for bit."""
    kn, lin, q = _windows(NT)
    ref = _trace(avg, kn, lin, q, key=("open", NT))
    prm = eng.make_params(2, bool(avg))
    worst, t = {}, FieldTable(JAC7)
    for ci, lens in enumerate(CHAINS):
        assert sum(lens) == NT
        for W in ((1, 2, 3) if ci == 1 else (3,)):
            segs = _chain(eng, kn, lin, q, prm, lens, layout, W)
            got = {k: np.concatenate([s[2][k] for s in segs], axis=1) for k in KEYS}
            assert all(v.shape[:2] == (W, NT) for v in got.values())
            check_pre(_flat(got, KEYS), _flat({k: v[:W] for k, v in ref.items()}, KEYS), what=("mean", "jac", "cov"), v2=True,
                      label="resume stj %s avg%d W%d %s" % (layout, avg, W, lens))
            for k in JAC7:
                worst[k] = max(worst.get(k, 0.0), float(np.abs(got[k] - ref[k][:W]).max()))
            t.add(got, {k: v[:W] for k, v in ref.items()}, "W%d %s" % (W, lens))
            for si, (a, b, rows, cin, cout) in enumerate(segs):
                if si == 0:
                    closed = _np(eng.preintegrate_running_stj(_dev(kn[:W, a:b + 1], eng), _dev(lin[:W], eng), _dev(q[:W], eng), prm, want=ALL))
                    for k in closed:
                        assert _bits(rows[k], closed[k]), (lens, W, k)
                old, old_c = _segment(eng, kn, lin, q, prm, a, b, cin, want=("mean", "cov", "cov_sym"), entry="preintegrate_running_resume", layout=layout, W=W)
                old = _np(old)
                for k in old:
                    assert _bits(rows[k], old[k]), (lens, W, si, k)
                assert _bits(_rec(cout), _rec(old_c)), (lens, W, si)
                only, only_c = _segment(eng, kn, lin, q, prm, a, b, cin, want=("jac",), layout=layout, W=W)
                only = _np(only)
                assert set(only) == set(JAC7) and all(_bits(only[k], rows[k]) for k in JAC7), (lens, W, si)
                assert _bits(_rec(only_c), _rec(cout)), (lens, W, si)
                fin, _ = eng.preintegrate_resume(_dev(kn[:W, b:b + 1], eng), _dev(lin[:W], eng), _dev(q[:W], eng), prm, want=("mean", "jac", "cov"),
                                                 carry_in=cout)
                fin = _np(fin)
                for k in JAC7 + MEAN + ("P",):
                    assert _bits(fin[k], rows[k][:, -1]), (lens, W, si, k)
    print("resume stj %s avg %d: largest error per field vs oracle.trace: %s" % (layout, avg, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    t.report("resume stj chains %s avg %d, per field" % (layout, avg), field_gates(FLOOR_CHAIN))
    t.check(field_gates(FLOOR_CHAIN), "resume stj chains %s avg %d" % (layout, avg))


@pytest.mark.parametrize("avg", [0, 1])
def test_repeat_rules(eng, avg):
    """A segment whose intervals are all skipped (dt = 0), a count-0 segment and an N = 1 count-0 segment repeat the carried row bit for
    bit in all seven fields (and in the means and P), and pass the state through; rows past a window's count repeat its final state."""
    kn, lin, q = _windows(NT)
    W, m, n = 3, CH + 1, CH
    prm = eng.make_params(2, bool(avg))
    head, carry = _segment(eng, kn, lin, q, prm, 0, m, None, W=W)
    head = _np(head)
    d = [_dev(x[:W], eng) for x in (lin, q)]
    still = kn[:W, m:m + n + 1].copy()
    still[:, :, 0] = still[:, :1, 0]
    for label, kw in (("all skipped", dict(knots=_dev(still, eng))),
                      ("count 0", dict(knots=_dev(kn[:W, m:m + n + 1], eng), count=_dev(np.zeros(W, dtype=np.int32), eng))),
                      ("N 1 count 0", dict(knots=_dev(kn[:W, m:m + 2], eng), count=_dev(np.zeros(W, dtype=np.int32), eng)))):
        rows, co = eng.preintegrate_running_resume_stj(kw.pop("knots"), d[0], d[1], prm, want=ALL, carry_in=carry, **kw)
        rows = _np(rows)
        for k in rows:
            for i in range(rows[k].shape[1]):
                assert _bits(rows[k][:, i], head[k][:, -1]), (label, k, i)
        assert _bits(_rec(co), _rec(carry)), label
    # counts 2, 0 and n: the rows from the count on repeat
    count = np.array([2, 0, n], dtype=np.int32)
    rows, _ = eng.preintegrate_running_resume_stj(_dev(kn[:W, m:m + n + 1], eng), d[0], d[1], prm, want=ALL, carry_in=carry, count=_dev(count, eng))
    rows = _np(rows)
    full = _np(_segment(eng, kn, lin, q, prm, m, m + n, carry, W=W)[0])
    for w in range(W):
        c = int(count[w])
        for k in JAC7:
            assert _bits(rows[k][w, :c], full[k][w, :c]), (w, k)
            last = rows[k][w, c - 1] if c else head[k][w, -1]
            for i in range(c, n):
                assert _bits(rows[k][w, i], last), (w, k, i)


def test_a_wrong_carry_gives_nan_in_that_window_only(eng):
    """A record of another model, and one without covariance state (left by a mean-only call): NaN in all rows of every field of
    that window and a NaN tag in its carry_out; the other windows keep their bits."""
    kn, lin, q = _windows(NT)
    W, m, n = 3, CH, CH + 1
    prm = eng.make_params(2)
    _, carry = _segment(eng, kn, lin, q, prm, 0, m, None, W=W)
    clean, clean_c = _segment(eng, kn, lin, q, prm, m, m + n, carry, W=W)
    clean = _np(clean)
    other = carry.clone()
    tag = int(other[1, 0].item())
    other[1, 0] = float((tag & ~(32 * 3)) | 32 * 1)
    _, means_only = _segment(eng, kn, lin, q, prm, 0, m, None, W=W, want=("mean",), entry="preintegrate_running_resume")
    bare = carry.clone()
    bare[1] = means_only[1]
    assert int(bare[1, 0].item()) & 2 == 0
    for label, bad in (("model", other), ("no covariance state", bare)):
        rows, co = _segment(eng, kn, lin, q, prm, m, m + n, bad, W=W)
        rows = _np(rows)
        for k in rows:
            assert np.isnan(rows[k][1]).all(), (label, k)
            assert _bits(rows[k][[0, 2]], clean[k][[0, 2]]), (label, k)
        assert np.isnan(co.cpu().numpy()[1, 0]) and _bits(_rec(co)[[0, 2]], _rec(clean_c)[[0, 2]]), label


def test_refusals_and_model_1(eng):
    from cpi_amd import CpiError
    kn, lin, q = _windows(CH)
    d = [_dev(x[:2], eng) for x in (kn, lin, q)]
    who = "cpi_running_resume_stj_batch: "
    with pytest.raises(CpiError, match=who + ".*need state_transition_jacobians != 0 here: the analytic O_a / O_b recursion has no running form"):
        eng.preintegrate_running_resume_stj(*d, eng.make_params(2, state_transition_jacobians=False), want=("jac",))
    with pytest.raises(CpiError, match=who + r"model must be 1 or 2 \(the Forster comparator has no running form and cannot be resumed\)"):
        eng.preintegrate_running_resume_stj(*d, eng.make_params(3), want=("mean",))
    with pytest.raises(CpiError, match=who + "model 2 needs q_k_lin"):
        eng.preintegrate_running_resume_stj(d[0], d[1], None, eng.make_params(2), want=("jac",))
    _, c = eng.preintegrate_running_resume_stj(*d, eng.make_params(2), want=("jac",))
    with pytest.raises(CpiError, match=who + "carry_in and carry_out overlap"):
        eng.preintegrate_running_resume_stj(*d, eng.make_params(2), want=("jac",), carry_in=c, carry_out=c)
    with pytest.raises(CpiError, match=r"cpi_preintegrate_running_resume: the Jacobian fields \(J_q ... O_b\) are not available for model 2"):
        eng.preintegrate_running_resume(*d, eng.make_params(2), want=("jac",))
    with pytest.raises(CpiError, match="cpi_running_resume_stj_batch_host: .*analytic O_a / O_b recursion has no running form"):
        eng.preintegrate_running_resume_stj_host(*[x.cpu() for x in d], eng.make_params(2, state_transition_jacobians=False), want=("jac",))
    # without a Jacobian field, or with model 1, the call is the old entry
    for prm, want, qk in ((eng.make_params(2, state_transition_jacobians=False), ("mean", "cov"), d[2]), (eng.make_params(1), ("mean", "jac", "cov"), None)):
        new, nc = eng.preintegrate_running_resume_stj(d[0], d[1], qk, prm, want=want)
        old, oc = eng.preintegrate_running_resume(d[0], d[1], qk, prm, want=want)
        new, old = _np(new), _np(old)
        assert set(new) == set(old) and all(_bits(new[k], old[k]) for k in old) and _bits(nc.cpu().numpy()[:, :17], oc.cpu().numpy()[:, :17])


@pytest.mark.parametrize("avg", [0, 1])
def test_host_form(eng, avg):
    """cpi_running_resume_stj_batch_host: the bits of the device form, rows and records, for a first and a continued segment."""
    kn, lin, q = _windows(NT)
    W, m, n = 3, CH + 1, CH + 1
    prm = eng.make_params(2, bool(avg))
    carry_d = carry_h = None
    for a, b in ((0, m), (m, m + n)):
        rows, co = _segment(eng, kn, lin, q, prm, a, b, carry_d, W=W)
        hrows, hco = eng.preintegrate_running_resume_stj_host(torch.from_numpy(kn[:W, a:b + 1].copy()), torch.from_numpy(lin[:W].copy()),
                                                              torch.from_numpy(q[:W].copy()), prm, want=ALL, carry_in=carry_h)
        rows = _np(rows)
        assert set(hrows) == set(rows) and set(JAC7) <= set(rows)
        for k in rows:
            assert _bits(hrows[k].numpy(), rows[k]), (a, k)
        assert _bits(_rec(hco), _rec(co)), a
        carry_d, carry_h = co, hco
