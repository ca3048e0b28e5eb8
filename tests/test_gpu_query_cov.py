"""GPU: the covariance at arbitrary times inside a window (cpi_query_cov_batch[_host], Engine.query[_host] with "cov" / "cov_sym",
cpi_host::CpiBatch::at_cov).

Reference for a query (w, t_q): the P of oracle_py.oracle().run on the cut window [knot 0 .. knot i, {clip(t_q), w_i, a_i}], exactly
the windows tests/test_gpu_query.py builds for the means (its _reference is used as it is, so the oracle runs once per case for both
files).  Every query of every case is compared, none is left out, at the contractual gate of tests/tol.py (cov_rel_err <= TOL_COV =
1e-6) and at the regression gate below: 100 x the largest error measured on an MI355X over test_parity (2.878e-15 for both models:
2.878e-13), never looser than TOL_COV (profiles/query_cov_bench.md).  The largest error of a test is printed (pytest -s)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from cpi_amd import synth
from tests.test_gpu_query import CASES, _case, _layout, _queries, _reference
from tests.sqrt_info_cases import e_row
from tests.tol import REG_SQRT_INFO_ROW, TOL_COV, cov_rel_err, sqrt_info_longdouble

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]
MEAN = ("DT", "alpha", "beta", "q")
JAC = ("J_q", "J_a", "J_b", "H_a", "H_b")
# queries per call: a wavefront holds 4 queries (model 1) or 2 (model 2) -- one less, exactly that and one more for both lane maps,
# 7 = two blocks less one, 200 = many blocks
CALL_SIZES = (1, 3, 4, 5, 7, 200)

# Largest cov_rel_err against the oracle over test_parity (all cases, layouts, imu_avg and both source forms of the rows), per model,
# measured on an MI355X (profiles/query_cov_bench.md): the tumbling windows for both models; the seeded windows stay below 1.2e-15.
# The regression gate is 100 x the floor, never looser than TOL_COV.
FLOOR = {1: 2.878e-15, 2: 2.878e-15}
# Composition (test_sqrt_information_at_query_times): largest |R - R_ref| / max |R_ref| of the square-root information of the queried
# P_sym against the longdouble factorisation of the oracle's P, measured as above (model 2, imu_avg 0); gated at 100 x.
FLOOR_SQRT = 7.21e-16


def _gate(model):
    return min(TOL_COV, 100.0 * FLOOR[model])


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _dev(a, eng):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


_TRI = np.array([c * 15 + r for c in range(15) for r in range(c + 1)])                       # packed entry -> index into column-major P
_FULL = np.array([min(r, c) + max(r, c) * (max(r, c) + 1) // 2 for c in range(15) for r in range(15)])   # and back, mirrored


def _tri(P):
    """[.., 225] column-major -> [.., 120]: its packed upper triangle (CPI_TRI_INDEX)."""
    return np.ascontiguousarray(P[..., _TRI])


def _mirror(S):
    """[.., 120] packed upper triangle -> [.., 225]: mirrored across the diagonal."""
    return np.ascontiguousarray(S[..., _FULL])


_rows_cache = {}


def _rows(eng, name, layout, model, avg):
    """The device arguments of a case and its running rows with the means, model 1's Jacobians, P and P_sym."""
    key = (name, layout, model, avg)
    if key not in _rows_cache:
        kn, lin, q, _ = _case(name)
        knots, first, count = _layout(name, layout)[:3]
        N = CASES[name][1]
        prm = eng.make_params(model, bool(avg))
        args = dict(knots=_dev(knots, eng), lin=_dev(lin, eng), q_k_lin=_dev(q, eng), params=prm, first=_dev(first, eng), count=_dev(count, eng),
                    N=None if first is None else N)
        want = ("mean", "cov", "cov_sym") + (("jac",) if model == 1 else ())
        rows = eng.preintegrate_running(args["knots"], args["lin"], args["q_k_lin"], prm, want=want, first=args["first"], count=args["count"],
                                        N=args["N"])
        _rows_cache[key] = (args, rows)
    return _rows_cache[key]


def _source(rows, form):
    """What cpi_query_cov_batch needs of the rows for a covariance-only request, holding the covariance as `form`."""
    return {"q": rows["q"], form: rows[form]}


def _query(eng, args, rows, qw, qt, want=("cov", "cov_sym")):
    return _np(eng.query(args["knots"], args["lin"], rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=args["q_k_lin"], params=args["params"],
                         want=want, first=args["first"], count=args["count"], N=args["N"]))


def _base(rows_np, form, qw, idx):
    """S of every query as the contract defines it: zeros for i == 0, else row w N + i - 1 (P, or P_sym mirrored)."""
    src = rows_np["P"] if form == "P" else _mirror(rows_np["P_sym"])
    S = src[qw, np.maximum(idx - 1, 0)].copy()
    S[idx == 0] = 0.0
    return S


def _stepped(name, layout, qw, qt, idx):
    """Which queries integrate a partial interval: i < n and t_q > t_i."""
    kn = _case(name)[0]
    counts = _layout(name, layout)[3]
    return np.array([i < counts[w] and t > kn[w, i, 0] for w, t, i in zip(qw, qt, idx)])


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("layout", ["dense", "ragged"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("model,avg", MODES)
def test_parity(eng, model, avg, name, layout):
    """The complete query list of the case, unsorted, in calls of 1, 3, 4, 5, 7 and 200 queries (the last call is filled up with
    repeats of earlier queries), once from rows that hold P and once from rows that hold P_sym only: every query against the oracle."""
    qw, qt, idx, ref = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    M = len(qw)
    got = {}
    for form in ("P", "P_sym"):
        P = np.full((M, 225), np.nan)
        rng = np.random.default_rng(3)
        at, c = 0, 0
        while at < M:
            size = CALL_SIZES[c % len(CALL_SIZES)]
            sel = np.arange(at, min(at + size, M))
            sel = np.concatenate([sel, rng.integers(0, M, size - len(sel))])
            out = _query(eng, args, _source(rows, form), qw[sel], qt[sel])
            assert out["P"].shape == (size, 225) and out["P_sym"].shape == (size, 120)
            assert _bits(out["P_sym"], _tri(out["P"])), "P_sym is not the upper triangle of P"
            seen = ~np.isnan(P[sel][:, 0])
            assert _bits(P[sel][seen], out["P"][seen]), "a repeated query gives other bits"
            P[sel] = out["P"]
            at += size
            c += 1
        assert np.isfinite(P).all()
        got[form] = P
    err = {form: cov_rel_err(P, ref["P"]) for form, P in got.items()}
    print("query cov parity model %d avg %d %s %s (%d queries): cov_rel_err from P rows %.3e, from P_sym rows %.3e, the two agree bitwise: %s"
          % (model, avg, name, layout, M, err["P"], err["P_sym"], _bits(got["P"], got["P_sym"])))
    bad = ["%s rows: %.3e > %.1e" % (f, e, _gate(model)) for f, e in err.items() if not e <= _gate(model)]
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ 2. bit rules
def _raw_call(eng, entry, args, rows, qw, qt, out, N=None, W=None):
    """cpi_query_batch / cpi_query_cov_batch through ctypes on device tensors; rows / out: dicts of tensors."""
    knots = args["knots"]
    W = W if W is not None else (knots.shape[0] if args["first"] is None else args["first"].shape[0])
    N = N if N is not None else (knots.shape[1] - 1 if args["first"] is None else args["N"])
    ro, oo = eng._outputs_struct(rows), eng._outputs_struct(out)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = getattr(eng.lib, entry)(eng.ctx, C.byref(args["params"]), W, N, ptr(knots), ptr(args["first"]), ptr(args["count"]), ptr(args["lin"]),
                                 ptr(args["q_k_lin"]), C.byref(ro), len(qt), ptr(qw), ptr(qt), C.byref(oo))
    torch.cuda.synchronize()
    return rc, (eng.lib.cpi_last_error(eng.ctx) or b"").decode()


@pytest.mark.parametrize("model,avg", MODES)
def test_bit_rules(eng, model, avg):
    name, layout = "n13", "ragged"
    W, N = CASES[name]
    qw, qt, idx, _ = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    r = _np(rows)
    stepped = _stepped(name, layout, qw, qt, idx)
    assert (~stepped & (idx > 0)).sum() >= 40 and (~stepped & (idx == 0)).sum() >= 3 * W and stepped.sum() >= 40
    out = {}
    for form in ("P", "P_sym"):
        out[form] = o = _query(eng, args, _source(rows, form), qw, qt)
        S = _base(r, form, qw, idx)
        # no step: S and its upper triangle, bit for bit; i == 0: all +0
        assert _bits(o["P"][~stepped], S[~stepped]) and _bits(o["P_sym"][~stepped], _tri(S[~stepped])), form
        zero = ~stepped & (idx == 0)
        assert not o["P"][zero].view(np.uint64).any() and not o["P_sym"][zero].view(np.uint64).any(), form
        assert _bits(o["P_sym"], _tri(o["P"])), form
        assert np.isfinite(o["P"]).all() and (np.abs(o["P"][stepped] - S[stepped]).max(axis=1) > 0).all(), form
        # a permutation of the queries permutes the outputs
        perm = np.random.default_rng(8).permutation(len(qw))
        o_p = _query(eng, args, _source(rows, form), qw[perm], qt[perm])
        assert _bits(o_p["P"], o["P"][perm]) and _bits(o_p["P_sym"], o["P_sym"][perm]), form
        # a NaN time: NaN in all 225 / 120 entries of that query, its neighbours untouched
        qt_nan = qt.copy()
        holes = [0, 3, 4, len(qt) - 1]
        qt_nan[holes] = np.nan
        o_n = _query(eng, args, _source(rows, form), qw, qt_nan)
        keep = np.ones(len(qt), dtype=bool)
        keep[holes] = False
        for f in ("P", "P_sym"):
            assert np.isnan(o_n[f][holes]).all() and _bits(o_n[f][keep], o[f][keep]), (form, f)
        # each output on its own
        assert _bits(_query(eng, args, _source(rows, form), qw, qt, want=("cov",))["P"], o["P"]), form
        assert _bits(_query(eng, args, _source(rows, form), qw, qt, want=("cov_sym",))["P_sym"], o["P_sym"]), form
    # rows that hold both forms are read as P
    assert _bits(_query(eng, args, {k: rows[k] for k in ("q", "P", "P_sym")}, qw, qt)["P"], out["P"]["P"])

    # the mean and Jacobian fields beside P are cpi_query_batch's, bit for bit; so is a call without P / P_sym
    groups = ("mean", "jac") if model == 1 else ("mean",)
    fields = MEAN + (JAC if model == 1 else ())
    mean_rows = {k: rows[k] for k in fields}
    plain = _query(eng, args, mean_rows, qw, qt, want=groups)
    both = _query(eng, args, dict(mean_rows, P_sym=rows["P_sym"]), qw, qt, want=groups + ("cov",))
    assert _bits(both["P"], out["P_sym"]["P"])
    for f in fields:
        assert _bits(both[f], plain[f]), f
    o = eng.alloc_outputs(len(qw), groups, model)
    for v in o.values():
        v.fill_(-7.0)
    rc, msg = _raw_call(eng, "cpi_query_cov_batch", args, mean_rows, _dev(qw, eng), _dev(qt, eng), o)
    assert rc == 0, msg
    for f in fields:
        assert _bits(o[f].cpu().numpy(), plain[f]), f


def test_zero_intervals_give_zeros_without_reading_rows(eng):
    """N == 0: every query gets the zero matrix (a NaN time NaN) and rows is not read -- an empty struct is passed."""
    for model in (1, 2):
        kn, lin, q = (t.to(eng.device) for t in synth.make_windows(4, 3, seed=77, edge_cases=False))
        args = dict(knots=kn[:, :1].contiguous(), lin=lin, q_k_lin=q, params=eng.make_params(model), first=None, count=None, N=None)
        qw = torch.tensor([0, 3, 1, 2, 2, 0], dtype=torch.int32, device=eng.device)
        qt = (kn[[0, 3, 1, 2, 2, 0], [1, 2, 0, 3, 1, 2], 0] + 0.002).contiguous()
        qt[4] = float("nan")
        out = eng.alloc_outputs(6, ("cov", "cov_sym"), model)
        for v in out.values():
            v.fill_(-7.0)
        rc, msg = _raw_call(eng, "cpi_query_cov_batch", args, {}, qw, qt, out, N=0)
        assert rc == 0, msg
        keep = np.arange(6) != 4
        for f, v in _np(out).items():
            assert not v[keep].view(np.uint64).any() and np.isnan(v[4]).all(), f


# ------------------------------------------------------------------------------------------------ 3. model-2 structure
@pytest.mark.parametrize("avg", [0, 1])
def test_model2_steps_from_a_row_with_theta_covariance(eng, avg):
    """Model 2 carries 18 rows and columns: the theta clone (rows / columns 15..17) is rebuilt from the 15 x 15 row.  Queries that
    step from a row i - 1 >= 1 whose theta rows and columns are non-zero, against the oracle: with the extension left out the
    g_tau x x_clone term of the v rows is lost (profiles/query_cov_bench.md)."""
    name, layout, model = "tumbling", "dense", 2
    qw, qt, idx, ref = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    sel = _stepped(name, layout, qw, qt, idx) & (idx >= 2)
    assert sel.sum() >= 100
    for form in ("P", "P_sym"):
        S = _base(_np(rows), form, qw[sel], idx[sel]).reshape(-1, 15, 15)
        assert (np.abs(S[:, :3, :]).max(axis=(1, 2)) > 0).all() and (np.abs(S[:, 6:9, :3]).max(axis=(1, 2)) > 0).all()
        out = _query(eng, args, _source(rows, form), qw[sel], qt[sel])
        e = cov_rel_err(out["P"], ref["P"][sel])
        print("model 2 avg %d, %d steps from rows with theta covariance (%s rows): cov_rel_err %.3e" % (avg, sel.sum(), form, e))
        assert e <= _gate(model)


# ------------------------------------------------------------------------------------------------ 4. contract
class _Call:
    """Valid arguments of cpi_query_cov_batch on 4 windows of 3 intervals; call(**changes) returns (code, message)."""
    W, N, Q = 4, 3, 6

    def __init__(self, eng, model=1):
        kn, lin, q = (t.to(eng.device) for t in synth.make_windows(self.W, self.N, seed=77, edge_cases=False))
        self.eng, self.prm = eng, eng.make_params(model)
        self.t = dict(knots=kn, lin=lin, q=q, qwin=torch.tensor([0, 3, 1, 2, 2, 0], dtype=torch.int32, device=eng.device),
                      qtime=(kn[[0, 3, 1, 2, 2, 0], [1, 2, 0, 3, 1, 2], 0] + 0.002).contiguous())
        self.rows = eng.preintegrate_running(kn, lin, q, self.prm, want=("mean", "cov", "cov_sym"))
        self.out = eng.alloc_outputs(self.Q, ("mean", "cov", "cov_sym"), model)
        for v in self.out.values():
            v.fill_(-7.0)
        self.ro, self.oo = eng._outputs_struct(self.rows), eng._outputs_struct(self.out)

    def __call__(self, **ch):
        a = dict(prm=C.byref(self.prm), W=self.W, N=self.N, knots=self.t["knots"].data_ptr(), first=None, count=None,
                 lin=self.t["lin"].data_ptr(), q=self.t["q"].data_ptr(), rows=C.byref(self.ro), Q=self.Q, qwin=self.t["qwin"].data_ptr(),
                 qtime=self.t["qtime"].data_ptr(), out=C.byref(self.oo))
        a.update(ch)
        rc = self.eng.lib.cpi_query_cov_batch(self.eng.ctx, a["prm"], a["W"], a["N"], a["knots"], a["first"], a["count"], a["lin"], a["q"],
                                              a["rows"], a["Q"], a["qwin"], a["qtime"], a["out"])
        return rc, (self.eng.lib.cpi_last_error(self.eng.ctx) or b"").decode()

    def without(self, d, *names):
        return C.byref(self.eng._outputs_struct({k: v for k, v in d.items() if k not in names}))


def test_refusals(eng):
    c = _Call(eng)
    assert c()[0] == 0
    torch.cuda.synchronize()
    assert not any((v == -7.0).any() for v in c.out.values())

    def refused(text, who="cpi_query_cov_batch: ", **ch):
        rc, msg = c(**ch)
        assert rc == 1 and msg.startswith(who) and text in msg, (rc, msg)

    cov_only = {k: c.out[k] for k in ("P", "P_sym")}
    refused("rows needs q", rows=c.without(c.rows, "q"), out=C.byref(eng._outputs_struct(cov_only)))
    refused("rows needs DT, alpha, beta and q", rows=c.without(c.rows, "q"))
    refused("rows needs DT, alpha, beta and q", rows=c.without(c.rows, "DT"))
    assert c(rows=c.without(c.rows, "DT", "alpha", "beta"), out=C.byref(eng._outputs_struct(cov_only)))[0] == 0   # the covariance needs q only
    for f in ("P", "P_sym"):
        refused("rows needs P or P_sym", rows=c.without(c.rows, "P", "P_sym"), out=c.without(c.out, "P" if f == "P_sym" else "P_sym"))
        assert c(rows=c.without(c.rows, f))[0] == 0                                                           # either form serves
    assert c(rows=c.without(c.rows, "P", "P_sym"), out=c.without(c.out, "P", "P_sym"))[0] == 0                # cpi_query_batch's request
    J = torch.zeros((c.Q, 9), dtype=torch.float64, device=eng.device)
    for f in JAC + ("O_a", "O_b"):
        refused("not available for model 2", prm=C.byref(eng.make_params(2)), out=C.byref(eng._outputs_struct(dict(c.out, **{f: J}))))
    refused("a Jacobian field of out needs the same field of rows", out=C.byref(eng._outputs_struct(dict(c.out, J_a=J))))
    refused("model must be 1 or 2 (the Forster comparator", prm=C.byref(eng.make_params(3)))
    refused("model must be 1 or 2", prm=C.byref(eng.make_params(4)))
    refused("model 2 needs q_k_lin", prm=C.byref(eng.make_params(2)), q=None)
    for name in ("prm", "rows", "out"):
        refused("prm/rows/out is NULL", **{name: None})
    for name in ("qwin", "qtime"):
        refused("qwin/qtime is NULL", **{name: None})
    for name in ("knots", "lin"):
        refused("knots/lin is NULL", **{name: None})
    for name in ("W", "N", "Q"):
        refused("negative size", **{name: -1})
    refused("W is 0", W=0)
    refused("N (intervals per window) must be <= 65535", N=65536)
    refused("Q exceeds 2^31 - 1", Q=2 ** 31)
    assert eng.lib.cpi_query_cov_batch(None, C.byref(c.prm), 1, 1, None, None, None, None, None, C.byref(c.ro), 1, None, None, C.byref(c.oo)) == 1
    # Q == 0 writes nothing, whatever else is passed
    c = _Call(eng, 2)
    for ch in (dict(Q=0), dict(Q=0, W=0), dict(Q=0, qwin=None, qtime=None, knots=None)):
        assert c(**ch)[0] == 0
    torch.cuda.synchronize()
    assert all((v == -7.0).all() for v in c.out.values())
    # the old entry still refuses the covariance, with its own text
    rc = eng.lib.cpi_query_batch(eng.ctx, C.byref(c.prm), c.W, c.N, c.t["knots"].data_ptr(), None, None, c.t["lin"].data_ptr(), c.t["q"].data_ptr(),
                                 C.byref(c.ro), c.Q, c.t["qwin"].data_ptr(), c.t["qtime"].data_ptr(), C.byref(c.oo))
    assert rc == 1 and (eng.lib.cpi_last_error(eng.ctx) or b"").decode().startswith("cpi_query_batch: P / P_sym are not available at query times")


def test_window_index_is_clamped_on_the_device(eng):
    name, model, avg = "n13", 2, 0
    kn = _case(name)[0]
    W = CASES[name][0]
    args, rows = _rows(eng, name, "dense", model, avg)
    qt = kn[[0, 0, W - 1, W - 1], [3, 3, 5, 5], 0] + 0.001
    wild = _query(eng, args, _source(rows, "P_sym"), np.array([-5, 0, 99, W - 1], dtype=np.int32), qt)
    for f in ("P", "P_sym"):
        assert _bits(wild[f][0], wild[f][1]) and _bits(wild[f][2], wild[f][3]) and np.abs(wild[f]).max() > 0, f


# ------------------------------------------------------------------------------------------------ 5. host form
@pytest.mark.parametrize("model,avg", [(1, 1), (2, 0)])
def test_host_form(eng, model, avg):
    """cpi_query_cov_batch_host: the bits of the device form on rows that hold P_sym (what it stages), and the validation of
    cpi_query_batch_host under its own name."""
    from cpi_amd import CpiError
    name = "n13"
    kn, lin, q, cnt = _case(name)
    W = CASES[name][0]
    qw, qt = _queries(kn, cnt)
    prm = eng.make_params(model, bool(avg))
    groups = ("mean", "jac") if model == 1 else ("mean",)
    rows = eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=groups + ("cov_sym",), count=_dev(cnt, eng))
    dev = _np(eng.query(_dev(kn, eng), _dev(lin, eng), rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=_dev(q, eng), params=prm,
                        want=groups + ("cov", "cov_sym"), count=_dev(cnt, eng)))
    cpu = [torch.from_numpy(x) for x in (kn, lin)]
    host = eng.query_host(*cpu, torch.from_numpy(qw), torch.from_numpy(qt), q_k_lin=torch.from_numpy(q), params=prm,
                          want=groups + ("cov", "cov_sym"), count=torch.from_numpy(cnt))
    assert set(host) == set(dev) and {"P", "P_sym"} <= set(host)
    for f in dev:
        assert _bits(host[f].numpy(), dev[f]), f
    only = eng.query_host(*cpu, torch.from_numpy(qw), torch.from_numpy(qt), q_k_lin=torch.from_numpy(q), params=prm, want=("cov_sym",),
                          count=torch.from_numpy(cnt))
    rows = eng.preintegrate_running(_dev(kn, eng), _dev(lin, eng), _dev(q, eng), prm, want=("mean", "cov_sym"), count=_dev(cnt, eng))   # as staged
    dev = _np(eng.query(_dev(kn, eng), _dev(lin, eng), rows, _dev(qw, eng), _dev(qt, eng), q_k_lin=_dev(q, eng), params=prm, want=("cov_sym",),
                        count=_dev(cnt, eng)))
    assert list(only) == ["P_sym"] and _bits(only["P_sym"].numpy(), dev["P_sym"])
    two = torch.from_numpy(qt[:2].copy())
    for bad in (-1, W):
        with pytest.raises(CpiError, match=r"cpi_query_cov_batch_host: qwin\[1\] = %d is not a window" % bad) as e:
            eng.query_host(*cpu, torch.tensor([0, bad], dtype=torch.int32), two, q_k_lin=torch.from_numpy(q), params=prm, want=("cov",))
        assert e.value.code == 1
    broken = kn.copy()
    broken[3, 5, 0] = broken[3, 4, 0] - 1.0
    with pytest.raises(CpiError, match="cpi_query_cov_batch_host: window 3 has a NaN, infinite or decreasing stamp at knot 5") as e:
        eng.query_host(torch.from_numpy(broken), cpu[1], torch.tensor([0, 3], dtype=torch.int32), two, q_k_lin=torch.from_numpy(q), params=prm,
                       want=("cov",))
    assert e.value.code == 1
    ok = eng.query_host(torch.from_numpy(broken), cpu[1], torch.tensor([0, 1], dtype=torch.int32), two, q_k_lin=torch.from_numpy(q),
                        params=prm, want=("cov",))                    # a window nobody queries may hold what it likes
    assert np.isfinite(ok["P"].numpy()).all()


# ------------------------------------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("model,avg", MODES)
def test_sqrt_information_at_query_times(eng, model, avg):
    """P_sym at the query times -> cpi_sqrt_information_packed_batch: the whitening of a keyframe factor stamped inside an interval,
    against the longdouble factorisation of the oracle's P.  Every query whose cut window has a positive length (the zero matrix of
    an empty window has no factorisation)."""
    name, layout = "n13", "dense"
    qw, qt, idx, ref = _reference(name, layout, model, avg)
    args, rows = _rows(eng, name, layout, model, avg)
    sel = (idx > 0) | _stepped(name, layout, qw, qt, idx)
    assert sel.sum() >= 150
    P_sym = eng.query(args["knots"], args["lin"], _source(rows, "P_sym"), _dev(qw[sel], eng), _dev(qt[sel], eng), q_k_lin=args["q_k_lin"],
                      params=args["params"], want=("cov_sym",))["P_sym"]
    R_tri = eng.sqrt_information(P_sym)
    torch.cuda.synchronize()
    R = np.zeros((int(sel.sum()), 225))
    R[:, _TRI] = R_tri.cpu().numpy()
    R = R.reshape(-1, 15, 15).transpose(0, 2, 1)                                 # [row][col], upper triangular
    assert np.isfinite(R).all()
    Pref = ref["P"][sel].reshape(-1, 15, 15).transpose(0, 2, 1)
    Rref = sqrt_info_longdouble(Pref)
    rel = float((np.abs(R - Rref).max(axis=(1, 2)) / np.abs(Rref).max(axis=(1, 2))).max())
    A = np.array(R, dtype=np.longdouble)
    ident = float(np.abs(np.asarray(A.transpose(0, 2, 1) @ A @ np.array(Pref, dtype=np.longdouble) - np.eye(15), dtype=np.float64)).max())
    row = float(e_row(R, Rref).max())                                            # row by row: rel sees the largest rows of R only
    print("sqrt information at query times model %d avg %d (%d factors): |R - R_ref| / max |R_ref| %.3e, row-wise %.3e, |R^T R P - I| %.3e"
          % (model, avg, sel.sum(), rel, row, ident))
    assert ident <= 1e-6 and rel <= 100.0 * FLOOR_SQRT
    assert row < REG_SQRT_INFO_ROW


# ------------------------------------------------------------------------------------------------ 7. graph
def test_running_then_query_cov_replays_from_a_graph(eng):
    """One capture of cpi_preintegrate_running (means + covariance) followed by cpi_query_cov_batch -- a chain without parallel
    branches -- replays to the bits of the eager calls, also on new measurements in the same buffers."""
    for model in (1, 2):
        kn, lin, q, cnt = (_dev(x, eng) for x in _case("tumbling"))
        qw_h, qt_h = _queries(_case("tumbling")[0], _case("tumbling")[3])
        qw, qt = _dev(qw_h, eng), _dev(qt_h, eng)
        prm = eng.make_params(model, True)
        want_r, want_q = ("mean", "cov_sym"), ("mean", "cov", "cov_sym")
        rows = eng.preintegrate_running(kn, lin, q, prm, want=want_r, count=cnt)
        out = eng.query(kn, lin, rows, qw, qt, q_k_lin=q, params=prm, want=want_q, count=cnt)

        def call():
            eng.preintegrate_running(kn, lin, q, prm, want=want_r, count=cnt, out=rows)
            eng.query(kn, lin, rows, qw, qt, q_k_lin=q, params=prm, want=want_q, count=cnt, out=out)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            call()                                          # warm-up on the side stream, as graph capture requires
        torch.cuda.synchronize()
        eager = {k: v.clone() for k, v in out.items()}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for v in list(out.values()) + list(rows.values()):
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], eager[k]), k
        kn[:, :, 1:4] *= 1.01                               # new measurements in the same buffers
        g.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        call()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], replayed[k]), k
        assert not torch.equal(out["P"], eager["P"])


# ------------------------------------------------------------------------------------------------ 8. C++ facade
@pytest.mark.parametrize("model", [1, 2])
def test_query_cov_cpp_facade(eng, model):
    """tests/cpp/test_query_cov.cpp: cpi_host::CpiBatch::at_cov against libcpi_amd.so; the program checks itself (P_meas on a stamp
    is running()'s bit for bit, P_meas inside an interval matches a window of its own, at() still leaves P_meas alone)."""
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    W, N = 6, 9
    kn, lin, q = (t.numpy() for t in synth.make_windows(W, N, seed=31, edge_cases=False))
    count = [9, 1, 4, 9, 6, 2]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_query_cov")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_query_cov.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        with open(os.path.join(tmp, "win.txt"), "w") as f:
            f.write("%d\n" % W)
            for w in range(W):
                f.write("%d\n" % count[w])
                f.write(" ".join("%.17g" % v for v in [*lin[w], *q[w]]) + "\n")
                for s in range(count[w] + 1):
                    f.write(" ".join("%.17g" % v for v in kn[w, s]) + "\n")
        for avg in (0, 1):
            p = subprocess.run([exe, os.path.join(tmp, "win.txt"), str(model), str(avg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            print(p.stdout.strip())
            assert p.stdout.splitlines()[-1] == "test_query_cov ok"
