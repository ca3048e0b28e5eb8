"""GPU: the contract of the preintegration entries' HOST code (cpi_amd/csrc/cpi_abi.hip) that no other test pins.

(a) Ragged host staging.  The four _host entries that take first / n_knots (batch, running, resume, running_resume) stage ragged
    windows whole.  The Python wrappers always pass first = None, so the entries are called through ctypes here, on one shared
    stream of 13 knots with an empty window, two windows that share a start and windows that share knots.  Every field -- and the
    carry record -- must equal, bit for bit, what the device-pointer entry writes for the same arrays.  Of a record only the parts a
    full request writes are compared (test_gpu_running_resume._live): the rest is staging memory no kernel touches.

(b) The no-op / refusal boundary.  One table row per entry (the 18 cpi_preintegrate_* entries and the two producers of the tiled
    layout that take window sizes): the return code of the zero-size calls with NULL data pointers, and one refusal of each kind
    the entry has, by code and by message.  Outputs, carry records and workspaces are filled with a sentinel and must be untouched
    after every one of these calls.  The expected values are the ones the entries had BEFORE their checks were folded into shared
    code; every refused call is refused on the host, before any kernel launch (a _host entry may have uploaded its inputs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cpi_amd import synth
from cpi_amd._lib import CPI_ERR_INVALID, CPI_OK, OUT_FIELDS, CpiOutputs
from tests.test_gpu_running_resume import _live

pytestmark = pytest.mark.gpu
OK, INV = CPI_OK, CPI_ERR_INVALID
SENTINEL = -7.25
CD_MAX = 566                                    # doubles of the larger carry record (model 2)


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return cpi_amd.Engine()


def _p(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


def _outputs(fields, rows, device):
    bufs = {name: torch.full((rows, n), SENTINEL, dtype=torch.float64, device=device) for name, n in OUT_FIELDS if name in fields}
    o = CpiOutputs()
    for name, _ in OUT_FIELDS:
        setattr(o, name, bufs[name].data_ptr() if name in bufs else None)
    return o, bufs


def _last_error(eng):
    return (eng.lib.cpi_last_error(eng.ctx) or b"").decode()


# ------------------------------------------------------------------------------------------------ (a) ragged host staging
RAG_K, RAG_W, RAG_N = 13, 5, 4
RAG_FIRST = np.array([0, 2, 2, 6, 8], dtype=np.int64)
RAG_COUNT = np.array([0, 1, 4, 3, 2], dtype=np.int32)
MEANS = ("DT", "alpha", "beta", "q")
ALL_M1 = tuple(n for n, _ in OUT_FIELDS if n not in ("O_a", "O_b"))
ALL_M2 = tuple(n for n, _ in OUT_FIELDS)
RUN_M2 = MEANS + ("P", "P_sym")                 # model 2 has no running Jacobians


def _ragged_case():
    kn, _, _ = synth.make_windows(1, RAG_K - 1, seed=411, edge_cases=False)
    _, lin, q = synth.make_windows(RAG_W, RAG_N, seed=412, edge_cases=False)
    return {"knots": kn[0].contiguous(), "first": torch.from_numpy(RAG_FIRST), "count": torch.from_numpy(RAG_COUNT), "lin": lin, "q": q}


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("entry", ["batch", "running", "resume", "running_resume"])
def test_ragged_host_staging_matches_device_entry(eng, entry, model):
    running, carry = "running" in entry, "resume" in entry
    fields = (ALL_M1 if model == 1 else (RUN_M2 if running else ALL_M2))
    rows = RAG_W * (RAG_N if running else 1)
    cd = eng.carry_doubles(model)
    prm = eng.make_params(model)
    host = _ragged_case()
    dev = {k: v.to(eng.device) for k, v in host.items()}
    fn_d, fn_h = getattr(eng.lib, "cpi_preintegrate_" + entry), getattr(eng.lib, "cpi_preintegrate_%s_host" % entry)
    cin_d = cin_h = None
    for step in range(2 if carry else 1):       # resume entries: from the zero state (NULL record), then from the first call's record
        od, bd = _outputs(fields, rows, eng.device)
        oh, bh = _outputs(fields, rows, "cpu")
        cout_d = torch.full((RAG_W, cd), SENTINEL, dtype=torch.float64, device=eng.device) if carry else None
        cout_h = torch.full((RAG_W, cd), SENTINEL, dtype=torch.float64) if carry else None
        head = (eng.ctx, C.byref(prm), RAG_W, RAG_N)
        cd_args = (_p(cin_d), _p(cout_d)) if carry else ()
        ch_args = (_p(cin_h), _p(cout_h)) if carry else ()
        rc = fn_d(*head, _p(dev["knots"]), _p(dev["first"]), _p(dev["count"]), _p(dev["lin"]), _p(dev["q"]), *cd_args, C.byref(od))
        assert rc == OK, _last_error(eng)
        rc = fn_h(*head, _p(host["knots"]), _p(host["first"]), _p(host["count"]), RAG_K, _p(host["lin"]), _p(host["q"]), *ch_args, C.byref(oh))
        assert rc == OK, _last_error(eng)
        torch.cuda.synchronize()
        for name in fields:
            got, want = bh[name].numpy(), bd[name].cpu().numpy()
            assert not np.any(want == SENTINEL), "%s: the device entry left rows of %s unwritten" % (entry, name)
            assert np.array_equal(got, want), "%s model %d step %d: %s differs between the host and the device entry" % (entry, model, step, name)
        if carry:
            for sl in _live(model):
                assert np.array_equal(cout_h.numpy()[:, sl], cout_d.cpu().numpy()[:, sl]), "%s model %d step %d: carry record" % (entry, model, step)
            cin_d, cin_h = cout_d, cout_h


# ------------------------------------------------------------------------------------------------ (b) no-op / refusal boundary
W, N, K, U, R = 3, 4, 16, 3, 3

BATCH = "ctx prm W N knots first count lin q out"
BATCH_H = "ctx prm W N knots first count nk lin q out"
CARRY = "ctx prm W N knots first count lin q cin cout out"
CARRY_H = "ctx prm W N knots first count nk lin q cin cout out"
STREAM = "ctx prm K stream W upd N lin q ws out"
STREAM_H = "ctx prm K stream W upd N lin q out cnt"
STREAMS = "ctx prm R K stream soff W upd uoff N lin q ws out"
STREAMS_H = "ctx prm R K stream soff W upd uoff N lin q out cnt"
TILED = "ctx prm W N tiles count lin q out"

FORSTER_RUN = "model must be 1 or 2 (the Forster comparator has no running form)"
FORSTER_RES = "model must be 1 or 2 (the Forster comparator cannot be resumed)"
FORSTER_RR = "model must be 1 or 2 (the Forster comparator has no running form and cannot be resumed)"
JAC_DEV = "the Jacobian fields (J_q ... O_b) are not available for model 2 (they are read out of the state transition matrix at the end of the recursion)"
JAC_HOST = "the Jacobian fields (J_q ... O_b) are not available for model 2"
LANES = "lanes_per_window must be 0 or one of 1,2,3,4,5,6,8,12,16,32,64"
TILED_ONLY = "the tiled layout serves the mean outputs (DT, alpha, beta, q) only"


def _row(sig, zero, n0=None, zero_data=None, null_prm=None, running=False, **refusals):
    """zero: code of W == 0 / U == 0 with NULL data pointers; zero_data: the same call with data, where NULL data is what is
    refused; n0: code of N == 0 with NULL data (None: the entry has no rule for it); null_prm: code of the zero-size call
    with a NULL prm as well; refusals: kind -> message (the entry's name and ": " are prepended unless it starts with "=")."""
    return dict(sig=sig, zero=zero, n0=n0, zero_data=zero_data, null_prm=null_prm, running=running, refusals=refusals)


# a message that starts with "=" is compared as it stands: it names the device-pointer entry the _host entry forwards to, or
# no entry at all
ENTRIES = {
    "cpi_preintegrate_batch": _row(BATCH, OK, null_prm=INV, no_q="model 2 needs q_k_lin", lanes7="=" + LANES),
    "cpi_preintegrate_resume": _row(CARRY, OK, null_prm=INV, forster=FORSTER_RES, no_q="model 2 needs q_k_lin", lanes7="=" + LANES,
                                    overlap="carry_in and carry_out overlap"),
    "cpi_preintegrate_running": _row(BATCH, OK, n0=OK, null_prm=INV, running=True, forster=FORSTER_RUN, jac2=JAC_DEV,
                                     no_q="model 2 needs q_k_lin", lanes7="=" + LANES),
    "cpi_preintegrate_running_resume": _row(CARRY, OK, n0=INV, null_prm=INV, running=True, forster=FORSTER_RR,
                                            jac2=JAC_DEV[:-1] + ": finish the chain with cpi_preintegrate_resume)",
                                            no_q="model 2 needs q_k_lin", lanes7="=" + LANES, overlap="carry_in and carry_out overlap"),
    "cpi_preintegrate_stream": _row(STREAM, OK, null_prm=OK, no_q="model 2 needs q_k_lin", lanes7="=" + LANES,
                                    misaligned="the workspace must be 16-byte aligned"),
    "cpi_preintegrate_streams": _row(STREAMS, OK, null_prm=OK, no_q="model 2 needs q_k_lin", lanes7="=" + LANES,
                                     misaligned="the workspace must be 16-byte aligned"),
    "cpi_preintegrate_stream_running": _row(STREAM, OK, n0=OK, null_prm=INV, running=True, forster=FORSTER_RUN, jac2=JAC_DEV,
                                            no_q="model 2 needs q_k_lin", lanes7="=" + LANES, misaligned="the workspace must be 16-byte aligned"),
    "cpi_preintegrate_streams_running": _row(STREAMS, OK, n0=OK, null_prm=INV, running=True, forster=FORSTER_RUN, jac2=JAC_DEV,
                                             no_q="model 2 needs q_k_lin", lanes7="=" + LANES, misaligned="the workspace must be 16-byte aligned"),
    "cpi_preintegrate_tiled_batch": _row(TILED, OK, null_prm=INV, forster="model must be 1 or 2", no_q="model 2 needs q_k_lin",
                                         not_mean=TILED_ONLY + "; Jacobians and covariance are FP64-bound, not HBM-bound: use cpi_preintegrate_batch",
                                         lanes9="lanes_per_window (here: wavefronts per tile) must be 0 (auto) or 1..8"),
    "cpi_preintegrate_batch_host": _row(BATCH_H, INV, zero_data=OK, null_prm=INV, no_q="=cpi_preintegrate_batch: model 2 needs q_k_lin",
                                        lanes7="=" + LANES),
    "cpi_preintegrate_resume_host": _row(CARRY_H, INV, zero_data=OK, null_prm=INV, forster=FORSTER_RES,
                                         no_q="=cpi_preintegrate_resume: model 2 needs q_k_lin", lanes7="=" + LANES,
                                         overlap="carry_in and carry_out overlap"),
    "cpi_preintegrate_running_host": _row(BATCH_H, INV, n0=INV, zero_data=OK, null_prm=INV, running=True, forster=FORSTER_RUN, jac2=JAC_HOST,
                                          no_q="=cpi_preintegrate_running: model 2 needs q_k_lin", lanes7="=" + LANES),
    "cpi_preintegrate_running_resume_host": _row(CARRY_H, INV, n0=INV, zero_data=OK, null_prm=INV, running=True, forster=FORSTER_RR, jac2=JAC_HOST,
                                                 no_q="=cpi_preintegrate_running_resume: model 2 needs q_k_lin", lanes7="=" + LANES,
                                                 overlap="carry_in and carry_out overlap"),
    "cpi_preintegrate_stream_host": _row(STREAM_H, OK, null_prm=OK, no_q="model 2 needs q_k_lin", lanes7="=" + LANES),
    "cpi_preintegrate_streams_host": _row(STREAMS_H, OK, null_prm=OK, no_q="model 2 needs q_k_lin", lanes7="=" + LANES,
                                          decreasing="stream_offsets decrease at run 1"),
    "cpi_preintegrate_stream_running_host": _row(STREAM_H, OK, n0=OK, null_prm=INV, running=True, forster=FORSTER_RUN, jac2=JAC_DEV,
                                                 no_q="model 2 needs q_k_lin", lanes7="=" + LANES),
    "cpi_preintegrate_streams_running_host": _row(STREAMS_H, OK, n0=OK, null_prm=INV, running=True, forster=FORSTER_RUN, jac2=JAC_DEV,
                                                  no_q="model 2 needs q_k_lin", lanes7="=" + LANES, decreasing="stream_offsets decrease at run 1"),
    "cpi_preintegrate_tiled_batch_host": _row(TILED, INV, zero_data=OK, null_prm=INV, forster="=cpi_preintegrate_tiled_batch: model must be 1 or 2",
                                              no_q="=cpi_preintegrate_tiled_batch: model 2 needs q_k_lin", not_mean=TILED_ONLY,
                                              lanes9="=cpi_preintegrate_tiled_batch: lanes_per_window (here: wavefronts per tile) must be 0 (auto) or 1..8"),
    "cpi_tile_windows": _row("ctx W N knots first count tiles_out", OK),
    "cpi_assemble_tiles": _row("ctx K stream W upd N tiles_out cnt_out", OK),
}
DATA_KEYS = ("knots", "first", "count", "lin", "q", "cin", "stream", "upd", "soff", "uoff", "tiles")


def test_table_covers_every_preintegration_entry():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpi_amd.h")).read()
    assert set(re.findall(r"\bint (cpi_preintegrate_\w+)\(", header)) == {n for n in ENTRIES if n.startswith("cpi_preintegrate_")}
    assert len(ENTRIES) == 20


class _World:
    """Valid, correctly sized arguments of every entry in device or host memory; outputs, records and workspace hold SENTINEL."""

    def __init__(self, eng, device, running, fields):
        f64 = dict(dtype=torch.float64, device=device)
        self.eng, self.device = eng, device
        t = torch.arange(K, **f64) * 0.005 + 100.0
        stream = torch.zeros((K, 7), **f64)
        stream[:, 0] = t
        stream[:, 6] = 9.8
        q = torch.zeros((W, 4), **f64)
        q[:, 3] = 1.0
        self.data = {
            "knots": stream[:W * (N + 1)].reshape(W, N + 1, 7).contiguous(), "first": None, "count": None,
            "lin": torch.zeros((W, 6), **f64), "q": q, "cin": None, "stream": stream,
            "upd": (t[[5, 10, 15]] + 0.001).contiguous(),
            "soff": torch.tensor([0, 5, 10, K], dtype=torch.int64, device=device),
            "uoff": torch.tensor([0, 1, 2, U], dtype=torch.int64, device=device),
            "tiles": torch.zeros((1, N + 1, 7, 64), **f64),
        }
        rows = W * N if running else W
        self.out_struct, self.out = _outputs(fields, rows, device)
        self.guarded = dict(self.out)
        self.guarded["cout"] = torch.full((W, CD_MAX), SENTINEL, **f64)
        self.guarded["cin"] = torch.full((W, CD_MAX), SENTINEL, **f64)   # only the overlap case passes it
        self.guarded["ws"] = torch.full((eng.lib.cpi_stream_workspace_bytes(U) // 8 + 2,), SENTINEL, **f64)
        self.guarded["tiles_out"] = torch.full((1, N + 1, 7, 64), SENTINEL, **f64)
        self.guarded["cnt"] = torch.full((U,), -77, dtype=torch.int32, device=device)

    def args(self, sig, prm, **over):
        """The ctypes argument list of `sig`; over: replacements by key (a tensor, None, an integer or a ready ctypes value)."""
        vals = dict(self.data)
        vals.update(W=W, N=N, K=K, R=R, nk=0, ctx=self.eng.ctx, prm=prm, out=self.out_struct, cout=self.guarded["cout"],
                    ws=self.guarded["ws"], tiles_out=self.guarded["tiles_out"], cnt=self.guarded["cnt"], cnt_out=self.guarded["cnt"])
        vals.update(over)
        a = []
        for key in sig.split():
            v = vals[key]
            if key == "prm" or key == "out":
                v = None if v is None else C.byref(v)
            elif torch.is_tensor(v):
                v = _p(v)
            a.append(v)
        return a

    def assert_untouched(self, what):
        torch.cuda.synchronize()
        for name, t in self.guarded.items():
            assert bool((t == (-77 if name == "cnt" else SENTINEL)).all()), "%s wrote %s" % (what, name)


def _with_jac(world):
    o, bufs = _outputs(MEANS + ("J_q",), world.out["DT"].shape[0], world.device)
    world.guarded.update({"J_q": bufs["J_q"], "DT2": bufs["DT"], "alpha2": bufs["alpha"], "beta2": bufs["beta"], "q2": bufs["q"]})
    return o


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_noop_and_refusal_boundary(eng, name):
    row = ENTRIES[name]
    fn = getattr(eng.lib, name)
    fn.restype = C.c_int
    host = name.endswith("_host")
    sig = row["sig"]
    world = _World(eng, "cpu" if host else eng.device, row["running"], MEANS if sig == TILED else MEANS + ("P",))   # the tiled entries serve means only
    no_data = {k: None for k in DATA_KEYS}
    prm1 = eng.make_params(1)

    def call(expect, what, prm=prm1, **over):
        rc = fn(*world.args(sig, prm, **over))
        assert rc == expect, "%s, %s: returned %d, expected %d (%s)" % (name, what, rc, expect, _last_error(eng))
        world.assert_untouched("%s, %s" % (name, what))

    # ---- zero-size calls
    call(row["zero"], "W == 0 / U == 0 with NULL data", W=0, **no_data)
    if row["zero_data"] is not None:
        call(row["zero_data"], "W == 0 with data", W=0)
    if row["n0"] is not None:
        call(row["n0"], "N == 0 with NULL data", N=0, **no_data)
    if row["null_prm"] is not None:
        call(row["null_prm"], "W == 0 / U == 0 with NULL data and a NULL prm", prm=None, W=0, **no_data)

    # ---- one refusal of each kind the entry has
    def refuse(kind, prm=prm1, **over):
        text = row["refusals"][kind]
        text = text[1:] if text.startswith("=") else name + ": " + text
        call(INV, kind, prm=prm, **over)
        assert _last_error(eng) == text, "%s, %s: message" % (name, kind)

    kinds = set(row["refusals"])
    if "forster" in kinds:
        refuse("forster", prm=eng.make_params(3))
    if "jac2" in kinds:
        refuse("jac2", prm=eng.make_params(2), out=_with_jac(world))
    if "not_mean" in kinds:
        refuse("not_mean", out=_with_jac(world))
    if "no_q" in kinds:
        refuse("no_q", prm=eng.make_params(2), q=None)
    if "lanes7" in kinds:
        refuse("lanes7", prm=eng.make_params(1, lanes_per_window=7))
    if "lanes9" in kinds:
        refuse("lanes9", prm=eng.make_params(1, lanes_per_window=9))
    if "overlap" in kinds:
        refuse("overlap", cin=world.guarded["cin"], cout=world.guarded["cin"])
    if "misaligned" in kinds:
        refuse("misaligned", ws=_p(world.guarded["ws"], 8))
    if "decreasing" in kinds:
        refuse("decreasing", soff=torch.tensor([0, 8, 5, K], dtype=torch.int64))
    assert kinds <= {"forster", "jac2", "not_mean", "no_q", "lanes7", "lanes9", "overlap", "misaligned", "decreasing"}
