"""Host-side mirror of the reference's preintegrator / factor interface over the C-ABI.

    Engine                 one (device, stream) context; batched device-resident entry points
    CpiV1 / CpiV2          same constructor, setLinearizationPoints(), feed_IMU() and public result
                           fields as the reference classes (cpi_compare/src/cpi/CpiBase.h:40-145,
                           CpiV1.h:62, CpiV2.h:84); the recursion runs on the GPU when a result is read
    ImuFactorCPIv1 / v2    constructor argument order of ImuFactorCPIv1.h:78-81 / ImuFactorCPIv2.h:82-85
                           and evaluateError(state_i, state_j) -> (error, H1, H2)

PyTorch is used for device memory and streams only.
"""
import ctypes as C
from ctypes import byref

import numpy as np
import torch

from . import _lib
from ._lib import OUT_FIELDS, CpiError, CpiLmParams, CpiOutputs, CpiParams

DEFAULT_SIGMAS = (0.005, 4e-6, 0.01, 2e-4)   # ADIS16448, cpi_compare/launch/synthetic_test.launch:13-17
DEFAULT_GRAV = (0.0, 0.0, 9.8)
MEAN_FIELDS = ("DT", "alpha", "beta", "q")
JAC_FIELDS = ("J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b")


def _group_of(name):
    """want-group of an output field: "mean", "jac", "cov" (P, dense 15 x 15) or "cov_sym" (P_sym: its packed upper triangle, 120
    doubles -- include/cpi_amd.h CPI_TRI_INDEX)."""
    if name in MEAN_FIELDS:
        return "mean"
    return "cov" if name == "P" else ("cov_sym" if name == "P_sym" else "jac")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fields(d):
    """The tensors of an output dict: a packed one (alloc_outputs) without its "_flat" / "_fields" entries."""
    return {k: v for k, v in d.items() if not k.startswith("_")}


def _tri_index(device=None):
    """(rows, cols) of the packed upper triangle in storage order: entry k of a packed matrix is (rows[k], cols[k])."""
    cols = torch.repeat_interleave(torch.arange(15, device=device), torch.arange(1, 16, device=device))
    start = cols * (cols + 1) // 2
    rows = torch.arange(120, device=device) - start
    return rows, cols


def pack_sym(M):
    """Dense [F, 225] (column-major 15 x 15; symmetric or upper triangular) -> packed upper triangle [F, 120]
    (include/cpi_amd.h: entry (i, j), i <= j, at i + j (j + 1) / 2).  pack_tri is the same gather."""
    rows, cols = _tri_index(M.device)
    return M.reshape(-1, 225)[:, cols * 15 + rows].contiguous()


pack_tri = pack_sym


def unpack_sym(Ps):
    """Packed upper triangle [F, 120] of a SYMMETRIC matrix (cpi_outputs.P_sym) -> dense [F, 225], both halves filled."""
    rows, cols = _tri_index(Ps.device)
    M = torch.zeros((Ps.shape[0], 225), dtype=Ps.dtype, device=Ps.device)
    M[:, rows * 15 + cols] = Ps      # lower half (element (j, i) of the column-major matrix sits at i * 15 + j)
    M[:, cols * 15 + rows] = Ps
    return M


def unpack_tri(Rt):
    """Packed [F, 120] of an UPPER-TRIANGULAR matrix (R_tri of cpi_sqrt_information_packed_batch) -> dense [F, 225]
    column-major with zeros below the diagonal (what cpi_sqrt_information_batch writes)."""
    rows, cols = _tri_index(Rt.device)
    M = torch.zeros((Rt.shape[0], 225), dtype=Rt.dtype, device=Rt.device)
    M[:, cols * 15 + rows] = Rt
    return M


class _nullctx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


class Engine:
    """One C-ABI context.  stream=None: the engine FOLLOWS torch's current stream of its device -- every call is issued
    on torch.cuda.current_stream() as it is at that call (so inputs produced and outputs allocated under
    `with torch.cuda.stream(s):` are used on the stream that owns them).  An explicit stream pins the engine to it; the
    caller then orders that stream against the producers / consumers of the tensors (EnginePool does that bookkeeping)."""

    def __init__(self, device=None, stream=None):
        self.lib = _lib.load()
        self._follow = stream is None
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        ctx = C.c_void_p()
        if stream is None and torch.cuda.is_available():
            stream = torch.cuda.current_stream(self.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else None
        rc = self.lib.cpi_ctx_create(self.device.index or 0, sptr, C.byref(ctx))
        if rc != 0:
            raise CpiError(rc, (self.lib.cpi_last_error(None) or b"").decode())
        self.ctx = ctx
        self.stream = stream

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.cpi_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CpiError(rc, (self.lib.cpi_last_error(self.ctx) or b"").decode())

    def _sync_stream(self):
        """Follow torch's current stream (see the class docstring); one pointer comparison per call."""
        if self._follow:
            cur = torch.cuda.current_stream(self.device)
            if cur.cuda_stream != self.stream.cuda_stream:
                self._check(self.lib.cpi_ctx_set_stream(self.ctx, C.c_void_p(cur.cuda_stream)))
                self.stream = cur

    def synchronize(self):
        self._check(self.lib.cpi_ctx_synchronize(self.ctx))

    def set_capture_overlap(self, depth):
        """cpi_ctx_set_capture_overlap: how many captured, provably disjoint batch calls may be unordered in a HIP graph (1 = none)."""
        self._check(self.lib.cpi_ctx_set_capture_overlap(self.ctx, int(depth)))

    def set_capture_strands(self, n):
        """cpi_ctx_set_capture_strands: captured, provably disjoint batch calls form n chains in a HIP graph (1 = one chain, the serial order)."""
        self._check(self.lib.cpi_ctx_set_capture_strands(self.ctx, int(n)))

    # ------------------------------------------------------------------ preintegration
    @staticmethod
    def make_params(model=1, imu_avg=False, state_transition_jacobians=True, sigmas=DEFAULT_SIGMAS,
                    grav=DEFAULT_GRAV, lanes_per_window=0):
        p = CpiParams()
        p.sigma_w, p.sigma_wb, p.sigma_a, p.sigma_ab = sigmas
        p.grav[:] = grav
        p.model, p.imu_avg = int(model), int(bool(imu_avg))
        p.state_transition_jacobians = int(bool(state_transition_jacobians))
        p.lanes_per_window = int(lanes_per_window)
        return p

    def alloc_outputs(self, W, want=("mean", "jac", "cov"), model=1, packed=False):
        """packed=True: all fields are views of ONE flat buffer (field-major, cpi_amd.dist.pack_layout), returned under
        the extra key "_flat" together with "_fields" -- a rank's whole output is then one contiguous slab and the
        multi-GPU gather one collective (cpi_amd.dist.gather_packed)."""
        names = []
        for name, n in OUT_FIELDS:
            grp = _group_of(name)
            if grp not in want:
                continue
            if model != 2 and name in ("O_a", "O_b"):
                continue
            names.append((name, n))
        out = {}
        if packed:
            from .dist import alloc_packed
            flat, out = alloc_packed(names, W, self.device)
            out["_flat"], out["_fields"] = flat, names
            return out
        for name, n in names:
            shape = (W,) if n == 1 else (W, n)
            out[name] = torch.empty(shape, dtype=torch.float64, device=self.device)
        return out

    @staticmethod
    def _outputs_struct(out):
        o = CpiOutputs()
        for name, _ in OUT_FIELDS:
            t = out.get(name)
            setattr(o, name, t.data_ptr() if t is not None else None)
        return o

    @staticmethod
    def _window_shape(knots, lin, first=None, count=None, N=None, others=(), cuda=True):
        """(W, N) of a batch -- dense knots [W, N + 1, 7], or ragged (first given: N = max intervals per window) -- after the
        asserts every windowed entry makes of its inputs (others: the remaining tensors, None allowed)."""
        if first is None:
            W, n1, _ = knots.shape
            N = n1 - 1
        else:
            W = first.shape[0]
            assert N is not None, "ragged layout needs N = max intervals per window"
        for t in (knots, lin, first, count) + tuple(others):
            assert t is None or (t.is_cuda == cuda and t.is_contiguous()), "inputs must be contiguous %s tensors" % ("CUDA" if cuda else "CPU")
        assert knots.dtype == torch.float64 and lin.dtype == torch.float64 and (count is None or count.dtype == torch.int32)
        return W, N

    def _carry_out(self, W, model, carry_in, carry_out, **where):
        """carry_out, allocated ([W, carry_doubles] float64; where: device= or pin_memory=) when not given; both records checked."""
        cd = self.carry_doubles(model)
        if carry_out is None and cd > 0:
            carry_out = torch.empty((W, cd), dtype=torch.float64, **where)
        for t in (carry_in, carry_out):
            assert t is None or (t.dtype == torch.float64 and t.numel() >= W * cd), "carry records are [W, carry_doubles] float64"
        return carry_out

    @staticmethod
    def _host_outputs(lead, groups, model, pinned):
        """CPU tensors of leading shape `lead` ((W,) or (W, N)) for the fields of these want-groups, page-locked when pinned."""
        return {name: torch.empty(lead if n == 1 else lead + (n,), dtype=torch.float64, pin_memory=pinned)
                for name, n in OUT_FIELDS if _group_of(name) in groups and (model == 2 or name not in ("O_a", "O_b"))}

    def preintegrate(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None,
                     count=None, N=None, out=None):
        """knots [W,N+1,7] (dense) or [K,7] with first[W] (int64) / count[W] (int32); lin [W,6];
        q_k_lin [W,4].  All CUDA float64 tensors.  Returns a dict of device tensors (matrices flat,
        column-major).  Asynchronous on the engine's stream."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, first, count, N, (q_k_lin,))
        if out is None:
            out = self.alloc_outputs(W, want, params.model)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_batch(self.ctx, C.byref(params), W, N, _ptr(knots), _ptr(first), _ptr(count),
                                                    _ptr(lin), _ptr(q_k_lin), C.byref(o)))
        return out

    def carry_doubles(self, model):
        """Doubles per window of a carry record (cpi_carry_doubles): 0 for the Forster comparator or an invalid model."""
        return int(self.lib.cpi_carry_doubles(int(model)))

    def preintegrate_resume(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None, count=None,
                            N=None, carry_in=None, carry_out=None, out=None):
        """cpi_preintegrate_resume: continue every window from carry_in ([W, carry_doubles] float64 CUDA tensor, None = the
        zero state) over these knots (layouts as in preintegrate).  Returns (out, carry_out); out holds the measurement of all
        the intervals so far, carry_out (allocated when not given) the state to continue from.  Asynchronous."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, first, count, N, (q_k_lin, carry_in, carry_out))
        carry_out = self._carry_out(W, params.model, carry_in, carry_out, device=self.device)
        if out is None:
            out = self.alloc_outputs(W, want, params.model)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_resume(self.ctx, C.byref(params), W, N, _ptr(knots), _ptr(first), _ptr(count),
                                                     _ptr(lin), _ptr(q_k_lin), _ptr(carry_in), _ptr(carry_out), C.byref(o)))
        return out, carry_out

    @staticmethod
    def _running_want(want, model):
        # model 2 has no running Jacobians (cpi_preintegrate_running refuses the fields): the default want drops them, an
        # explicit request reaches the library and is refused there
        return tuple(g for g in want if not (g == "jac" and model == 2 and want == ("mean", "jac", "cov")))

    @staticmethod
    def _running_views(flat, W, N):
        return {k: (v if k.startswith("_") else v.view((W, N) + tuple(v.shape[1:]))) for k, v in flat.items()}

    def _rows_out(self, W, N, want, params, out, filter_want, cuda=True, packed=False, pinned=None):
        """(rows, their cpi_outputs): `out`, or [W, N, ...] tensors allocated for the want-groups -- device views of [W * N, ...]
        arrays (packed as in alloc_outputs) or host tensors (page-locked when pinned).  filter_want: the default want loses model
        2's "jac" (_running_want); the _stj forms serve it."""
        if out is None:
            want = self._running_want(tuple(want), params.model) if filter_want else tuple(want)
            if cuda:
                out = self._running_views(self.alloc_outputs(W * N, want, params.model, packed), W, N)
            else:
                out = self._host_outputs((W, N), want, params.model, pinned)
        return out, self._outputs_struct(out)   # which reads the field names only: a packed dict's "_flat" / "_fields" do not reach it

    def _running_args(self, knots, lin, q_k_lin, params, want, first, count, N, carry=None, packed=False, pinned=None, out=None, cuda=True,
                      filter_want=True):
        """What the preintegrate_running* methods share, up to the C call: the asserts, then carry_out and the rows where not given,
        then the engine on torch's stream.  carry: None or (carry_in, carry_out) for the _resume forms; cuda: device tensors (dense
        or ragged, rows packed on request) or host tensors (dense; fresh ones page-locked when pinned); filter_want: see _rows_out.
        Returns (the arguments of the entry, rows, carry_out)."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, first, count, N, (q_k_lin,) + (carry or ()), cuda)
        if carry is not None:
            where = {"device": self.device} if cuda else {"pin_memory": pinned}
            carry = (carry[0], self._carry_out(W, params.model, carry[0], carry[1], **where))
        out, o = self._rows_out(W, N, want, params, out, filter_want, cuda, packed, pinned)
        self._sync_stream()
        windows = (_ptr(first), _ptr(count)) if cuda else (None, _ptr(count), 0)
        rest = (C.byref(o),) if carry is None else (_ptr(carry[0]), _ptr(carry[1]), C.byref(o))
        args = (self.ctx, C.byref(params), W, N, _ptr(knots)) + windows + (_ptr(lin), _ptr(q_k_lin)) + rest
        return args, out, None if carry is None else carry[1]

    def preintegrate_running(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None,
                             count=None, N=None, packed=False, out=None):
        """cpi_preintegrate_running: the measurement after EVERY interval.  Inputs as in preintegrate.  Returns a dict of
        tensors with leading shape [W, N]: entry [w, i] is what preintegrate returns for window w cut after interval i
        (skipped intervals and i >= count repeat the previous row; [w, N - 1] is the window's measurement).  The tensors are
        views of [W * N, ...] arrays, so {k: v.reshape(W * N, ...)} is an ordinary measurement dict for predict / factor_eval
        (idx_i[row] = row // N).  Models 1 and 2; Jacobians for model 1 only (the default want drops them for model 2).
        packed / out: as alloc_outputs(W * N, ..., packed) / the dict of an earlier call.  Asynchronous."""
        args, out, _ = self._running_args(knots, lin, q_k_lin, params, want, first, count, N, packed=packed, out=out)
        self._check(self.lib.cpi_preintegrate_running(*args))
        return out

    def preintegrate_running_host(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), count=None,
                                  pinned=True, out=None):
        """preintegrate_running for a dense batch held in HOST memory (CPU float64 tensors): cpi_preintegrate_running_host.
        Returns a dict of CPU tensors with leading shape [W, N]; synchronous."""
        args, out, _ = self._running_args(knots, lin, q_k_lin, params, want, None, count, None, pinned=pinned, out=out, cuda=False)
        self._check(self.lib.cpi_preintegrate_running_host(*args))
        return out

    def preintegrate_running_stj(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None,
                                 count=None, N=None, packed=False, out=None):
        """cpi_running_stj_batch: preintegrate_running with model 2's Jacobian rows.  Arguments and result as
        preintegrate_running; for model 2 (state_transition_jacobians set) "jac" means all seven matrices J_q J_a J_b H_a H_b
        O_a O_b after every interval, read out of the state transition columns of the covariance recursion.  The mean and P /
        P_sym rows are bit for bit those of preintegrate_running; without "jac", or for model 1, the call is
        preintegrate_running.  Asynchronous."""
        args, out, _ = self._running_args(knots, lin, q_k_lin, params, want, first, count, N, packed=packed, out=out, filter_want=False)
        self._check(self.lib.cpi_running_stj_batch(*args))
        return out

    def preintegrate_running_stj_host(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), count=None,
                                      pinned=True, out=None):
        """preintegrate_running_stj for a dense batch held in HOST memory (CPU float64 tensors):
        cpi_running_stj_batch_host.  Returns a dict of CPU tensors with leading shape [W, N]; synchronous."""
        args, out, _ = self._running_args(knots, lin, q_k_lin, params, want, None, count, None, pinned=pinned, out=out, cuda=False, filter_want=False)
        self._check(self.lib.cpi_running_stj_batch_host(*args))
        return out

    def preintegrate_running_resume(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None,
                                    count=None, N=None, carry_in=None, carry_out=None, packed=False, out=None):
        """cpi_preintegrate_running_resume: the rows of preintegrate_running for windows that continue from carry_in
        ([W, carry_doubles] float64 CUDA tensor, None = the zero state) over these knots.  Returns (rows, carry_out): rows as
        preintegrate_running returns them ([W, N, ...] views; entry [w, i] is the measurement of everything the record stands
        for plus intervals 0 .. i of this segment), carry_out (allocated when not given, never carry_in itself) as
        preintegrate_resume returns it -- the state of row N - 1.  The records of the two resume entries are interchangeable.
        Models 1 and 2; Jacobians for model 1 only (the default want drops them for model 2).  Asynchronous."""
        args, out, carry_out = self._running_args(knots, lin, q_k_lin, params, want, first, count, N, (carry_in, carry_out), packed=packed,
                                                  out=out)
        self._check(self.lib.cpi_preintegrate_running_resume(*args))
        return out, carry_out

    def preintegrate_running_resume_host(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), count=None,
                                         carry_in=None, carry_out=None, pinned=True, out=None):
        """preintegrate_running_resume for a dense batch held in HOST memory (CPU float64 tensors, the records included):
        cpi_preintegrate_running_resume_host.  Returns (rows, carry_out) as CPU tensors; synchronous."""
        args, out, carry_out = self._running_args(knots, lin, q_k_lin, params, want, None, count, None, (carry_in, carry_out), pinned=pinned,
                                                  out=out, cuda=False)
        self._check(self.lib.cpi_preintegrate_running_resume_host(*args))
        return out, carry_out

    def preintegrate_running_resume_stj(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None,
                                        count=None, N=None, carry_in=None, carry_out=None, packed=False, out=None):
        """cpi_running_resume_stj_batch: preintegrate_running_resume with model 2's Jacobian rows.  Arguments and result as
        preintegrate_running_resume; for model 2 (state_transition_jacobians set) "jac" means all seven matrices after every
        interval of this segment, continued from the transition columns carry_in holds (the call then needs and leaves the
        covariance state whether or not "cov" is wanted).  The mean and P / P_sym rows and carry_out are bit for bit those of
        preintegrate_running_resume; without "jac", or for model 1, the call is preintegrate_running_resume.  A dense call on
        knots [W, 2, 7] with count = zeros reads the record out as one row per window: the base of query_open.  Asynchronous."""
        args, out, carry_out = self._running_args(knots, lin, q_k_lin, params, want, first, count, N, (carry_in, carry_out), packed=packed,
                                                  out=out, filter_want=False)
        self._check(self.lib.cpi_running_resume_stj_batch(*args))
        return out, carry_out

    def preintegrate_running_resume_stj_host(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), count=None,
                                             carry_in=None, carry_out=None, pinned=True, out=None):
        """preintegrate_running_resume_stj for a dense batch held in HOST memory (CPU float64 tensors, the records included):
        cpi_running_resume_stj_batch_host.  Returns (rows, carry_out) as CPU tensors; synchronous."""
        args, out, carry_out = self._running_args(knots, lin, q_k_lin, params, want, None, count, None, (carry_in, carry_out), pinned=pinned,
                                                  out=out, cuda=False, filter_want=False)
        self._check(self.lib.cpi_running_resume_stj_batch_host(*args))
        return out, carry_out

    @staticmethod
    def _wants_cov(want):
        return "cov" in want or "cov_sym" in want

    @staticmethod
    def _check_queries(qwin, qtime):
        Q = qtime.shape[0]
        assert qwin.dtype == torch.int32 and qtime.dtype == torch.float64 and qwin.shape == (Q,), "qwin [Q] int32, qtime [Q] float64"
        return Q

    @staticmethod
    def _check_rows(rows, W, N, text):
        """The tensors of a rows dict, each a contiguous CUDA tensor of leading shape [W, N]; text: what the caller says otherwise."""
        r = _fields(rows)
        for v in r.values():
            assert v.is_cuda and v.is_contiguous() and v.shape[:2] == (W, N), text
        return r

    def _query_args(self, knots, lin, rows, rows_text, qwin, qtime, q_k_lin, params, want, first, count, N, out, base=()):
        """What query / query_stj / query_open share, up to the C call: the asserts, then the outputs where not given, then the
        engine on torch's stream.  base: nothing, or (base,) for query_open, whose entry takes the base rows and base_N last.
        Returns (the arguments of the entry, out)."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, first, count, N, (q_k_lin, qwin, qtime))
        Q = self._check_queries(qwin, qtime)
        r = self._check_rows(rows, W, N, rows_text)
        if base:
            bo, base_N = None, 0
            if base[0] is not None:
                b = _fields(base[0])
                sizes = {v.numel() // (W * n) for k, v in b.items() for name, n in OUT_FIELDS if name == k}
                assert len(sizes) == 1 and all(v.is_cuda and v.is_contiguous() and v.shape[0] == W for v in b.values()), \
                    "base: a dict of [W, base_N, ...] tensors with one base_N"
                base_N = int(sizes.pop())
                bo = C.byref(self._outputs_struct(b))
            base = (bo, base_N)
        if out is None:
            out = self.alloc_outputs(Q, tuple(want), params.model)
        o = self._outputs_struct(out)
        ro = self._outputs_struct(r)
        self._sync_stream()
        return (self.ctx, C.byref(params), W, N, _ptr(knots), _ptr(first), _ptr(count), _ptr(lin), _ptr(q_k_lin), C.byref(ro), Q,
                _ptr(qwin), _ptr(qtime), C.byref(o)) + base, out

    def _query_host_args(self, knots, lin, qwin, qtime, q_k_lin, params, want, count, carry, pinned, out):
        """What query_host / query_stj_host / query_open_host share, up to the C call.  carry: nothing, or (carry_in, carry_out)
        for query_open_host.  Returns (the arguments of the entry, out, carry_out)."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, count=count, others=(q_k_lin, qwin, qtime) + carry, cuda=False)
        Q = self._check_queries(qwin, qtime)
        if carry:
            carry = (carry[0], self._carry_out(W, params.model, carry[0], carry[1], pin_memory=pinned))
        if out is None:
            out = self._host_outputs((Q,), tuple(want), params.model, pinned)
        o = self._outputs_struct(out)
        self._sync_stream()
        return (self.ctx, C.byref(params), W, N, _ptr(knots), None, _ptr(count), 0, _ptr(lin), _ptr(q_k_lin)) + tuple(map(_ptr, carry)) + (
            Q, _ptr(qwin), _ptr(qtime), C.byref(o)), out, carry and carry[1]

    def query(self, knots, lin, rows, qwin, qtime, q_k_lin=None, params=None, want=("mean",), first=None, count=None, N=None,
              out=None):
        """cpi_query_batch: the measurement at arbitrary times inside a window.  knots / lin / q_k_lin / params / first / count / N:
        the arguments of the preintegrate_running call that returned `rows` (its dict, [W, N, ...] tensors); qwin [Q] int32 and
        qtime [Q] float64 CUDA tensors: query k asks for window qwin[k] at time qtime[k] (any order, repeats allowed; the
        stamps of a queried window must be finite and non-decreasing).  want: ("mean",) or ("mean", "jac") -- the Jacobians for
        model 1 only, and rows must hold them -- and / or "cov" (P, [Q, 225]) / "cov_sym" (P_sym, [Q, 120]): the covariance at
        the query times (cpi_query_cov_batch; rows must hold q and P or P_sym, models 1 and 2).  Returns a dict of [Q, ...]
        tensors: a time on a knot stamp (or at / past the window's end) gives the running row bit for bit, a time inside an
        interval that row advanced over the partial interval with the reading held, a time before the window the zero state, a
        NaN time NaN.  The result is an ordinary measurement dict: predict(model, result, states, idx_i=qwin) gives the states
        AT the query times, sqrt_information(result["P_sym"]) the whitening of a factor there.  Asynchronous."""
        entry = self.lib.cpi_query_cov_batch if self._wants_cov(want) else self.lib.cpi_query_batch
        args, out = self._query_args(knots, lin, rows, "rows: the [W, N, ...] dict of preintegrate_running", qwin, qtime, q_k_lin, params,
                                     want, first, count, N, out)
        self._check(entry(*args))
        return out

    def query_host(self, knots, lin, qwin, qtime, q_k_lin=None, params=None, want=("mean",), count=None, pinned=True, out=None):
        """query for a dense batch held in HOST memory (CPU tensors): cpi_query_batch_host.  There is no rows argument -- the
        running rows are computed on the device and stay there, Q rows come back.  qwin and the stamps of every queried window
        are validated (CpiError names the window).  want as in query: with "cov" / "cov_sym" the call is
        cpi_query_cov_batch_host and the covariance rows stay on the device as well.  Returns a dict of CPU tensors [Q, ...];
        synchronous."""
        entry = self.lib.cpi_query_cov_batch_host if self._wants_cov(want) else self.lib.cpi_query_batch_host
        args, out, _ = self._query_host_args(knots, lin, qwin, qtime, q_k_lin, params, want, count, (), pinned, out)
        self._check(entry(*args))
        return out

    def query_stj(self, knots, lin, rows, qwin, qtime, q_k_lin=None, params=None, want=("mean",), first=None, count=None, N=None,
                  out=None):
        """cpi_query_stj_batch: query with model 2's Jacobians.  Arguments and result as query; for model 2
        (state_transition_jacobians set) "jac" in want means all seven matrices J_q J_a J_b H_a H_b O_a O_b at the query times,
        and rows -- the dict of preintegrate_running_stj on the same arguments -- must then hold q and all seven.  The mean
        fields and P / P_sym are bit for bit those of query; the result feeds sqrt_information / factor_eval for model 2 with
        idx_i = qwin.  Asynchronous."""
        args, out = self._query_args(knots, lin, rows, "rows: the [W, N, ...] dict of preintegrate_running_stj", qwin, qtime, q_k_lin, params,
                                     want, first, count, N, out)
        self._check(self.lib.cpi_query_stj_batch(*args))
        return out

    def query_stj_host(self, knots, lin, qwin, qtime, q_k_lin=None, params=None, want=("mean",), count=None, pinned=True, out=None):
        """query_stj for a dense batch held in HOST memory (CPU tensors): cpi_query_stj_batch_host.  No rows argument: the running
        rows (for a model-2 Jacobian request all seven Jacobian fields) are computed on the device and stay there.  Returns a
        dict of CPU tensors [Q, ...]; synchronous."""
        args, out, _ = self._query_host_args(knots, lin, qwin, qtime, q_k_lin, params, want, count, (), pinned, out)
        self._check(self.lib.cpi_query_stj_batch_host(*args))
        return out

    def query_open(self, knots, lin, rows, qwin, qtime, base, q_k_lin=None, params=None, want=("mean",), first=None, count=None,
                   N=None, out=None):
        """cpi_query_open_batch: query_stj for windows that are still open.  knots / lin / q_k_lin / params / first / count / N and
        rows describe the SEGMENT (the chunk that has just arrived) as given to and returned by preintegrate_running_resume[_stj];
        base: the state each window had before knot 0 of the segment, as a dict of [W, base_N, ...] (or [W, ...]) tensors whose row
        [w, base_N - 1] is used -- the rows dict of the PREVIOUS chunk's call in place, or the one-row read-out of a record
        (preintegrate_running_resume_stj).  It stands where the zero state stands in query: a time on or before the segment's
        first stamp returns the base row bit for bit, a time inside interval 0 advances it.  base must hold what rows must hold
        for the request.  base=None: query_stj.  Returns a dict of [Q, ...] tensors.  Asynchronous."""
        args, out = self._query_args(knots, lin, rows, "rows: the [W, N, ...] dict of preintegrate_running_resume[_stj]", qwin, qtime, q_k_lin,
                                     params, want, first, count, N, out, (base,))
        self._check(self.lib.cpi_query_open_batch(*args))
        return out

    def query_open_host(self, knots, lin, qwin, qtime, q_k_lin=None, params=None, want=("mean",), count=None, carry_in=None,
                        carry_out=None, pinned=True, out=None):
        """One chunk of a live loop from HOST memory (CPU tensors): cpi_query_open_batch_host.  The base rows are read out of
        carry_in (None: the zero state), the chunk's rows and carry_out are computed on the device, the queries run against
        them.  Returns (out, carry_out): a dict of CPU tensors [Q, ...] and the record to continue from; synchronous."""
        args, out, carry_out = self._query_host_args(knots, lin, qwin, qtime, q_k_lin, params, want, count, (carry_in, carry_out), pinned, out)
        self._check(self.lib.cpi_query_open_batch_host(*args))
        return out, carry_out

    # ------------------------------------------------------------------ joining consecutive windows
    def _merge_args(self, meas, G, first, count, cuda):
        m = _fields(meas)
        assert "DT" in m, "meas: a measurement dict ([rows, ...] tensors) as the preintegration entries return it"
        in_rows = m["DT"].shape[0]
        for k, v in m.items():
            assert v.is_cuda == cuda and v.is_contiguous() and v.dtype == torch.float64 and v.shape[0] == in_rows, \
                "meas: contiguous float64 %s tensors of %d rows" % ("CUDA" if cuda else "CPU", in_rows)
        for t, dt, name in ((first, torch.int64, "first [M] int64"), (count, torch.int32, "count [M] int32")):
            assert t is None or (t.is_cuda == cuda and t.is_contiguous() and t.dtype == dt and t.dim() == 1), name
        assert first is None or count is None or first.shape == count.shape, "first and count are both [M]"
        if G is None:
            assert first is None and count is None, "G (the largest group) is required with first / count"
            G = max(in_rows, 1)                        # one group: everything joined
        M = first.shape[0] if first is not None else count.shape[0] if count is not None else (in_rows + G - 1) // max(G, 1)
        return m, in_rows, int(G), M

    def merge(self, meas, G=None, first=None, count=None, want=("mean", "jac", "cov"), packed=False, out=None):
        """cpi_merge_batch: consecutive preintegrated windows joined into one measurement, without the IMU readings.  meas: a
        model-1 measurement dict of [rows, ...] CUDA tensors (what preintegrate / preintegrate_stream / ... return), the windows
        in time order and ALL PREINTEGRATED AT THE SAME lin (the call cannot check that).  Output row j = rows first[j] ..
        first[j] + count[j] - 1 joined, oldest first; first [M] int64 (None: group j starts at row j * G), count [M] int32 (None:
        G rows each; clamped into [0, G]; groups are clipped at the end of meas), G = the largest group (None without first /
        count: everything joined into one row).  Decimation to every 5th update time is merge(meas, G=5).  count 0 gives the zero
        state, count 1 the row itself bit for bit.  want as in query: "mean", "jac", "cov" (P) and / or "cov_sym" (P_sym); the
        Jacobians and the covariance need all five Jacobians in meas, the covariance P or P_sym as well.  packed: the outputs are
        views of one flat buffer (alloc_outputs).  Returns a dict of [M, ...] tensors.  Asynchronous."""
        m, in_rows, G, M = self._merge_args(meas, G, first, count, True)
        if out is None:
            out = self.alloc_outputs(M, tuple(want), 1, packed)
        o = self._outputs_struct(out)
        i = self._outputs_struct(m)
        self._sync_stream()
        self._check(self.lib.cpi_merge_batch(self.ctx, 1, M, G, in_rows, C.byref(i), _ptr(first), _ptr(count), C.byref(o)))
        return out

    def merge_host(self, meas, G=None, first=None, count=None, want=("mean", "jac", "cov"), packed=False, out=None, pinned=True):
        """merge for measurements held in HOST memory (CPU tensors): cpi_merge_batch_host.  Only the fields the request reads go
        up; the dense layout runs through the chunked pipeline, a ragged one is staged whole.  Returns a dict of CPU tensors
        [M, ...] (packed: views of one flat buffer); synchronous; bit for bit the device form."""
        m, in_rows, G, M = self._merge_args(meas, G, first, count, False)
        if out is None:
            if packed:
                from .dist import alloc_packed
                names = [(name, n) for name, n in OUT_FIELDS if _group_of(name) in want and name not in ("O_a", "O_b")]
                flat, out = alloc_packed(names, M, torch.device("cpu"))
                out["_flat"], out["_fields"] = flat, names
            else:
                out = self._host_outputs((M,), tuple(want), 1, pinned)
        o = self._outputs_struct(out)
        i = self._outputs_struct(m)
        self._sync_stream()
        self._check(self.lib.cpi_merge_batch_host(self.ctx, 1, M, G, in_rows, C.byref(i), _ptr(first), _ptr(count), C.byref(o)))
        return out

    def preintegrate_host(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), count=None, pinned=True, out=None):
        """Dense batch held in HOST memory (CPU float64 tensors; pinned ones overlap upload / kernels / download):
        cpi_preintegrate_batch_host.  Returns a dict of CPU tensors (page-locked when pinned=True; out= re-uses the
        dict of an earlier call); synchronous."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, count=count, others=(q_k_lin,), cuda=False)
        if out is None:
            out = self._host_outputs((W,), want, params.model, pinned)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_batch_host(self.ctx, C.byref(params), W, N, _ptr(knots), None, _ptr(count), 0,
                                                         _ptr(lin), _ptr(q_k_lin), C.byref(o)))
        return out

    def tile_knots(self, knots):
        """dense knots [W, N+1, 7] -> tiles [ceil(W/64), N+1, 7, 64] on the device (cpi_tile_knots)."""
        W, n1, _ = knots.shape
        tiles = torch.empty(((W + 63) // 64, n1, 7, 64), dtype=torch.float64, device=self.device)
        self._sync_stream()
        self._check(self.lib.cpi_tile_knots(self.ctx, W, n1 - 1, _ptr(knots), _ptr(tiles)))
        return tiles

    def tile_windows(self, knots, first, count, N):
        """a shared knot stream [K, 7] indexed by first[W] (int64) / count[W] (int32) -> tiles [ceil(W/64), N+1, 7, 64] on the
        device (cpi_tile_windows).  A full extra pass: one-off use and tests."""
        W = first.shape[0]
        tiles = torch.empty(((W + 63) // 64, N + 1, 7, 64), dtype=torch.float64, device=self.device)
        self._sync_stream()
        self._check(self.lib.cpi_tile_windows(self.ctx, W, N, _ptr(knots), _ptr(first), _ptr(count), _ptr(tiles)))
        return tiles

    def assemble_tiles(self, stream, update_times, N, tiles=None, count=None):
        """Window assembly ON THE DEVICE, straight into the tiled layout (cpi_assemble_tiles; GraphSolver_IMU.cpp:50-69 for
        every window at once): stream [K, 7] with non-decreasing stamps, update_times [U] non-decreasing, both CUDA float64.
        Returns (tiles [ceil(U/64), N+1, 7, 64], count [U] int32 = the TRUE interval counts: check count.max() <= N)."""
        K, U = stream.shape[0], update_times.shape[0]
        assert stream.is_cuda and stream.is_contiguous() and update_times.is_cuda and update_times.is_contiguous()
        if tiles is None:
            tiles = torch.empty(((U + 63) // 64, N + 1, 7, 64), dtype=torch.float64, device=self.device)
        if count is None:
            count = torch.empty((U,), dtype=torch.int32, device=self.device)
        self._sync_stream()
        self._check(self.lib.cpi_assemble_tiles(self.ctx, K, _ptr(stream), U, _ptr(update_times), N, _ptr(tiles), _ptr(count)))
        return tiles, count

    @staticmethod
    def _check_f64(tensors, cuda=True):
        where = "CUDA" if cuda else "CPU"
        for t in tensors:
            assert t is None or (t.is_cuda == cuda and t.is_contiguous() and t.dtype == torch.float64), "inputs must be contiguous %s float64 tensors" % where

    @staticmethod
    def _bound_N(N, check_counts, who, bound, why=""):
        """N as given, else bound() -- with check_counts only: a bound nobody checks the counts against has to be the caller's."""
        if N is not None:
            return int(N)
        if not check_counts:
            raise ValueError("%s: check_counts=False needs an explicit N%s" % (who, why))
        return bound()

    @staticmethod
    def _check_host_counts(cnt, U, N, who):
        if U and int(cnt.max()) > N:
            raise ValueError("%s: a window has %d intervals, N = %d" % (who, int(cnt.max()), N))

    def preintegrate_stream(self, stream, update_times, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), N=None, out=None,
                            return_counts=False, check_counts=True, workspace=None):
        """One IMU stream cut at update times and preintegrated IN PLACE (cpi_preintegrate_stream: the caller-side loop of
        GraphSolver_IMU.cpp:43-75 for all windows at once, zero copies of the IMU data, every model and output).
        stream [K, 7] with non-decreasing stamps, update_times [U] non-decreasing, lin [U, 6], q_k_lin [U, 4]: CUDA float64.
        N = upper bound of the intervals per window; with check_counts (one synchronisation) raises when a window holds more.
        N=None (default): the exact bound, computed from the stamps by stream_bound() -- one searchsorted over the K stamps and ONE
        HOST SYNCHRONISATION on first use of a (stream, update_times) pair (cached afterwards by storage and version), issued on
        the engine's stream: that first call is NOT asynchronous and NOT graph-capturable.  Callers that need either pass an integer
        N (e.g. stream_bound() taken once, outside the capture) or N="loose" = min(K, 65535): no pass over the stamps, no
        synchronisation -- the library picks the mean kernel's lane split from N, so a loose bound costs speed on small batches
        (and check_counts=False keeps the whole call free of synchronisations)."""
        params = params or self.make_params()
        K, U = stream.shape[0], update_times.shape[0]
        self._check_f64((stream, update_times, lin, q_k_lin))
        if N is None:
            N = self.stream_bound(stream, update_times)
        elif isinstance(N, str):
            assert N == "loose", 'N: an integer, None (exact bound, synchronises once per pair) or "loose"'
            N = max(1, min(K, 65535))
        if out is None:
            out = self.alloc_outputs(U, want, params.model)
        ws = workspace if workspace is not None else self.stream_workspace(U)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_stream(self.ctx, C.byref(params), K, _ptr(stream), U, _ptr(update_times), int(N), _ptr(lin),
                                                     _ptr(q_k_lin), _ptr(ws), C.byref(o)))
        # The workspace (28 bytes per window) must outlive the kernels that read it.  Allocated here it came from torch's
        # caching allocator on the stream the kernels were just issued on (follow mode), so dropping the reference is safe: the
        # block can only be handed to later, stream-ordered allocations of that stream.  An engine pinned to an explicit stream
        # says so to the allocator.  Nothing but output fields is stored in the returned dict.
        if workspace is None and not self._follow and self.stream is not None:
            ws.record_stream(self.stream)
        counts = self._stream_counts(ws, U, N, return_counts, check_counts, "preintegrate_stream")
        return (out, counts) if return_counts else out

    def stream_bound(self, stream, update_times):
        """Longest window (whole intervals + a tail) that cutting `stream` at `update_times` can produce: the closed form of
        the deque loop (GraphSolver_IMU.cpp:50-69; cpi_cut_windows_kernel) on the stamps, tail assumed.  Device tensors: issued
        on the ENGINE's stream (not torch's current one) and followed by one host synchronisation (.item()); the result is cached
        per (storage, shape, version) of the two tensors, so a loop over the same buffers pays it once."""
        key = tuple((t.data_ptr(), tuple(t.shape), t._version) for t in (stream, update_times))
        hit = getattr(self, "_bound_cache", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        pinned = stream.is_cuda and not self._follow and self.stream is not None
        with torch.cuda.stream(self.stream) if pinned else _nullctx():
            n = self._stream_bound(stream, update_times)
        self._bound_cache = (key, n)
        return n

    @staticmethod
    def _stream_bound(stream, update_times):
        K, U = stream.shape[0], update_times.shape[0]
        if K == 0 or U == 0:
            return 1
        c = torch.searchsorted(stream[:, 0].contiguous(), update_times, right=True)
        fp = torch.zeros_like(c)
        fp[1:] = (c[:-1] - 1).clamp_min(0)
        m = torch.maximum((c - 1).clamp_min(0), fp) - fp
        return max(1, min(int(m.max().item()) + 1, 65535))

    def stream_workspace(self, U):
        """Device workspace of preintegrate_stream for U windows (28 bytes per window; re-usable across calls)."""
        return torch.empty((self.lib.cpi_stream_workspace_bytes(U) // 8 + 1,), dtype=torch.float64, device=self.device)

    def preintegrate_stream_host(self, stream, update_times, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), N=None,
                                 pinned=False, return_counts=False):
        """preintegrate_stream for a caller that holds everything in HOST memory (cpi_preintegrate_stream_host): the IMU
        stream [K,7], the update times [U], one linearisation point per window -- CPU float64 tensors in, CPU tensors out;
        synchronous.  A window longer than N intervals raises (N defaults to the longest window the stamps allow: nothing can be)."""
        params = params or self.make_params()
        K, U = stream.shape[0], update_times.shape[0]
        N = int(N) if N is not None else self._stream_bound(stream, update_times)     # the same default as the device entry: same lane split, same bits
        self._check_f64((stream, update_times, lin, q_k_lin), cuda=False)
        out = self._host_outputs((U,), want, params.model, pinned)
        cnt = torch.empty((U,), dtype=torch.int32)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_stream_host(self.ctx, C.byref(params), K, _ptr(stream), U, _ptr(update_times), N,
                                                          _ptr(lin), _ptr(q_k_lin), C.byref(o), _ptr(cnt)))
        self._check_host_counts(cnt, U, N, "preintegrate_stream_host")
        return (out, cnt) if return_counts else out

    @staticmethod
    def _runs(data, offsets, name, device):
        """(one tensor, offsets) or a list of per-run tensors (offsets None) -> (tensor, int64 offsets [R + 1] on `device`)."""
        if isinstance(data, (list, tuple)):
            assert offsets is None, "%s: a list of per-run tensors carries its own offsets (pass None)" % name
            lens = [int(t.shape[0]) for t in data]
            data = torch.cat(list(data), dim=0).contiguous() if data else None
            offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), device=device)
            return data, offsets
        assert offsets is not None, "%s: one tensor needs its run offsets [R + 1]" % name
        if not torch.is_tensor(offsets):
            offsets = torch.tensor(np.asarray(offsets, dtype=np.int64), device=device)
        return data, offsets.to(device=device, dtype=torch.int64).contiguous()

    def preintegrate_streams(self, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin=None, params=None,
                             want=("mean", "jac", "cov"), N=None, out=None, return_counts=False, check_counts=True, workspace=None):
        """MANY IMU streams (runs, trajectories) cut at their update times and preintegrated in ONE call
        (cpi_preintegrate_streams): run r owns the readings stream[stream_offsets[r]:stream_offsets[r + 1]] and the windows
        [update_offsets[r], update_offsets[r + 1]); window u of run r equals window u - update_offsets[r] of preintegrate_stream on
        run r alone (same N, params and lane split).  Stamps non-decreasing within a run, any order across runs.
        stream [K, 7], update_times [U], lin [U, 6], q_k_lin [U, 4]: CUDA float64; the offsets [R + 1]: int64 tensors (moved to
        the device) or sequences.  Convenience: stream may be a LIST of per-run [K_r, 7] tensors and update_times a list of per-run
        [U_r] tensors (pass None as their offsets) -- they are concatenated ONCE, here (a copy of every reading, and offsets built
        on the host: not graph-capturable).
        N, return_counts, check_counts, workspace as in preintegrate_stream: N=None = streams_bound() (one host
        synchronisation, NOT cached), N="loose" = min(K, 65535) (no synchronisation), an integer is used as given."""
        params = params or self.make_params()
        stream, soff = self._runs(stream, stream_offsets, "stream", self.device)
        update_times, uoff = self._runs(update_times, update_offsets, "update_times", self.device)
        if stream is None:
            stream = torch.empty((0, 7), dtype=torch.float64, device=self.device)
        if update_times is None:
            update_times = torch.empty((0,), dtype=torch.float64, device=self.device)
        R, K, U = soff.shape[0] - 1, stream.shape[0], update_times.shape[0]
        assert uoff.shape[0] == R + 1, "stream_offsets and update_offsets must both hold R + 1 entries"
        self._check_f64((stream, update_times, lin, q_k_lin))
        if N is None:
            N = self.streams_bound(stream, soff, update_times, uoff)
        elif isinstance(N, str):
            assert N == "loose", 'N: an integer, None (exact bound, synchronises once) or "loose"'
            N = max(1, min(K, 65535))
        if out is None:
            out = self.alloc_outputs(U, want, params.model)
        ws = workspace if workspace is not None else self.streams_workspace(R, U)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_streams(self.ctx, C.byref(params), R, K, _ptr(stream), _ptr(soff), U, _ptr(update_times),
                                                      _ptr(uoff), int(N), _ptr(lin), _ptr(q_k_lin), _ptr(ws), C.byref(o)))
        # the workspace and the offsets must outlive the kernels that read them (see preintegrate_stream)
        if not self._follow and self.stream is not None:
            for t in ((ws,) if workspace is None else ()) + (soff, uoff, stream, update_times):
                t.record_stream(self.stream)
        counts = self._stream_counts(ws, U, N, return_counts, check_counts, "preintegrate_streams")
        return (out, counts) if return_counts else out

    @staticmethod
    def streams_bound(stream, stream_offsets, update_times, update_offsets):
        """Longest window (whole intervals + a tail) that cutting every run at its update times can produce: stream_bound's closed
        form of the deque loop run by run, the maximum over all runs (runs without readings or update times contribute nothing).
        Works on CPU or CUDA tensors; reads the offsets on the host and ends in ONE host synchronisation.  Not cached: it is
        recomputed on every call (a cache keyed by storage and version serves stale bounds to re-allocated buffers)."""
        so = [int(v) for v in torch.as_tensor(stream_offsets).cpu().tolist()]
        uo = [int(v) for v in torch.as_tensor(update_offsets).cpu().tolist()]
        assert len(so) == len(uo) and len(so) >= 1, "offsets: R + 1 entries each"
        stamps = stream[:, 0].contiguous()
        best = []
        for r in range(len(so) - 1):
            if so[r + 1] <= so[r] or uo[r + 1] <= uo[r]:
                continue
            c = torch.searchsorted(stamps[so[r]:so[r + 1]].contiguous(), update_times[uo[r]:uo[r + 1]].contiguous(), right=True)
            fp = torch.zeros_like(c)
            fp[1:] = (c[:-1] - 1).clamp_min(0)
            best.append((torch.maximum((c - 1).clamp_min(0), fp) - fp).max())
        if not best:
            return 1
        return max(1, min(int(torch.stack(best).max().item()) + 1, 65535))

    def streams_workspace(self, R, U):
        """Device workspace of preintegrate_streams (cpi_streams_workspace_bytes; re-usable across calls)."""
        return torch.empty((self.lib.cpi_streams_workspace_bytes(R, U) // 8 + 1,), dtype=torch.float64, device=self.device)

    def preintegrate_streams_host(self, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin=None, params=None,
                                  want=("mean", "jac", "cov"), N=None, pinned=False, return_counts=False):
        """preintegrate_streams from HOST memory (cpi_preintegrate_streams_host, which validates the offsets): CPU float64 tensors
        and int64 offsets in, CPU tensors out; synchronous.  N defaults to streams_bound(); a longer window raises."""
        params = params or self.make_params()
        soff = torch.as_tensor(np.asarray(stream_offsets, dtype=np.int64))
        uoff = torch.as_tensor(np.asarray(update_offsets, dtype=np.int64))
        R, K, U = soff.shape[0] - 1, stream.shape[0], update_times.shape[0]
        N = int(N) if N is not None else self.streams_bound(stream, soff, update_times, uoff)
        self._check_f64((stream, update_times, lin, q_k_lin), cuda=False)
        out = self._host_outputs((U,), want, params.model, pinned)
        cnt = torch.empty((U,), dtype=torch.int32)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_streams_host(self.ctx, C.byref(params), R, K, _ptr(stream), _ptr(soff), U, _ptr(update_times),
                                                           _ptr(uoff), N, _ptr(lin), _ptr(q_k_lin), C.byref(o), _ptr(cnt)))
        self._check_host_counts(cnt, U, N, "preintegrate_streams_host")
        return (out, cnt) if return_counts else out

    # ---- running rows from IMU stream(s), cut in place (cpi_preintegrate_stream_running / cpi_preintegrate_streams_running)
    def _stream_counts(self, ws, U, N, return_counts, check_counts, who):
        counts = torch.empty((0,), dtype=torch.int32, device=self.device)
        if U and (return_counts or check_counts):
            off = (self.lib.cpi_stream_counts(_ptr(ws), U) - ws.data_ptr()) // 4
            with torch.cuda.stream(self.stream) if (not self._follow and self.stream is not None) else _nullctx():
                counts = ws.view(torch.int32)[off:off + U].clone()   # a copy: a re-used workspace is overwritten by the next call
            if check_counts and int(counts.max().item()) > N:
                raise ValueError("%s: a window has %d intervals, more than N = %d" % (who, int(counts.max().item()), N))
        return counts

    def preintegrate_stream_running(self, stream, update_times, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), N=None,
                                    packed=False, out=None, return_counts=False, check_counts=True, workspace=None, _stj=False):
        """The measurement after EVERY interval of every window of ONE IMU stream, cut in place
        (cpi_preintegrate_stream_running): the inputs, N, return_counts, check_counts and workspace of preintegrate_stream, the
        want / packed / out and the returned [U, N, ...] tensors of preintegrate_running -- entry [u, i] is window u after
        interval i, skipped intervals and i >= count repeat the previous row, [u, N - 1] is what preintegrate_stream returns.
        Bit for bit preintegrate_running on assemble_windows(stream, update_times) with the same N, params and lanes.
        N=None: stream_bound() (the longest window with a tail assumed: exact when the longest window ends in a tail, one row
        more -- a repeated final row per window -- when its update time falls on a stamp; the output is U * N rows; one host
        synchronisation on first use of a pair); with check_counts=False an integer N is REQUIRED: the bound's cache is keyed by storage and version and can serve
        a stale N, which only the count check catches.  Models 1 and 2; Jacobians for model 1 only."""
        params = params or self.make_params()
        K, U = stream.shape[0], update_times.shape[0]
        self._check_f64((stream, update_times, lin, q_k_lin))
        N = self._bound_N(N, check_counts, "preintegrate_stream_running", lambda: self.stream_bound(stream, update_times),
                          " (the cached bound may be stale)")
        out, o = self._rows_out(U, N, want, params, out, not _stj, packed=packed)
        ws = workspace if workspace is not None else self.stream_workspace(U)
        self._sync_stream()
        if _stj:
            self._check(self.lib.cpi_stream_running_stj_batch(self.ctx, C.byref(params), 1, K, _ptr(stream), None, U, _ptr(update_times),
                                                              None, N, _ptr(lin), _ptr(q_k_lin), _ptr(ws), C.byref(o)))
        else:
            self._check(self.lib.cpi_preintegrate_stream_running(self.ctx, C.byref(params), K, _ptr(stream), U, _ptr(update_times), N,
                                                                 _ptr(lin), _ptr(q_k_lin), _ptr(ws), C.byref(o)))
        if workspace is None and not self._follow and self.stream is not None:   # see preintegrate_stream
            ws.record_stream(self.stream)
        counts = self._stream_counts(ws, U, N, return_counts, check_counts, "preintegrate_stream_running")
        return (out, counts) if return_counts else out

    def preintegrate_streams_running(self, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin=None, params=None,
                                     want=("mean", "jac", "cov"), N=None, packed=False, out=None, return_counts=False,
                                     check_counts=True, workspace=None, _stj=False):
        """preintegrate_stream_running for MANY IMU streams in one call (cpi_preintegrate_streams_running): the inputs of
        preintegrate_streams (the list-of-runs form included), the [U, N, ...] rows of preintegrate_running, U the windows of all
        runs.  N=None: streams_bound() (tail assumed, as stream_bound(); one host synchronisation, not cached); check_counts=False
        needs an integer N."""
        params = params or self.make_params()
        stream, soff = self._runs(stream, stream_offsets, "stream", self.device)
        update_times, uoff = self._runs(update_times, update_offsets, "update_times", self.device)
        if stream is None:
            stream = torch.empty((0, 7), dtype=torch.float64, device=self.device)
        if update_times is None:
            update_times = torch.empty((0,), dtype=torch.float64, device=self.device)
        R, K, U = soff.shape[0] - 1, stream.shape[0], update_times.shape[0]
        assert uoff.shape[0] == R + 1, "stream_offsets and update_offsets must both hold R + 1 entries"
        self._check_f64((stream, update_times, lin, q_k_lin))
        N = self._bound_N(N, check_counts, "preintegrate_streams_running", lambda: self.streams_bound(stream, soff, update_times, uoff))
        out, o = self._rows_out(U, N, want, params, out, not _stj, packed=packed)
        ws = workspace if workspace is not None else self.streams_workspace(R, U)
        self._sync_stream()
        entry = self.lib.cpi_stream_running_stj_batch if _stj else self.lib.cpi_preintegrate_streams_running
        self._check(entry(self.ctx, C.byref(params), R, K, _ptr(stream), _ptr(soff), U,
                          _ptr(update_times), _ptr(uoff), N, _ptr(lin), _ptr(q_k_lin), _ptr(ws), C.byref(o)))
        # the workspace and the offsets must outlive the kernels that read them (see preintegrate_stream)
        if not self._follow and self.stream is not None:
            for t in ((ws,) if workspace is None else ()) + (soff, uoff, stream, update_times):
                t.record_stream(self.stream)
        counts = self._stream_counts(ws, U, N, return_counts, check_counts, "preintegrate_streams_running")
        return (out, counts) if return_counts else out

    def preintegrate_stream_running_host(self, stream, update_times, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"),
                                         N=None, pinned=False, return_counts=False, check_counts=True, _stj=False):
        """preintegrate_stream_running from HOST memory (cpi_preintegrate_stream_running_host): CPU float64 tensors in, CPU
        tensors [U, N, ...] out; synchronous.  N defaults to the longest window the stamps allow; with check_counts a window longer
        than N raises (check_counts=False needs an integer N and returns the truncated rows)."""
        params = params or self.make_params()
        K, U = stream.shape[0], update_times.shape[0]
        self._check_f64((stream, update_times, lin, q_k_lin), cuda=False)
        N = self._bound_N(N, check_counts, "preintegrate_stream_running_host", lambda: self._stream_bound(stream, update_times))
        out, o = self._rows_out(U, N, want, params, None, not _stj, cuda=False, pinned=pinned)
        cnt = torch.empty((U,), dtype=torch.int32)
        self._sync_stream()
        if _stj:
            self._check(self.lib.cpi_stream_running_stj_batch_host(self.ctx, C.byref(params), 1, K, _ptr(stream), None, U, _ptr(update_times),
                                                                   None, N, _ptr(lin), _ptr(q_k_lin), C.byref(o), _ptr(cnt)))
        else:
            self._check(self.lib.cpi_preintegrate_stream_running_host(self.ctx, C.byref(params), K, _ptr(stream), U, _ptr(update_times), N,
                                                                      _ptr(lin), _ptr(q_k_lin), C.byref(o), _ptr(cnt)))
        if check_counts:
            self._check_host_counts(cnt, U, N, "preintegrate_stream_running_host")
        return (out, cnt) if return_counts else out

    def preintegrate_streams_running_host(self, stream, stream_offsets, update_times, update_offsets, lin, q_k_lin=None, params=None,
                                          want=("mean", "jac", "cov"), N=None, pinned=False, return_counts=False, check_counts=True,
                                          _stj=False):
        """preintegrate_streams_running from HOST memory (cpi_preintegrate_streams_running_host, which validates the offsets): CPU
        float64 tensors and int64 offsets in, CPU tensors [U, N, ...] out; synchronous.  N, check_counts as in
        preintegrate_stream_running_host (the default N is streams_bound())."""
        params = params or self.make_params()
        soff = torch.as_tensor(np.asarray(stream_offsets, dtype=np.int64))
        uoff = torch.as_tensor(np.asarray(update_offsets, dtype=np.int64))
        R, K, U = soff.shape[0] - 1, stream.shape[0], update_times.shape[0]
        self._check_f64((stream, update_times, lin, q_k_lin), cuda=False)
        N = self._bound_N(N, check_counts, "preintegrate_streams_running_host", lambda: self.streams_bound(stream, soff, update_times, uoff))
        out, o = self._rows_out(U, N, want, params, None, not _stj, cuda=False, pinned=pinned)
        cnt = torch.empty((U,), dtype=torch.int32)
        self._sync_stream()
        entry = self.lib.cpi_stream_running_stj_batch_host if _stj else self.lib.cpi_preintegrate_streams_running_host
        self._check(entry(self.ctx, C.byref(params), R, K, _ptr(stream), _ptr(soff), U, _ptr(update_times), _ptr(uoff), N, _ptr(lin),
                          _ptr(q_k_lin), C.byref(o), _ptr(cnt)))
        if check_counts:
            self._check_host_counts(cnt, U, N, "preintegrate_streams_running_host")
        return (out, cnt) if return_counts else out

    # ---- model 2's Jacobian rows from IMU stream(s) (cpi_stream_running_stj_batch) and the query by absolute time (cpi_query_stream_batch)
    def preintegrate_stream_running_stj(self, stream, update_times, lin, **kw):
        """preintegrate_stream_running with model 2's Jacobian rows (cpi_stream_running_stj_batch, one stream): the arguments and
        the result of preintegrate_stream_running; for model 2 (state_transition_jacobians set) "jac" means all seven matrices after
        every interval, bit for bit preintegrate_running_stj on assemble_windows(stream, update_times).  Without "jac", or for model
        1, the call is preintegrate_stream_running."""
        return self.preintegrate_stream_running(stream, update_times, lin, _stj=True, **kw)

    def preintegrate_streams_running_stj(self, stream, stream_offsets, update_times, update_offsets, lin, **kw):
        """preintegrate_streams_running with model 2's Jacobian rows (cpi_stream_running_stj_batch, many streams)."""
        return self.preintegrate_streams_running(stream, stream_offsets, update_times, update_offsets, lin, _stj=True, **kw)

    def preintegrate_stream_running_stj_host(self, stream, update_times, lin, **kw):
        """preintegrate_stream_running_stj from HOST memory (cpi_stream_running_stj_batch_host); arguments and result as
        preintegrate_stream_running_host."""
        return self.preintegrate_stream_running_host(stream, update_times, lin, _stj=True, **kw)

    def preintegrate_streams_running_stj_host(self, stream, stream_offsets, update_times, update_offsets, lin, **kw):
        """preintegrate_streams_running_stj from HOST memory (cpi_stream_running_stj_batch_host, which validates the offsets)."""
        return self.preintegrate_streams_running_host(stream, stream_offsets, update_times, update_offsets, lin, _stj=True, **kw)

    def query_stream(self, stream, update_times, lin, rows, qtime, q_k_lin=None, params=None, want=("mean",), N=None,
                     stream_offsets=None, update_offsets=None, qrun=None, workspace=None, out=None):
        """cpi_query_stream_batch: the query family by ABSOLUTE time over IMU stream(s) read in place.  stream / update_times / lin /
        q_k_lin / params / N / the offsets: the arguments of the preintegrate_stream[s]_running[_stj] call that returned `rows` (its
        dict of [U, N, ...] tensors; N defaults to their second dimension).  Both offsets None: one stream; otherwise int64 [R + 1]
        CUDA tensors (or sequences) and qrun [Q] int32 names the run of every query.  qtime [Q] float64: absolute times, any order.
        The window (the first of the run whose update time is not before the query time; the last one for a later time) and the
        interval are found on the device.  want as in query_stj: "mean", "jac" (model 1: five matrices, model 2: seven), "cov",
        "cov_sym".  Returns (out, qwin): out a dict of [Q, ...] tensors, bit for bit query_stj on the host-assembled windows with
        qwin; qwin [Q] int32, the GLOBAL window of every query (-1 and NaN rows for a run without update times) -- the idx_i of
        predict / factor_eval / factor_hessian.  Asynchronous; the call cuts the windows into the workspace itself."""
        params = params or self.make_params()
        r = _fields(rows)
        K, U, Q = stream.shape[0], update_times.shape[0], qtime.shape[0]
        if N is None:
            N = next(iter(r.values())).shape[1]
        N = int(N)
        one = stream_offsets is None and update_offsets is None
        soff = uoff = None
        R = 1
        if not one:
            _, soff = self._runs(stream, stream_offsets, "stream", self.device)
            _, uoff = self._runs(update_times, update_offsets, "update_times", self.device)
            R = soff.shape[0] - 1
            assert uoff.shape[0] == R + 1, "stream_offsets and update_offsets must both hold R + 1 entries"
        self._check_f64((stream, update_times, lin, q_k_lin, qtime))
        assert qrun is None or (qrun.is_cuda and qrun.dtype == torch.int32 and qrun.shape == (Q,)), "qrun [Q] int32"
        self._check_rows(r, U, N, "rows: the [U, N, ...] dict of preintegrate_stream[s]_running[_stj]")
        if out is None:
            out = self.alloc_outputs(Q, tuple(want), params.model)
        qwin = torch.empty((Q,), dtype=torch.int32, device=self.device)
        ws = workspace if workspace is not None else self.streams_workspace(R, U)
        o = self._outputs_struct(out)
        ro = self._outputs_struct(r)
        self._sync_stream()
        self._check(self.lib.cpi_query_stream_batch(self.ctx, C.byref(params), R, K, _ptr(stream), _ptr(soff), U, _ptr(update_times),
                                                    _ptr(uoff), N, _ptr(lin), _ptr(q_k_lin), _ptr(ws), C.byref(ro), Q, _ptr(qrun),
                                                    _ptr(qtime), _ptr(qwin), C.byref(o)))
        if not self._follow and self.stream is not None:   # see preintegrate_stream
            for t in ((ws,) if workspace is None else ()) + (() if one else (soff, uoff)) + (qwin,):
                t.record_stream(self.stream)
        return out, qwin

    def query_stream_host(self, stream, update_times, lin, qtime, q_k_lin=None, params=None, want=("mean",), N=None,
                          stream_offsets=None, update_offsets=None, qrun=None, pinned=True, out=None):
        """query_stream from HOST memory (cpi_query_stream_batch_host): CPU tensors in; there is no rows argument -- the running rows
        are computed on the device and stay there.  The offsets and qrun are validated.  N defaults to stream_bound() /
        streams_bound().  Returns (out, qwin) as CPU tensors; synchronous."""
        params = params or self.make_params()
        K, U, Q = stream.shape[0], update_times.shape[0], qtime.shape[0]
        one = stream_offsets is None and update_offsets is None
        soff = uoff = None
        R = 1
        if not one:
            soff = torch.as_tensor(np.asarray(stream_offsets, dtype=np.int64))
            uoff = torch.as_tensor(np.asarray(update_offsets, dtype=np.int64))
            R = soff.shape[0] - 1
        if N is None:
            N = self._stream_bound(stream, update_times) if one else self.streams_bound(stream, soff, update_times, uoff)
        self._check_f64((stream, update_times, lin, q_k_lin, qtime), cuda=False)
        assert qrun is None or (qrun.dtype == torch.int32 and qrun.shape == (Q,)), "qrun [Q] int32"
        if out is None:
            out = self._host_outputs((Q,), tuple(want), params.model, pinned)
        qwin = torch.empty((Q,), dtype=torch.int32)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_query_stream_batch_host(self.ctx, C.byref(params), R, K, _ptr(stream), _ptr(soff), U, _ptr(update_times),
                                                         _ptr(uoff), int(N), _ptr(lin), _ptr(q_k_lin), Q, _ptr(qrun), _ptr(qtime),
                                                         _ptr(qwin), C.byref(o)))
        return out, qwin

    def preintegrate_tiled_host(self, tiles, W, lin, q_k_lin=None, params=None, count=None, pinned=True, out=None):
        """Mean outputs from tiles held in HOST memory (cpi_preintegrate_tiled_batch_host: chunked upload / kernel /
        download pipeline).  CPU float64 tensors; returns CPU tensors; synchronous."""
        params = params or self.make_params()
        N = tiles.shape[1] - 1
        for t in (tiles, lin, q_k_lin, count):
            assert t is None or (not t.is_cuda and t.is_contiguous()), "inputs must be contiguous CPU tensors"
        assert tiles.shape[0] == (W + 63) // 64 and tiles.shape[2:] == (7, 64)
        if out is None:
            out = self._host_outputs((W,), ("mean",), params.model, pinned)
        o = self._outputs_struct(out)
        self._sync_stream()
        self._check(self.lib.cpi_preintegrate_tiled_batch_host(self.ctx, C.byref(params), W, N, _ptr(tiles), _ptr(count), _ptr(lin),
                                                               _ptr(q_k_lin), C.byref(o)))
        return out

    def preintegrate_tiled(self, tiles, W, lin, q_k_lin=None, params=None, count=None, out=None, bind=False):
        """Mean outputs from the tiled layout (include/cpi_amd.h: cpi_preintegrate_tiled_batch).  bind=True: returns
        (call, out) with the foreign call pre-bound, like bind_preintegrate."""
        params = params or self.make_params()
        N = tiles.shape[1] - 1
        assert tiles.is_cuda and tiles.is_contiguous() and tiles.shape[0] == (W + 63) // 64 and tiles.shape[2:] == (7, 64)
        if out is None:
            out = self.alloc_outputs(W, ("mean",), params.model)
        o = self._outputs_struct(out)
        args = (self.ctx, C.byref(params), W, N, _ptr(tiles), _ptr(count), _ptr(lin), _ptr(q_k_lin), C.byref(o))
        fn, check, sync = self.lib.cpi_preintegrate_tiled_batch, self._check, self._sync_stream

        def call():
            sync()
            rc = fn(*args)
            if rc:
                check(rc)
        call._keep = (o, params, tiles, lin, q_k_lin, count, out)
        if bind:
            return call, out
        call()
        return out

    def bind_preintegrate(self, knots, lin, q_k_lin=None, params=None, want=("mean", "jac", "cov"), first=None, count=None,
                          N=None, out=None):
        """A zero-argument callable that issues exactly this preintegrate() call again and again: the ctypes argument
        objects are built once, so a step costs one foreign call (~2 us of host time instead of ~10) -- for callers that
        re-run fixed buffers in a loop (bench.py; a C or C++ host has no such overhead to begin with).  Returns
        (call, out)."""
        params = params or self.make_params()
        W, N = self._window_shape(knots, lin, first, count, N, (q_k_lin,))
        if out is None:
            out = self.alloc_outputs(W, want, params.model)
        o = self._outputs_struct(out)
        args = (self.ctx, C.byref(params), W, N, _ptr(knots), _ptr(first), _ptr(count), _ptr(lin), _ptr(q_k_lin), C.byref(o))
        fn, check, sync = self.lib.cpi_preintegrate_batch, self._check, self._sync_stream

        def call():
            sync()
            rc = fn(*args)
            if rc:
                check(rc)
        call._keep = (o, params, knots, lin, q_k_lin, first, count, out)   # the buffers live as long as the callable
        return call, out

    # ------------------------------------------------------------------ factors
    def sqrt_information(self, P, out=None):
        """R = chol_upper(P^-1) per factor (GTSAM noiseModel::Gaussian::Covariance).  P [F,225] (dense) -> R [F,225] with zeros
        below the diagonal; P [F,120] (the packed upper triangle: outputs' P_sym) -> R_tri [F,120], the same values
        (cpi_sqrt_information_packed_batch)."""
        F, n = P.shape
        assert n in (225, 120) and P.is_contiguous(), "P must be [F,225] (dense) or [F,120] (packed upper triangle)"
        R = out if out is not None else torch.empty((F, n), dtype=torch.float64, device=self.device)
        assert R.shape == (F, n) and R.is_contiguous()
        self._sync_stream()
        fn = self.lib.cpi_sqrt_information_batch if n == 225 else self.lib.cpi_sqrt_information_packed_batch
        self._check(fn(self.ctx, F, _ptr(P), _ptr(R)))
        return R

    def factor_eval(self, model, meas, lin, q_k_lin, states, idx_i=None, idx_j=None, want_H=True, grav=DEFAULT_GRAV,
                    out=None, sqrt_info=None):
        """sqrt_info [F,225] or its packed triangle [F,120] (from sqrt_information): return the WHITENED residual / Jacobians
        (R e, R H1, R H2); the packed form reads 840 bytes less per factor and gives the same bits."""
        F = lin.shape[0]
        if out is None:
            out = {"err": torch.empty((F, 15), dtype=torch.float64, device=self.device)}
            if want_H:
                out["H1"] = torch.empty((F, 225), dtype=torch.float64, device=self.device)
                out["H2"] = torch.empty((F, 225), dtype=torch.float64, device=self.device)
        m = self._outputs_struct(meas)
        g = (C.c_double * 3)(*grav)
        self._sync_stream()
        if sqrt_info is None:
            self._check(self.lib.cpi_factor_eval_batch(self.ctx, int(model), g, F, C.byref(m), _ptr(lin), _ptr(q_k_lin),
                                                       _ptr(states), states.shape[0], _ptr(idx_i), _ptr(idx_j),
                                                       _ptr(out["err"]), _ptr(out.get("H1")), _ptr(out.get("H2"))))
        else:
            assert sqrt_info.shape == (F, 225) or sqrt_info.shape == (F, 120)
            fn = self.lib.cpi_factor_eval_whitened_batch if sqrt_info.shape[1] == 225 else self.lib.cpi_factor_eval_whitened_tri_batch
            self._check(fn(self.ctx, int(model), g, F, C.byref(m), _ptr(lin), _ptr(q_k_lin), _ptr(states), states.shape[0], _ptr(idx_i),
                           _ptr(idx_j), _ptr(sqrt_info), _ptr(out["err"]), _ptr(out.get("H1")), _ptr(out.get("H2"))))
        return out

    def factor_eval_packed(self, model, meas, lin, q_k_lin, states, idx_i=None, idx_j=None, grav=DEFAULT_GRAV, out=None):
        """State-dependent part of evaluateError only: [F,72] = err[15] + the 3x3 blocks H1(0,0), H1(6,0), H1(12,0),
        H1(0,3), R(q_GtoK), H2(0,0) (column-major) + 3 zeros; see include/cpi_amd.h.  unpack_factor() rebuilds the
        dense pair."""
        F = lin.shape[0]
        if out is None:
            out = torch.empty((F, 72), dtype=torch.float64, device=self.device)
        m = self._outputs_struct(meas)
        g = (C.c_double * 3)(*grav)
        self._sync_stream()
        self._check(self.lib.cpi_factor_eval_packed_batch(self.ctx, int(model), g, F, C.byref(m), _ptr(lin), _ptr(q_k_lin),
                                                          _ptr(states), states.shape[0], _ptr(idx_i), _ptr(idx_j), _ptr(out)))
        return out

    def factor_hessian(self, model, meas, lin, q_k_lin, states, sqrt_info, idx_i=None, idx_j=None, grav=DEFAULT_GRAV, out=None):
        """[F, 496]: packed upper triangle of the augmented information matrix [A1 A2 b]^T [A1 A2 b] with A = R H, b = -R e
        (what a GTSAM HessianFactor built from the linearised factor holds); see include/cpi_amd.h."""
        F = lin.shape[0]
        if out is None:
            out = torch.empty((F, 496), dtype=torch.float64, device=self.device)
        m = self._outputs_struct(meas)
        g = (C.c_double * 3)(*grav)
        self._sync_stream()
        assert sqrt_info.shape == (F, 225) or sqrt_info.shape == (F, 120), "sqrt_info: [F,225] dense or [F,120] packed triangle"
        fn = self.lib.cpi_factor_hessian_batch if sqrt_info.shape[1] == 225 else self.lib.cpi_factor_hessian_tri_batch
        self._check(fn(self.ctx, int(model), g, F, C.byref(m), _ptr(lin), _ptr(q_k_lin), _ptr(states), states.shape[0], _ptr(idx_i),
                       _ptr(idx_j), _ptr(sqrt_info), _ptr(out)))
        return out

    def predict(self, model, meas, states_i, idx_i=None, grav=DEFAULT_GRAV, out=None):
        F = meas["DT"].shape[0]
        xj = out if out is not None else torch.empty((F, 16), dtype=torch.float64, device=self.device)
        m = self._outputs_struct(meas)
        g = (C.c_double * 3)(*grav)
        self._sync_stream()
        self._check(self.lib.cpi_predict_batch(self.ctx, int(model), g, F, C.byref(m), _ptr(states_i), states_i.shape[0],
                                               _ptr(idx_i), _ptr(xj)))
        return xj

    # ------------------------------------------------------------------ the optimiser's trial step
    @staticmethod
    def _trial_tensor(t, cols, cuda, name, rows=None):
        assert (t.dtype == torch.float64 and t.is_contiguous() and t.is_cuda == cuda and t.dim() == 2 and t.shape[1] == cols
                and (rows is None or t.shape[0] == rows)), \
            "%s: a contiguous float64 %s tensor [%s, %d]" % (name, "CUDA" if cuda else "CPU", "S" if rows is None else rows, cols)

    def _retract(self, fn, states, delta, out, cuda):
        self._trial_tensor(states, 16, cuda, "states")
        S = states.shape[0]
        self._trial_tensor(delta, 15, cuda, "delta", S)
        if out is None:
            out = torch.empty_like(states)
        self._trial_tensor(out, 16, cuda, "out", S)
        self._sync_stream()
        self._check(fn(self.ctx, S, _ptr(states), _ptr(delta), _ptr(out)))
        return out

    def retract(self, states, delta, out=None):
        """cpi_retract_batch: out[s] = JPLNavState::retract(states[s], delta[s]) -- the map along which H1 / H2 of the factor sweeps
        are derivatives.  states [S,16] = [q bg v ba p], delta [S,15] = [dtheta bg v ba p], CUDA float64.  out=states is the
        in-place form (same bits); any other overlap is refused.  Asynchronous."""
        return self._retract(self.lib.cpi_retract_batch, states, delta, out, True)

    def retract_host(self, states, delta, out=None):
        """retract on CPU tensors (cpi_retract_batch_host): synchronous, the device form's bits."""
        return self._retract(self.lib.cpi_retract_batch_host, states, delta, out, False)

    def _local(self, fn, x, other, out, cuda):
        self._trial_tensor(x, 16, cuda, "x")
        S = x.shape[0]
        self._trial_tensor(other, 16, cuda, "other", S)
        if out is None:
            out = torch.empty((S, 15), dtype=torch.float64, device=x.device)
        self._trial_tensor(out, 15, cuda, "out", S)
        self._sync_stream()
        self._check(fn(self.ctx, S, _ptr(x), _ptr(other), _ptr(out)))
        return out

    def local_coordinates(self, x, other, out=None):
        """cpi_local_batch: xi[s] = JPLNavState::localCoordinates(x[s], other[s]) = [2 vec(other.q (x) inv(x.q)), other - x], [S,15].
        Asynchronous."""
        return self._local(self.lib.cpi_local_batch, x, other, out, True)

    def local_coordinates_host(self, x, other, out=None):
        """local_coordinates on CPU tensors (cpi_local_batch_host): synchronous, the device form's bits."""
        return self._local(self.lib.cpi_local_batch_host, x, other, out, False)

    def factor_cost_total_doubles(self, F):
        """Doubles of the workspace behind the total of factor_cost (cpi_factor_cost_total_doubles)."""
        return int(self.lib.cpi_factor_cost_total_doubles(int(F)))

    def _cost_common(self, meas, lin, q_k_lin, states, idx_i, idx_j, cuda):
        F = lin.shape[0]
        self._trial_tensor(lin, 6, cuda, "lin")
        self._trial_tensor(states, 16, cuda, "states")
        if q_k_lin is not None:
            self._trial_tensor(q_k_lin, 4, cuda, "q_k_lin", F)
        for name, t in (("idx_i", idx_i), ("idx_j", idx_j)):
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda == cuda and t.shape == (F,)), \
                "%s: a contiguous int32 %s tensor [F]" % (name, "CUDA" if cuda else "CPU")
        for k, v in meas.items():
            if not k.startswith("_"):
                assert v.dtype == torch.float64 and v.is_contiguous() and v.is_cuda == cuda and v.shape[0] == F, \
                    "meas[%r]: a contiguous float64 %s tensor of F rows" % (k, "CUDA" if cuda else "CPU")
        return F

    def factor_cost(self, model, meas, lin, q_k_lin, states, sqrt_info, idx_i=None, idx_j=None, grav=DEFAULT_GRAV, want_err=False,
                    want_total=True, out=None):
        """cpi_factor_cost_batch / _tri_batch: the cost of the F factors at `states` -- GTSAM's NoiseModelFactor::error summed over the
        graph -- without the 3.7 KB of Jacobians per factor of factor_eval.  sqrt_info [F,225] or its packed triangle [F,120] (from
        sqrt_information; same bits).  Returns a dict:
          "chi2"       [F]     |R e|^2 per factor, always
          "werr"       [F,15]  R e (want_err)
          "workspace"  [factor_cost_total_doubles(F)]  the caller-visible buffer behind the total (want_total)
          "total"      [1]     0.5 sum chi2: a view of workspace[:1] -- reading it never synchronises, and its bits do not depend on
                               the run or on want_err
        out= re-uses the tensors of an earlier call (graph capture): a dict with "chi2", with "werr" when want_err and with
        "workspace" when want_total (asserted; "total" is set to the view when missing).  A "werr" or "workspace" that out holds
        beyond the flags is written too: the keys of out say what the call fills.  Asynchronous."""
        F = self._cost_common(meas, lin, q_k_lin, states, idx_i, idx_j, True)
        assert sqrt_info.dim() == 2 and sqrt_info.shape[0] == F and sqrt_info.shape[1] in (225, 120), \
            "sqrt_info: [F,225] dense or [F,120] packed triangle"
        self._trial_tensor(sqrt_info, sqrt_info.shape[1], True, "sqrt_info", F)
        if out is None:
            out = {"chi2": torch.empty((F,), dtype=torch.float64, device=self.device)}
            if want_err:
                out["werr"] = torch.empty((F, 15), dtype=torch.float64, device=self.device)
            if want_total:
                out["workspace"] = torch.empty((self.factor_cost_total_doubles(F),), dtype=torch.float64, device=self.device)
        else:
            assert "chi2" in out and (not want_err or "werr" in out) and (not want_total or "workspace" in out), \
                "out: a dict with 'chi2', with 'werr' when want_err and with 'workspace' when want_total"
        chi2, werr, ws = out["chi2"], out.get("werr"), out.get("workspace")
        assert chi2.dtype == torch.float64 and chi2.is_cuda and chi2.is_contiguous() and chi2.shape == (F,), "out['chi2']: CUDA float64 [F]"
        if werr is not None:
            self._trial_tensor(werr, 15, True, "out['werr']", F)
        assert ws is None or (ws.dtype == torch.float64 and ws.is_cuda and ws.is_contiguous() and ws.dim() == 1
                              and ws.numel() >= self.factor_cost_total_doubles(F)), \
            "out['workspace']: CUDA float64, factor_cost_total_doubles(F) elements"
        if ws is not None:
            out["total"] = ws[:1]
        m = self._outputs_struct(meas)
        g = (C.c_double * 3)(*grav)
        self._sync_stream()
        fn = self.lib.cpi_factor_cost_batch if sqrt_info.shape[1] == 225 else self.lib.cpi_factor_cost_tri_batch
        self._check(fn(self.ctx, int(model), g, F, C.byref(m), _ptr(lin), _ptr(q_k_lin), _ptr(states), states.shape[0], _ptr(idx_i),
                       _ptr(idx_j), _ptr(sqrt_info), _ptr(chi2), _ptr(werr), _ptr(ws)))
        return out

    def factor_cost_host(self, model, meas, lin, q_k_lin, states, idx_i=None, idx_j=None, grav=DEFAULT_GRAV, want_err=False,
                         want_total=True):
        """cpi_factor_cost_batch_host on CPU tensors: GTSAM's factor.error(values) for F factors in one call.  meas holds the
        measurement with its covariance ("P_sym" [F,120] when present, else "P" [F,225]); the square-root information is
        factorised on the device.  Returns CPU tensors {"chi2", "werr" (want_err), "total" [1] (want_total)}; synchronous."""
        F = self._cost_common(meas, lin, q_k_lin, states, idx_i, idx_j, False)
        out = {"chi2": torch.empty((F,), dtype=torch.float64)}
        if want_err:
            out["werr"] = torch.empty((F, 15), dtype=torch.float64)
        if want_total:
            out["total"] = torch.empty((1,), dtype=torch.float64)
        m = self._outputs_struct(meas)
        g = (C.c_double * 3)(*grav)
        self._sync_stream()
        self._check(self.lib.cpi_factor_cost_batch_host(self.ctx, int(model), g, F, C.byref(m), _ptr(lin), _ptr(q_k_lin), _ptr(states),
                                                        states.shape[0], _ptr(idx_i), _ptr(idx_j), _ptr(out["chi2"]),
                                                        _ptr(out.get("werr")), _ptr(out.get("total"))))
        return out

    # ------------------------------------------------------------------ the step itself, for chains of IMU factors
    DAMPING = {"identity": 0, "diagonal": 1}

    def chain_solve_workspace_doubles(self, S):
        """Doubles of the workspace of chain_solve for S states (cpi_chain_solve_workspace_doubles)."""
        return int(self.lib.cpi_chain_solve_workspace_doubles(int(S)))

    @staticmethod
    def chain_indices(C, G, first=None, count=None):
        """int32 (idx_i, idx_j) of the factors of C chains for the Hessian / cost sweeps, in the order chain_solve reads them with
        ffirst=None when the chains tile the states back to back: factor k of chain c joins states first[c] + k and first[c] + k + 1.
        first [C] int64 (None: c * G), count [C] int32 states per chain (None: G; clamped into [0, G]).  Plain torch ops on the
        device of first / count (CPU when both are None)."""
        dev = first.device if first is not None else (count.device if count is not None else torch.device("cpu"))
        f = first.to(torch.int64) if first is not None else torch.arange(C, dtype=torch.int64, device=dev) * G
        n = count.to(torch.int64).clamp(0, G) if count is not None else torch.full((C,), G, dtype=torch.int64, device=dev)
        nf = (n - 1).clamp(min=0)
        k = torch.arange(max(G - 1, 0), dtype=torch.int64, device=dev)[None, :]
        idx_i = (f[:, None] + k)[k < nf[:, None]]
        return idx_i.to(torch.int32).contiguous(), (idx_i + 1).to(torch.int32).contiguous()

    @staticmethod
    def _chain_ranges(C, G, first, count, ffirst, cuda):
        """What every entry of the chain family checks of first / count / ffirst; returns C."""
        where = "CUDA" if cuda else "CPU"
        for name, t, dt in (("first", first, torch.int64), ("count", count, torch.int32), ("ffirst", ffirst, torch.int64)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.is_cuda == cuda and t.dim() == 1), \
                "%s: a contiguous %s %s tensor [C]" % (name, str(dt).split(".")[1], where)
        if C is None:
            C = next((t.shape[0] for t in (first, count, ffirst) if t is not None), None)
        assert C is not None, "C: the number of chains (or first / count / ffirst, which have it)"
        assert all(t is None or t.shape[0] == C for t in (first, count, ffirst)), "first / count / ffirst: [C]"
        assert G is not None and G >= 1, "G: the longest chain in states, >= 1"
        return int(C)

    def _chain_args(self, hess, C, G, first, count, ffirst, prior, lam, damping, out, status, cuda):
        where = "CUDA" if cuda else "CPU"
        assert damping in self.DAMPING, "damping: 'identity' or 'diagonal'"
        C = self._chain_ranges(C, G, first, count, ffirst, cuda)
        if hess is not None:
            self._trial_tensor(hess, 496, cuda, "hess")
        if prior is not None:
            self._trial_tensor(prior, 136, cuda, "prior")
        S = out.shape[0] if out is not None else (prior.shape[0] if prior is not None else C * G)
        if out is None:
            # rows of no chain are not written: they read NaN rather than whatever the allocator left there
            out = torch.full((S, 15), float("nan"), dtype=torch.float64, device=self.device if cuda else "cpu")
        self._trial_tensor(out, 15, cuda, "out", S)
        assert prior is None or prior.shape[0] == S, "prior: [S, 136] with the S of out"
        if lam is not None:
            if not torch.is_tensor(lam):
                lam = torch.full((C,), float(lam), dtype=torch.float64, device=out.device)
            elif lam.numel() == 1 and C != 1:
                lam = lam.reshape(1).expand(C).contiguous()      # torch ops on the tensor's device: no host read
            lam = lam.reshape(-1)
            assert lam.dtype == torch.float64 and lam.is_contiguous() and lam.is_cuda == cuda and lam.shape == (C,), \
                "lam: a number, or a float64 %s tensor with one element or C" % where
        assert status is None or (status.dtype == torch.int32 and status.is_contiguous() and status.is_cuda == cuda and status.shape == (C,)), \
            "status: a contiguous int32 %s tensor [C]" % where
        F = hess.shape[0] if hess is not None else 0
        return C, int(G), S, F, lam, out

    def chain_solve(self, hess, C=None, G=None, first=None, count=None, ffirst=None, prior=None, lam=None, damping="identity", out=None,
                    status=None, workspace=None):
        """cpi_chain_solve_batch: the Gauss-Newton / Levenberg-Marquardt step delta [S,15] of C chains of IMU factors -- the damped
        block-tridiagonal system of include/cpi_amd.h, solved by a block Cholesky along every chain on the rows of factor_hessian as
        they are.  hess [F,496] (None only with G == 1); chain c owns the states first[c] .. first[c] + count[c] - 1 (None: c * G
        and G) and the hess rows ffirst[c] + k (None: first[c] - c: chain_indices gives the matching idx_i / idx_j); prior None or
        [S,136] packed [Lam eta; eta^T .] per state; lam None, a number, or a CUDA float64 tensor of one element or C (expanded with
        torch ops: no host read; a Levenberg-Marquardt loop keeps it on the device); damping "identity" or "diagonal".  S comes from
        out, else prior, else C * G.  status: an int32 [C] tensor to fill (0 solved, s + 1 the block of state s was not positive
        definite, -1 the chain's factor rows leave hess); a failed chain's rows are NaN.  workspace: float64,
        chain_solve_workspace_doubles(S) elements (allocated when None; pass one for graph capture).  Rows of no chain are not written
        (NaN in a tensor this call allocates).  retract takes delta as it is.  Asynchronous."""
        C_, G_, S, F, lam, out = self._chain_args(hess, C, G, first, count, ffirst, prior, lam, damping, out, status, True)
        need = self.chain_solve_workspace_doubles(S)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.float64, device=self.device)
        assert (workspace.dtype == torch.float64 and workspace.is_cuda and workspace.is_contiguous() and workspace.dim() == 1
                and workspace.numel() >= need), "workspace: CUDA float64, chain_solve_workspace_doubles(S) elements"
        self._sync_stream()
        self._check(self.lib.cpi_chain_solve_batch(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess), _ptr(prior),
                                                   _ptr(lam), self.DAMPING[damping], _ptr(out), _ptr(status), _ptr(workspace)))
        return out

    def chain_solve_host(self, hess, C=None, G=None, first=None, count=None, ffirst=None, prior=None, lam=None, damping="identity",
                         out=None, status=None):
        """chain_solve on CPU tensors (cpi_chain_solve_batch_host): every chain's state and factor range is validated (CpiError names
        the chain), synchronous, the device form's bits."""
        C_, G_, S, F, lam, out = self._chain_args(hess, C, G, first, count, ffirst, prior, lam, damping, out, status, False)
        self._sync_stream()
        self._check(self.lib.cpi_chain_solve_batch_host(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess),
                                                        _ptr(prior), _ptr(lam), self.DAMPING[damping], _ptr(out), _ptr(status)))
        return out

    # ------------------------------------------------------------------ the covariance of what the loop converged to
    def _marginals_out(self, S, out, cross, cuda):
        dev = self.device if cuda else "cpu"
        if out is None:
            # rows of no chain are not written: they read NaN rather than whatever the allocator left there
            out = torch.full((S, 120), float("nan"), dtype=torch.float64, device=dev)
        self._trial_tensor(out, 120, cuda, "out", S)
        if cross is True:
            cross = torch.full((S, 225), float("nan"), dtype=torch.float64, device=dev)
        elif cross is False:
            cross = None
        if cross is not None:
            self._trial_tensor(cross, 225, cuda, "cross", S)
        return out, cross

    def chain_marginals(self, workspace, C=None, G=None, first=None, count=None, status=None, out=None, cross=None):
        """cpi_chain_marginals_batch: the covariance of every state of C solved chains, cov [S,120] -- Sigma[s][s] as the packed upper
        triangle in the packing of P_sym (unpack_sym gives the dense block, sqrt_information the square-root information of a prior
        carried on) -- and, with cross=True or a [S,225] tensor, Sigma[s][s+1] column-major per state (the row of a chain's last
        state is not written): returns cov, or (cov, cross).  workspace, C, G, first, count: those of the chain_solve that wrote the
        workspace.  What is inverted is the matrix that solve factorised, damping included: the covariance of the estimate comes
        from a solve with lam=None at the converged states.  status: the int32 [C] tensor the solve filled (a chain whose status is
        not 0 gets NaN rows); None vouches for every chain.  S comes from out, else cross, else first is None: C * G, else
        workspace.numel() // 360.  Rows of no chain are not written (NaN in a tensor this call allocates).  Asynchronous."""
        for name, t, dt in (("first", first, torch.int64), ("count", count, torch.int32), ("status", status, torch.int32)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.is_cuda and t.dim() == 1), \
                "%s: a contiguous %s CUDA tensor [C]" % (name, str(dt).split(".")[1])
        if C is None:
            C = next((t.shape[0] for t in (first, count, status) if t is not None), None)
        assert C is not None, "C: the number of chains (or first / count / status, which have it)"
        assert all(t is None or t.shape[0] == C for t in (first, count, status)), "first / count / status: [C]"
        assert G is not None and G >= 1, "G: the longest chain in states, >= 1"
        assert workspace.dtype == torch.float64 and workspace.is_cuda and workspace.is_contiguous() and workspace.dim() == 1, \
            "workspace: the CUDA float64 workspace of chain_solve"
        if out is not None:
            S = out.shape[0]
        elif torch.is_tensor(cross):
            S = cross.shape[0]
        else:
            S = C * G if first is None else workspace.numel() // 360
        assert workspace.numel() >= self.chain_solve_workspace_doubles(S), "workspace: chain_solve_workspace_doubles(S) elements"
        out, cross = self._marginals_out(S, out, cross, True)
        self._sync_stream()
        self._check(self.lib.cpi_chain_marginals_batch(self.ctx, C, int(G), S, _ptr(first), _ptr(count), _ptr(status), _ptr(workspace),
                                                       _ptr(out), _ptr(cross)))
        return out if cross is None else (out, cross)

    def chain_marginals_host(self, hess, C=None, G=None, first=None, count=None, ffirst=None, prior=None, cross=False, out=None,
                             status=None):
        """chain_marginals on CPU tensors (cpi_chain_marginals_batch_host): the UNDAMPED system of hess / prior (the arguments of
        chain_solve_host) is factorised on the device and inverted block by block; every chain's state and factor range is validated
        (CpiError names the chain); synchronous, the device forms' bits.  Returns cov [S,120], or (cov, cross) with cross=True or a
        [S,225] tensor; status: an int32 [C] tensor that receives the solve's codes (a failed chain's rows are NaN)."""
        C_, G_, S, F, _, _ = self._chain_args(hess, C, G, first, count, ffirst, prior, None, "identity",
                                              None if out is None else torch.empty((out.shape[0], 15), dtype=torch.float64), status, False)
        out, cross = self._marginals_out(S, out, cross, False)
        self._sync_stream()
        self._check(self.lib.cpi_chain_marginals_batch_host(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess),
                                                            _ptr(prior), _ptr(out), _ptr(cross), _ptr(status)))
        return out if cross is None else (out, cross)

    # ------------------------------------------------------------------ the window slides: the oldest states become a prior
    def _marginalize_args(self, hess, C, G, first, count, ffirst, prior, drop, out, status, cuda):
        where = "CUDA" if cuda else "CPU"
        for name, t, dt in (("first", first, torch.int64), ("count", count, torch.int32), ("ffirst", ffirst, torch.int64),
                            ("status", status, torch.int32)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.is_cuda == cuda and t.dim() == 1), \
                "%s: a contiguous %s %s tensor [C]" % (name, str(dt).split(".")[1], where)
        if C is None:
            C = next((t.shape[0] for t in (first, count, ffirst) if t is not None), None)
        assert C is not None, "C: the number of chains (or first / count / ffirst, which have it)"
        assert all(t is None or t.shape[0] == C for t in (first, count, ffirst, status)), "first / count / ffirst / status: [C]"
        assert G is not None and G >= 1, "G: the longest chain in states, >= 1"
        if hess is not None:
            self._trial_tensor(hess, 496, cuda, "hess")
        C_, G_, F = int(C), int(G), (hess.shape[0] if hess is not None else 0)
        if prior is not None:
            self._trial_tensor(prior, 136, cuda, "prior")
            S = prior.shape[0]
        else:
            S = C_ * G_ if first is None else 1 << 40        # without a prior no array has S rows: S only clips the chains
        M = 0
        if torch.is_tensor(drop):
            assert drop.dtype == torch.int32 and drop.is_contiguous() and drop.is_cuda == cuda and drop.shape == (C_,), \
                "drop: an int, or a contiguous int32 %s tensor [C]" % where
        else:
            M, drop = int(drop), None
        if out is None:
            out = torch.empty((C_, 136), dtype=torch.float64, device=self.device if cuda else "cpu")
        self._trial_tensor(out, 136, cuda, "out", C_)
        return C_, G_, S, F, M, drop, out

    def chain_marginalize(self, hess, C=None, G=None, first=None, count=None, ffirst=None, prior=None, drop=1, out=None, status=None):
        """cpi_chain_marginalize_batch: the leading drop states of every chain eliminated into a prior on the first state that stays
        -- out [C,136], row c the packed [Lam eta; eta^T .] of state drop_c of the reduced chain: the Schur complement of the
        eliminated states over the factors and priors that touch only them (include/cpi_amd.h; undamped, no workspace).  hess, C, G,
        first, count, ffirst, prior: those of chain_solve.  drop: an int for every chain, or an int32 [C] CUDA tensor; 0 <= drop <
        the chain's states.  status: an int32 [C] tensor to fill (0; s + 1: the block of eliminated state s was not positive
        definite; -1: the factor rows leave hess or drop is outside the chain); such a chain's row is NaN.  Put row c at state
        first[c] + drop_c of prior and solve first + drop, count - drop, ffirst + drop on the same arrays: the full chain's delta for
        the states that stay.  S comes from prior, else C * G.  Asynchronous."""
        C_, G_, S, F, M, drop, out = self._marginalize_args(hess, C, G, first, count, ffirst, prior, drop, out, status, True)
        self._sync_stream()
        self._check(self.lib.cpi_chain_marginalize_batch(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess), _ptr(prior),
                                                         M, _ptr(drop), _ptr(out), _ptr(status)))
        return out

    def chain_marginalize_host(self, hess, C=None, G=None, first=None, count=None, ffirst=None, prior=None, drop=1, out=None, status=None):
        """chain_marginalize on CPU tensors (cpi_chain_marginalize_batch_host): every chain's state range, factor range and drop is
        validated (CpiError names the chain), synchronous, the device form's bits."""
        C_, G_, S, F, M, drop, out = self._marginalize_args(hess, C, G, first, count, ffirst, prior, drop, out, status, False)
        self._sync_stream()
        self._check(self.lib.cpi_chain_marginalize_batch_host(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess),
                                                              _ptr(prior), M, _ptr(drop), _ptr(out), _ptr(status)))
        return out


    # ------------------------------------------------------------------ long chains: segments condensed in parallel along the chain
    def chain_condense_states(self, G, K):
        """Gr, the reduced states of a chain slot of G states cut into segments of K factors (cpi_chain_condense_states)."""
        return int(self.lib.cpi_chain_condense_states(int(G), int(K)))

    def chain_condense_workspace_doubles(self, S):
        """Doubles of the workspace of chain_condense for S states (cpi_chain_condense_workspace_doubles)."""
        return int(self.lib.cpi_chain_condense_workspace_doubles(int(S)))

    def chain_condense_buffers(self, C, G, S, K, cuda=True):
        """Every buffer chain_solve_segmented needs for C chains of at most G states over S state rows at segment length K, as a dict
        (allocate once, pass as buffers=: the three calls then allocate nothing and capture into a graph)."""
        dev = self.device if cuda else "cpu"
        Gr = self.chain_condense_states(G, K)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device=dev)
        return dict(rhess=f64(C * (Gr - 1), 496), rprior=f64(C * Gr, 136), rcount=i32(C), seg_status=i32(C * (Gr - 1)),
                    workspace=f64(self.chain_condense_workspace_doubles(S)), rdelta=f64(C * Gr, 15), status=i32(C),
                    solve_workspace=f64(self.chain_solve_workspace_doubles(C * Gr)))

    def _condense_args(self, hess, K, C, G, first, count, ffirst, prior, lam, damping, S, rhess, rprior, rcount, status, workspace, cuda):
        where = "CUDA" if cuda else "CPU"
        dev = self.device if cuda else "cpu"
        assert damping in self.DAMPING, "damping: 'identity' or 'diagonal'"
        assert int(K) >= 1, "K: the factors of a segment, >= 1"
        C = self._chain_ranges(C, G, first, count, ffirst, cuda)
        G, K = int(G), int(K)
        if hess is not None:
            self._trial_tensor(hess, 496, cuda, "hess")
        if prior is not None:
            self._trial_tensor(prior, 136, cuda, "prior")
        S = int(S) if S is not None else (prior.shape[0] if prior is not None else C * G)
        assert prior is None or prior.shape[0] == S, "prior: [S, 136]"
        if lam is not None:
            if not torch.is_tensor(lam):
                lam = torch.full((C,), float(lam), dtype=torch.float64, device=dev)
            elif lam.numel() == 1 and C != 1:
                lam = lam.reshape(1).expand(C).contiguous()      # torch ops on the tensor's device: no host read
            lam = lam.reshape(-1)
            assert lam.dtype == torch.float64 and lam.is_contiguous() and lam.is_cuda == cuda and lam.shape == (C,), \
                "lam: a number, or a float64 %s tensor with one element or C" % where
        Gr = self.chain_condense_states(G, K)
        if rhess is None:
            rhess = torch.empty((C * (Gr - 1), 496), dtype=torch.float64, device=dev)
        if rprior is None:
            rprior = torch.empty((C * Gr, 136), dtype=torch.float64, device=dev)
        if rcount is None:
            rcount = torch.zeros((C,), dtype=torch.int32, device=dev)
        self._trial_tensor(rhess, 496, cuda, "rhess", C * (Gr - 1))
        self._trial_tensor(rprior, 136, cuda, "rprior", C * Gr)
        for name, t, rows in (("rcount", rcount, C), ("status", status, C * (Gr - 1))):
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda == cuda and t.shape == (rows,)), \
                "%s: a contiguous int32 %s tensor [%d]" % (name, where, rows)
        need = self.chain_condense_workspace_doubles(S)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.float64, device=dev)
        assert (workspace.dtype == torch.float64 and workspace.is_cuda == cuda and workspace.is_contiguous() and workspace.dim() == 1
                and workspace.numel() >= need), "workspace: %s float64, chain_condense_workspace_doubles(S) elements" % where
        F = hess.shape[0] if hess is not None else 0
        return C, G, S, F, K, lam, Gr, rhess, rprior, rcount, workspace

    def chain_condense(self, hess, K, C=None, G=None, first=None, count=None, ffirst=None, prior=None, lam=None, damping="identity", S=None,
                       rhess=None, rprior=None, rcount=None, status=None, workspace=None):
        """cpi_chain_condense_batch: every chain cut into segments of K factors and the states between the two ends of each segment
        eliminated, one 16-lane group per segment -- parallel ALONG the chain.  hess, C, G, first, count, ffirst, prior, lam, damping:
        those of chain_solve (the damping is baked into the reduced system).  Returns (rhess [C (Gr - 1), 496], rprior [C Gr, 136],
        rcount [C] int32, Gr, workspace): the reduced chains in the tile layout, for chain_solve(rhess, C=C, G=Gr, count=rcount,
        prior=rprior) with lam=None, and the records chain_expand reads.  S (the state rows) comes from prior, else C * G.  status:
        an int32 [C (Gr - 1)] tensor to fill, per segment slot (0; s + 1: the block of interior state s of the chain was not positive
        definite; -1: the factor rows leave hess); such a segment's rhess row is NaN.  Rows of reduced slots beyond rcount[c] are not
        written.  Pass rhess, rprior, rcount and workspace (chain_condense_workspace_doubles(S) elements) for graph capture.
        Asynchronous."""
        C_, G_, S_, F, K_, lam, Gr, rhess, rprior, rcount, workspace = self._condense_args(
            hess, K, C, G, first, count, ffirst, prior, lam, damping, S, rhess, rprior, rcount, status, workspace, True)
        self._sync_stream()
        self._check(self.lib.cpi_chain_condense_batch(self.ctx, C_, G_, S_, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess), _ptr(prior),
                                                      _ptr(lam), self.DAMPING[damping], K_, _ptr(rhess), _ptr(rprior), _ptr(rcount),
                                                      _ptr(status), _ptr(workspace)))
        return rhess, rprior, rcount, Gr, workspace

    def chain_condense_host(self, hess, K, C=None, G=None, first=None, count=None, ffirst=None, prior=None, lam=None, damping="identity",
                            S=None, rhess=None, rprior=None, rcount=None, status=None, workspace=None):
        """chain_condense on CPU tensors (cpi_chain_condense_batch_host): every chain's state and factor range is validated (CpiError
        names the chain), synchronous, the device form's bits; the workspace comes back as a CPU tensor for chain_expand_host."""
        C_, G_, S_, F, K_, lam, Gr, rhess, rprior, rcount, workspace = self._condense_args(
            hess, K, C, G, first, count, ffirst, prior, lam, damping, S, rhess, rprior, rcount, status, workspace, False)
        self._sync_stream()
        self._check(self.lib.cpi_chain_condense_batch_host(self.ctx, C_, G_, S_, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(hess),
                                                           _ptr(prior), _ptr(lam), self.DAMPING[damping], K_, _ptr(rhess), _ptr(rprior),
                                                           _ptr(rcount), _ptr(status), _ptr(workspace)))
        return rhess, rprior, rcount, Gr, workspace

    def _expand_args(self, rdelta, workspace, K, C, G, first, count, out, S, cuda):
        where = "CUDA" if cuda else "CPU"
        assert int(K) >= 1, "K: the factors of a segment, >= 1"
        C = self._chain_ranges(C, G, first, count, None, cuda)
        G, K = int(G), int(K)
        Gr = self.chain_condense_states(G, K)
        self._trial_tensor(rdelta, 15, cuda, "rdelta", C * Gr)
        S = int(S) if S is not None else (out.shape[0] if out is not None else C * G)
        if out is None:
            # rows of no chain are not written: they read NaN rather than whatever the allocator left there
            out = torch.full((S, 15), float("nan"), dtype=torch.float64, device=self.device if cuda else "cpu")
        self._trial_tensor(out, 15, cuda, "out", S)
        assert (workspace.dtype == torch.float64 and workspace.is_cuda == cuda and workspace.is_contiguous() and workspace.dim() == 1
                and workspace.numel() >= self.chain_condense_workspace_doubles(S)), \
            "workspace: the %s float64 workspace of chain_condense" % where
        return C, G, S, K, out

    def chain_expand(self, rdelta, workspace, K, C=None, G=None, first=None, count=None, out=None, S=None):
        """cpi_chain_expand_batch: the reduced solve's delta rows rdelta [C Gr, 15] copied to the segment ends and substituted back into
        the interiors of every segment, one 16-lane group per segment.  workspace, K, C, G, first, count: those of the chain_condense
        that wrote the workspace.  Returns delta [S, 15] (S from out, else C * G); rows of no chain are not written (NaN in a tensor
        this call allocates); a chain whose reduced solve failed is NaN in every row.  Asynchronous."""
        C_, G_, S_, K_, out = self._expand_args(rdelta, workspace, K, C, G, first, count, out, S, True)
        self._sync_stream()
        self._check(self.lib.cpi_chain_expand_batch(self.ctx, C_, G_, S_, _ptr(first), _ptr(count), K_, _ptr(rdelta), _ptr(workspace), _ptr(out)))
        return out

    def chain_expand_host(self, rdelta, workspace, K, C=None, G=None, first=None, count=None, out=None, S=None):
        """chain_expand on CPU tensors (cpi_chain_expand_batch_host): every chain's state range is validated, synchronous, the device
        form's bits."""
        C_, G_, S_, K_, out = self._expand_args(rdelta, workspace, K, C, G, first, count, out, S, False)
        self._sync_stream()
        self._check(self.lib.cpi_chain_expand_batch_host(self.ctx, C_, G_, S_, _ptr(first), _ptr(count), K_, _ptr(rdelta), _ptr(workspace), _ptr(out)))
        return out

    def chain_solve_segmented(self, hess, K, C=None, G=None, first=None, count=None, ffirst=None, prior=None, lam=None, damping="identity",
                              out=None, status=None, buffers=None):
        """chain_solve for LONG chains, in three calls on the stream: chain_condense at segment length K, chain_solve of the reduced
        chains (lam=None: the damping is in the reduced system), chain_expand.  Arguments as chain_solve.  Returns (delta [S, 15],
        status [C] int32): the reduced solve's status -- 0, or j + 1 for the REDUCED state j whose block was not positive definite,
        which is also what a failed or refused segment causes (buffers["seg_status"] says which); such a chain's rows are NaN.
        buffers: the dict of chain_condense_buffers(C, G, S, K) (allocated when None); with it, a tensor lam, out and status given,
        nothing is allocated and the three calls capture into one graph.  Asynchronous."""
        C_ = self._chain_ranges(C, G, first, count, ffirst, True)
        S = out.shape[0] if out is not None else (prior.shape[0] if prior is not None else C_ * int(G))
        b = buffers if buffers is not None else self.chain_condense_buffers(C_, G, S, K)
        if status is None:
            status = b["status"]
        rhess, rprior, rcount, Gr, ws = self.chain_condense(hess, K, C=C_, G=G, first=first, count=count, ffirst=ffirst, prior=prior, lam=lam,
                                                            damping=damping, S=S, rhess=b["rhess"], rprior=b["rprior"], rcount=b["rcount"],
                                                            status=b["seg_status"], workspace=b["workspace"])
        self.chain_solve(rhess if Gr > 1 else None, C=C_, G=Gr, count=rcount, prior=rprior, out=b["rdelta"], status=status,
                         workspace=b["solve_workspace"])
        out = self.chain_expand(b["rdelta"], ws, K, C=C_, G=G, first=first, count=count, out=out, S=S)
        return out, status

    # ------------------------------------------------------------------ the Levenberg-Marquardt step per chain
    LM_DEFAULTS = (0.1, 10.0, 0.0, 1e5, 1e-5, 1e-5)     # cpi_lm_params NULL: the defaults of GTSAM's LevenbergMarquardtParams
    LM_RUNNING, LM_CONVERGED, LM_GAVE_UP = 0, 1, 2

    @staticmethod
    def _lm_params(params):
        """None (the library's defaults), a dict with any of lam_down, lam_up, lam_min, lam_max, abs_tol, rel_tol, or six numbers."""
        if params is None:
            return None
        if isinstance(params, CpiLmParams):
            return params
        names = [n for n, _ in CpiLmParams._fields_]
        vals = dict(zip(names, Engine.LM_DEFAULTS))
        if isinstance(params, dict):
            assert set(params) <= set(names), "params: keys among %s" % ", ".join(names)
            vals.update(params)
        else:
            assert len(params) == 6, "params: None, a dict, or the six numbers of cpi_lm_params"
            vals = dict(zip(names, params))
        p = CpiLmParams()
        for n in names:
            setattr(p, n, float(vals[n]))
        return p

    @staticmethod
    def _lm_vector(t, n, dt, cuda, name):
        assert t.dtype == dt and t.is_contiguous() and t.is_cuda == cuda and t.shape == (n,), \
            "%s: a contiguous %s %s tensor [%d]" % (name, str(dt).split(".")[1], "CUDA" if cuda else "CPU", n)

    def _prior_relinearize(self, fn, states, anchor, prior0, idx, out, pcost, want_prior, want_cost, cuda):
        self._trial_tensor(states, 16, cuda, "states")
        S, P = states.shape[0], anchor.shape[0]
        self._trial_tensor(anchor, 16, cuda, "anchor")
        self._trial_tensor(prior0, 136, cuda, "prior0", P)
        if idx is not None:
            self._lm_vector(idx, P, torch.int32, cuda, "idx")
        else:
            assert P <= S, "idx=None: record p belongs to state p, so P <= S"
        dev = states.device
        # rows of states without a record are not written: zeros in what this call allocates (no prior there, no cost)
        if out is None and want_prior:
            out = torch.zeros((S, 136), dtype=torch.float64, device=dev)
        if pcost is None and want_cost:
            pcost = torch.zeros((S,), dtype=torch.float64, device=dev)
        assert out is not None or pcost is not None, "at least one of the prior rows and pcost"
        if out is not None:
            self._trial_tensor(out, 136, cuda, "out", S)
        if pcost is not None:
            self._lm_vector(pcost, S, torch.float64, cuda, "pcost")
        self._sync_stream()
        self._check(fn(self.ctx, S, P, _ptr(idx), _ptr(states), _ptr(anchor), _ptr(prior0), _ptr(out), _ptr(pcost)))
        return out, pcost

    def prior_relinearize(self, states, anchor, prior0, idx=None, out=None, pcost=None, want_prior=True, want_cost=True):
        """cpi_prior_relinearize_batch: the priors of P records at the current states and their cost.  states [S,16]; anchor [P,16] the
        state each prior was linearised at; prior0 [P,136] = [Lam eta0; . .] (a row of chain_marginalize as it is; eta0 = 0 for a
        Gaussian centred on anchor); idx None (record p belongs to state p) or int32 [P] (an index outside [0, S) skips the record).
        Returns (prior [S,136], pcost [S]): row s = [Lam, eta = eta0 + Lam xi, 0] with xi = local_coordinates(states[s], anchor[p]) --
        what chain_solve takes as prior --, pcost[s] = 0.5 xi^T Lam xi + eta0^T xi.  out= / pcost= re-use tensors (graph capture);
        want_prior=False / want_cost=False leave that output out (None is returned in its place) unless a tensor is given for it.
        Rows of states without a record are not written: zeros in what this call allocates.  Asynchronous."""
        return self._prior_relinearize(self.lib.cpi_prior_relinearize_batch, states, anchor, prior0, idx, out, pcost, want_prior, want_cost, True)

    def prior_relinearize_host(self, states, anchor, prior0, idx=None, out=None, pcost=None, want_prior=True, want_cost=True):
        """prior_relinearize on CPU tensors (cpi_prior_relinearize_batch_host): synchronous, the device form's bits."""
        return self._prior_relinearize(self.lib.cpi_prior_relinearize_batch_host, states, anchor, prior0, idx, out, pcost, want_prior, want_cost,
                                       False)

    def _lm_sizes(self, C, G, first, count, ffirst, chi2, pcost, S, cuda):
        C_ = self._chain_ranges(C, G, first, count, ffirst, cuda)
        if chi2 is not None:
            self._lm_vector(chi2, chi2.shape[0] if chi2.dim() == 1 else -1, torch.float64, cuda, "chi2")
        if pcost is not None:
            self._lm_vector(pcost, pcost.shape[0] if pcost.dim() == 1 else -1, torch.float64, cuda, "pcost")
        if S is None:
            S = pcost.shape[0] if pcost is not None else (C_ * int(G) if first is None else None)
        assert S is not None, "S: the number of state rows -- from pcost, from C * G when first is None, else the caller's"
        assert pcost is None or pcost.shape[0] == S, "pcost: [S]"
        return C_, int(G), int(S), (chi2.shape[0] if chi2 is not None else 0)

    def _chain_cost(self, fn, chi2, pcost, C, G, first, count, ffirst, S, out, cuda):
        C_, G_, S, F = self._lm_sizes(C, G, first, count, ffirst, chi2, pcost, S, cuda)
        if out is None:
            out = torch.empty((C_,), dtype=torch.float64, device=self.device if cuda else "cpu")
        self._lm_vector(out, C_, torch.float64, cuda, "out")
        self._sync_stream()
        self._check(fn(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), _ptr(chi2), _ptr(pcost), _ptr(out)))
        return out

    def chain_cost(self, chi2, pcost=None, C=None, G=None, first=None, count=None, ffirst=None, S=None, out=None):
        """cpi_chain_cost_batch: cost [C], cost[c] = 0.5 sum of the chain's chi2 rows + the sum of its pcost rows -- the objective per
        chain, in a fixed summation shape (the same inputs give the same bits, whatever C or the chain's position).  chi2 [F] from
        factor_cost (None only with G == 1), pcost None or [S] from prior_relinearize; C, G, first, count, ffirst: those of
        chain_solve.  S, the number of state rows the chains are clipped to: pcost's rows, else C * G when first is None, else the
        caller's S=.  A chain without states gives 0, one whose factor rows leave chi2 gives NaN.  Asynchronous."""
        return self._chain_cost(self.lib.cpi_chain_cost_batch, chi2, pcost, C, G, first, count, ffirst, S, out, True)

    def chain_cost_host(self, chi2, pcost=None, C=None, G=None, first=None, count=None, ffirst=None, S=None, out=None):
        """chain_cost on CPU tensors (cpi_chain_cost_batch_host): every chain's state and factor range is validated (CpiError names the
        chain), synchronous, the device form's bits."""
        return self._chain_cost(self.lib.cpi_chain_cost_batch_host, chi2, pcost, C, G, first, count, ffirst, S, out, False)

    def _chain_accept(self, fn, chi2_new, pcost_new, trial, cost, states, lam, phase, C, G, first, count, ffirst, chi2, accepted, params, cuda):
        self._trial_tensor(states, 16, cuda, "states")
        S = states.shape[0]
        self._trial_tensor(trial, 16, cuda, "trial", S)
        C_, G_, S, F = self._lm_sizes(C, G, first, count, ffirst, chi2_new, pcost_new, S, cuda)
        assert pcost_new is None or pcost_new.shape[0] == S, "pcost_new: [S] with the S of states"
        for name, t, dt in (("cost", cost, torch.float64), ("lam", lam, torch.float64), ("phase", phase, torch.int32)):
            self._lm_vector(t, C_, dt, cuda, name)
        if accepted is not None:
            self._lm_vector(accepted, C_, torch.int32, cuda, "accepted")
        if chi2 is not None:
            self._lm_vector(chi2, F, torch.float64, cuda, "chi2")
        p = self._lm_params(params)
        self._sync_stream()
        self._check(fn(self.ctx, C_, G_, S, F, _ptr(first), _ptr(count), _ptr(ffirst), None if p is None else byref(p), _ptr(chi2_new),
                       _ptr(pcost_new), _ptr(trial), _ptr(cost), _ptr(states), _ptr(chi2), _ptr(lam), _ptr(phase), _ptr(accepted)))
        return accepted

    def chain_accept(self, chi2_new, pcost_new, trial, cost, states, lam, phase, C=None, G=None, first=None, count=None, ffirst=None,
                     chi2=None, accepted=None, params=None):
        """cpi_chain_accept_batch: the decision of a Levenberg-Marquardt step, per chain and on the device.  chi2_new [F] / pcost_new
        (None or [S]) / trial [S,16]: the trial's; cost [C], states [S,16], lam [C], phase [C] int32 are updated IN PLACE, chi2 [F]
        too when given.  A running chain (phase 0) whose trial cost -- the value chain_cost gives, same bits -- is below cost[c] takes
        the trial's rows, the new cost and lam * lam_down (not below lam_min); otherwise lam * lam_up, or phase LM_GAVE_UP once that
        passes lam_max; phase LM_CONVERGED when the decrease (or the rejected difference) is inside abs_tol or rel_tol * |cost|.  A NaN
        cost is a rejection.  A chain whose phase is not 0 is left alone.  params: None (the library's defaults: 0.1, 10, 0, 1e5, 1e-5,
        1e-5), a dict with any of lam_down, lam_up, lam_min, lam_max, abs_tol, rel_tol, or the six numbers.  accepted: an int32 [C]
        tensor to fill with 1 / 0, which is also what is returned.  Asynchronous."""
        return self._chain_accept(self.lib.cpi_chain_accept_batch, chi2_new, pcost_new, trial, cost, states, lam, phase, C, G, first, count,
                                  ffirst, chi2, accepted, params, True)

    def chain_accept_host(self, chi2_new, pcost_new, trial, cost, states, lam, phase, C=None, G=None, first=None, count=None, ffirst=None,
                          chi2=None, accepted=None, params=None):
        """chain_accept on CPU tensors (cpi_chain_accept_batch_host): every chain's state and factor range is validated (CpiError names
        the chain), synchronous, the device form's bits."""
        return self._chain_accept(self.lib.cpi_chain_accept_batch_host, chi2_new, pcost_new, trial, cost, states, lam, phase, C, G, first,
                                  count, ffirst, chi2, accepted, params, False)

    # ------------------------------------------------------------------ absolute measurements of states
    FIX_KINDS = {"position": 0, "velocity": 1, "orientation": 2, "pose": 3}
    _FIX_Z, _FIX_R = (3, 3, 4, 7), (6, 6, 6, 21)

    @staticmethod
    def fix_offsets(idx, S):
        """mfirst [S + 1] int64 for cpi_state_fix_batch from a NON-DECREASING integer tensor idx [M], idx[m] the state of fix m: state s
        owns the fixes mfirst[s] .. mfirst[s + 1] - 1.  Computed on idx's device with searchsorted: no host read, so nothing is checked --
        an index that decreases, is below 0 or is S or more is the caller's error: such fixes are counted to state 0 or to no state
        and the offsets no longer describe idx (the entry itself stays inside its arrays whatever mfirst holds)."""
        assert idx.dim() == 1 and not idx.is_floating_point(), "idx: an integer tensor [M], non-decreasing"
        return torch.searchsorted(idx.contiguous(), torch.arange(int(S) + 1, dtype=idx.dtype, device=idx.device)).to(torch.int64)

    def _state_fix(self, fn, states, kind, z, R, mfirst, weight, base, pcost_base, out, pcost, chi2, want_rows, want_cost, cuda):
        k = self.FIX_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
        assert k in (0, 1, 2, 3), "kind: 'position', 'velocity', 'orientation', 'pose' or CPI_FIX_* (0 .. 3)"
        self._trial_tensor(states, 16, cuda, "states")
        S, M = states.shape[0], z.shape[0]
        self._trial_tensor(z, self._FIX_Z[k], cuda, "z")
        self._trial_tensor(R, self._FIX_R[k], cuda, "R", M)
        self._lm_vector(mfirst, S + 1, torch.int64, cuda, "mfirst")
        if weight is not None:
            self._lm_vector(weight, M, torch.float64, cuda, "weight")
        if base is not None:
            self._trial_tensor(base, 136, cuda, "base", S)
        if pcost_base is not None:
            self._lm_vector(pcost_base, S, torch.float64, cuda, "pcost_base")
        dev = states.device
        if out is None and want_rows:
            out = torch.empty((S, 136), dtype=torch.float64, device=dev)      # every row is written
        if pcost is None and want_cost:
            pcost = torch.empty((S,), dtype=torch.float64, device=dev)
        assert out is not None or pcost is not None or chi2 is not None, "at least one of the rows, pcost and chi2"
        if out is not None:
            self._trial_tensor(out, 136, cuda, "out", S)
        if pcost is not None:
            self._lm_vector(pcost, S, torch.float64, cuda, "pcost")
        if chi2 is not None:
            self._lm_vector(chi2, M, torch.float64, cuda, "chi2")
        self._sync_stream()
        self._check(fn(self.ctx, S, M, k, _ptr(mfirst), _ptr(states), _ptr(z), _ptr(R), _ptr(weight), _ptr(base), _ptr(pcost_base), _ptr(out),
                       _ptr(pcost), _ptr(chi2)))
        return out, pcost

    def state_fix(self, states, kind, z, R, mfirst, weight=None, base=None, pcost_base=None, out=None, pcost=None, chi2=None, want_rows=True,
                  want_cost=True):
        """cpi_state_fix_batch: absolute measurements of states added to their rows [Lam eta] and to their cost.  states [S,16]; kind
        'position' (z [M,3] = p), 'velocity' (z [M,3] = v), 'orientation' (z [M,4], a JPL quaternion as in a state row) or 'pose'
        (z [M,7], q then p), or the enum value 0 .. 3; R [M,6] ([M,21] for a pose): the upper-triangular square-root information of
        every fix in the packing of R_tri (pack_tri of a d x d upper triangle); mfirst int64 [S+1]: state s owns the fixes mfirst[s] ..
        mfirst[s+1] - 1 (fix_offsets makes it from the state index of every fix); weight None or [M].  Returns (rows [S,136], pcost
        [S]): rows[s] = base[s] (or 0) + sum w R^T R on the fixed tangent rows with eta += w R^T R e -- what chain_solve takes as prior
        --, pcost[s] = pcost_base[s] (or 0) + sum 0.5 w |R e|^2.  Every state is written, never in place: chain a second sensor, or
        the carried prior of prior_relinearize, through base= / pcost_base=.  chi2= an [M] tensor to fill with |R e|^2 of every fix
        WITHOUT the weight (a gate).  out= / pcost= re-use tensors (graph capture); want_rows=False / want_cost=False leave that output
        out (None is returned in its place) unless a tensor is given for it; without rows no row is read or written.  Asynchronous."""
        return self._state_fix(self.lib.cpi_state_fix_batch, states, kind, z, R, mfirst, weight, base, pcost_base, out, pcost, chi2, want_rows,
                               want_cost, True)

    def state_fix_host(self, states, kind, z, R, mfirst, weight=None, base=None, pcost_base=None, out=None, pcost=None, chi2=None, want_rows=True,
                       want_cost=True):
        """state_fix on CPU tensors (cpi_state_fix_batch_host): mfirst is validated (CpiError names the state), synchronous, the device
        form's bits."""
        return self._state_fix(self.lib.cpi_state_fix_batch_host, states, kind, z, R, mfirst, weight, base, pcost_base, out, pcost, chi2,
                               want_rows, want_cost, False)

    def _lm_fixes(self, x, fixes, pair, base, rows):
        """The fixes of chain_lm in list order at the states x, ping-pong through the two buffers of pair (the entry is never in place):
        rows [S,136] on top of base when rows, else pcost [S] on top of base.  Returns the tensor the last call wrote."""
        for k, f in enumerate(fixes):
            dst = pair[k % 2]
            if rows:
                self.state_fix(x, f["kind"], f["z"], f["R"], f["mfirst"], weight=f.get("weight"), base=base, out=dst, want_cost=False)
            else:
                self.state_fix(x, f["kind"], f["z"], f["R"], f["mfirst"], weight=f.get("weight"), pcost_base=base, pcost=dst, want_rows=False)
            base = dst
        return base

    # ------------------------------------------------------------------ measurements between the two states of a factor
    BETWEEN_KINDS = {"position": 0, "orientation": 1, "pose": 2}
    _BETWEEN_Z, _BETWEEN_R = (3, 4, 7), (6, 6, 21)

    def _state_between(self, fn, states, kind, z, R, mfirst, idx_i, idx_j, weight, hess_base, chi2_base, out, chi2, chi2_m, want_rows, want_cost,
                       cuda):
        k = self.BETWEEN_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
        assert k in (0, 1, 2), "kind: 'position', 'orientation', 'pose' or CPI_BETWEEN_* (0 .. 2)"
        self._trial_tensor(states, 16, cuda, "states")
        S, M, F = states.shape[0], z.shape[0], mfirst.shape[0] - 1
        self._trial_tensor(z, self._BETWEEN_Z[k], cuda, "z")
        self._trial_tensor(R, self._BETWEEN_R[k], cuda, "R", M)
        self._lm_vector(mfirst, F + 1, torch.int64, cuda, "mfirst")
        for name, idx in (("idx_i", idx_i), ("idx_j", idx_j)):
            if idx is not None:
                self._lm_vector(idx, F, torch.int32, cuda, name)
        if weight is not None:
            self._lm_vector(weight, M, torch.float64, cuda, "weight")
        if hess_base is not None:
            self._trial_tensor(hess_base, 496, cuda, "hess_base", F)
        if chi2_base is not None:
            self._lm_vector(chi2_base, F, torch.float64, cuda, "chi2_base")
        dev = states.device
        if out is None and want_rows:
            out = torch.empty((F, 496), dtype=torch.float64, device=dev)      # every row is written
        if chi2 is None and want_cost:
            chi2 = torch.empty((F,), dtype=torch.float64, device=dev)
        assert out is not None or chi2 is not None or chi2_m is not None, "at least one of the rows, chi2 and chi2_m"
        if out is not None:
            self._trial_tensor(out, 496, cuda, "out", F)
        if chi2 is not None:
            self._lm_vector(chi2, F, torch.float64, cuda, "chi2")
        if chi2_m is not None:
            self._lm_vector(chi2_m, M, torch.float64, cuda, "chi2_m")
        if F == 0:                                                            # a no-op: empty tensors have no address to pass
            return out, chi2
        self._sync_stream()
        self._check(fn(self.ctx, F, M, k, _ptr(mfirst), _ptr(states), S, _ptr(idx_i), _ptr(idx_j), _ptr(z), _ptr(R), _ptr(weight), _ptr(hess_base),
                       _ptr(chi2_base), _ptr(out), _ptr(chi2), _ptr(chi2_m)))
        return out, chi2

    def state_between(self, states, kind, z, R, mfirst, idx_i=None, idx_j=None, weight=None, hess_base=None, chi2_base=None, out=None, chi2=None,
                      chi2_m=None, want_rows=True, want_cost=True):
        """cpi_state_between_batch: measurements between the two consecutive states of every IMU factor (odometry) added to the factor's
        row of factor_hessian and to its chi2.  states [S,16]; kind 'position' (z [M,3]: the position of state j in the body frame of
        state i), 'orientation' (z [M,4]: the JPL quaternion q_j (x) inv(q_i)) or 'pose' (z [M,7], q then p), or the enum value 0 .. 2;
        R [M,6] ([M,21] for a pose): the upper-triangular square-root information in the packing of R_tri; mfirst int64 [F+1]: factor f
        owns the measurements mfirst[f] .. mfirst[f+1] - 1 (fix_offsets makes it from the factor index of every measurement); idx_i /
        idx_j int32 [F] as factor_hessian takes them (None: f and f + 1); weight None or [M].  Returns (rows [F,496], chi2 [F]):
        rows[f] = hess_base[f] (or 0) + sum w [A | b]^T [A | b] on the touched columns, chi2[f] = chi2_base[f] (or 0) + sum w |R e|^2.
        IN PLACE: out=hess_base and chi2=chi2_base (the same tensors) are allowed and touch only what the measurements touch.  chi2_m=
        an [M] tensor to fill with |R e|^2 of every measurement WITHOUT the weight (a gate).  want_rows=False / want_cost=False leave
        that output out (None is returned in its place) unless a tensor is given for it; without rows no row is read or written.
        Asynchronous."""
        return self._state_between(self.lib.cpi_state_between_batch, states, kind, z, R, mfirst, idx_i, idx_j, weight, hess_base, chi2_base, out,
                                   chi2, chi2_m, want_rows, want_cost, True)

    def state_between_host(self, states, kind, z, R, mfirst, idx_i=None, idx_j=None, weight=None, hess_base=None, chi2_base=None, out=None,
                           chi2=None, chi2_m=None, want_rows=True, want_cost=True):
        """state_between on CPU tensors (cpi_state_between_batch_host): mfirst and the indices are validated (CpiError names the factor),
        synchronous, the device form's bits."""
        return self._state_between(self.lib.cpi_state_between_batch_host, states, kind, z, R, mfirst, idx_i, idx_j, weight, hess_base, chi2_base,
                                   out, chi2, chi2_m, want_rows, want_cost, False)

    def _lm_betweens(self, x, betweens, idx_i, idx_j, hess, chi2):
        """The betweens of chain_lm in list order at the states x, IN PLACE: onto the rows hess [F,496] when given, else onto chi2 [F]."""
        for b in betweens:
            if hess is not None:
                self.state_between(x, b["kind"], b["z"], b["R"], b["mfirst"], idx_i, idx_j, weight=b.get("weight"), hess_base=hess, out=hess,
                                   want_cost=False)
            else:
                self.state_between(x, b["kind"], b["z"], b["R"], b["mfirst"], idx_i, idx_j, weight=b.get("weight"), chi2_base=chi2, chi2=chi2,
                                   want_rows=False)

    def chain_lm(self, model, meas, lin, q_k_lin, states, R_tri, C, G, first=None, count=None, ffirst=None, idx_i=None, idx_j=None,
                 prior0=None, anchor=None, prior_idx=None, lam=1e-3, iterations=10, params=None, damping="diagonal", grav=DEFAULT_GRAV,
                 cost_history=None, buffers=None, init=True, fixes=None, betweens=None):
        """Levenberg-Marquardt on C chains of IMU factors, every chain with a lambda, a cost and a phase of its own: the loop of
        INTEGRATION.md 3p issued eagerly -- a thin composition of the entries, no kernel of its own, no host read, every buffer
        allocated before the first iteration.  Before the loop (init): factor_cost, prior_relinearize and chain_cost at `states`; per
        iteration: prior_relinearize(states) -> factor_hessian -> chain_solve -> retract -> factor_cost(trial) ->
        prior_relinearize(trial, pcost only) -> chain_accept.
          meas, lin, q_k_lin, R_tri, idx_i, idx_j   the F factors as factor_hessian / factor_cost take them (idx None: chain_indices)
          states [S,16]                             updated IN PLACE (an accepted chain's rows are replaced)
          prior0 / anchor / prior_idx               the priors as prior_relinearize takes them; None: no priors
          fixes                                     None or a list of dicts with kind, z, R, mfirst and optionally weight, as state_fix
                                                    takes them: absolute measurements of the states.  Every prior_relinearize of the
                                                    loop is followed by the fixes in list order -- rows before factor_hessian, pcost
                                                    only in the two cost evaluations
          betweens                                  None or a list of dicts with kind, z, R, mfirst and optionally weight, as
                                                    state_between takes them: measurements between the two states of the factors
                                                    (mfirst indexes the F factors).  Issued IN PLACE in list order after every
                                                    factor_hessian (onto the rows) and after every factor_cost (onto chi2, the current
                                                    and the trial one) with the loop's idx_i / idx_j; no buffer of
                                                    their own.  Without them the launches are those of a call without the argument
          lam                                       the initial lambda: a number, or a float64 CUDA tensor [C] that is updated in place
          cost_history                              None or a float64 CUDA tensor [iterations + 1, C]: row 0 the initial cost, row i
                                                    the cost after iteration i (device copies; nothing is read on the host)
          buffers                                   None or a dict: filled with the buffers of the first call and re-used by later ones
                                                    (init=False skips the part before the loop: one iteration under graph capture).
                                                    Its keys are interface: "cost", "lam" [C] float64, "phase", "accepted", "status"
                                                    [C] int32 -- what the loop keeps per chain and a caller may read or reset --,
                                                    "chi2", "chi2_new" [F], "hess" [F,496], "delta" [S,15], "trial" [S,16],
                                                    "workspace", "idx_i", "idx_j", and with priors "prior" [S,136], "pcost",
                                                    "pcost_new" [S], and with fixes "fix_rows" (two [S,136]) and
                                                    "fix_pcost" (two [S]), added to a dict that a call without fixes filled
        Returns (states, cost [C], lam [C], phase [C] int32: LM_RUNNING, LM_CONVERGED, LM_GAVE_UP)."""
        F, S, dev = lin.shape[0], states.shape[0], self.device
        C_ = self._chain_ranges(C, G, first, count, ffirst, True)
        b = buffers if buffers is not None else {}
        if not b:
            f64 = dict(dtype=torch.float64, device=dev)
            if torch.is_tensor(lam):
                self._lm_vector(lam, C_, torch.float64, True, "lam")
                b["lam"] = lam
            else:
                b["lam"] = torch.full((C_,), float(lam), **f64)
            b.update(cost=torch.zeros((C_,), **f64), phase=torch.zeros((C_,), dtype=torch.int32, device=dev),
                     accepted=torch.zeros((C_,), dtype=torch.int32, device=dev), status=torch.zeros((C_,), dtype=torch.int32, device=dev),
                     chi2=torch.zeros((F,), **f64), chi2_new=torch.zeros((F,), **f64), hess=torch.zeros((F, 496), **f64),
                     delta=torch.zeros((S, 15), **f64), trial=torch.zeros((S, 16), **f64),
                     workspace=torch.empty((self.chain_solve_workspace_doubles(S),), **f64))
            if prior0 is not None:
                b.update(prior=torch.zeros((S, 136), **f64), pcost=torch.zeros((S,), **f64), pcost_new=torch.zeros((S,), **f64))
            if idx_i is None or idx_j is None:
                ii, jj = self.chain_indices(C_, G, first, count)
                b["idx_i"], b["idx_j"] = ii.to(dev), jj.to(dev)
            else:
                b["idx_i"], b["idx_j"] = idx_i, idx_j
        if fixes and "fix_rows" not in b:                                     # also a buffers dict that a call without fixes filled
            b.update(fix_rows=[torch.zeros((S, 136), dtype=torch.float64, device=dev) for _ in range(2)],
                     fix_pcost=[torch.zeros((S,), dtype=torch.float64, device=dev) for _ in range(2)])
        chain = dict(C=C_, G=G, first=first, count=count, ffirst=ffirst)
        sweep = dict(idx_i=b["idx_i"], idx_j=b["idx_j"], grav=grav)
        priors = prior0 is not None
        if init:
            self.factor_cost(model, meas, lin, q_k_lin, states, R_tri, want_total=False, out={"chi2": b["chi2"]}, **sweep)
            self._lm_betweens(states, betweens or (), b["idx_i"], b["idx_j"], None, b["chi2"])
            if priors:
                self.prior_relinearize(states, anchor, prior0, idx=prior_idx, pcost=b["pcost"], want_prior=False)
            self.chain_cost(b["chi2"], self._lm_fixes(states, fixes or (), b.get("fix_pcost"), b.get("pcost"), False), out=b["cost"], **chain)
            if cost_history is not None:
                cost_history[0].copy_(b["cost"])
        for it in range(iterations):
            if priors:
                self.prior_relinearize(states, anchor, prior0, idx=prior_idx, out=b["prior"], want_cost=False)
            rows = self._lm_fixes(states, fixes or (), b.get("fix_rows"), b.get("prior"), True)
            self.factor_hessian(model, meas, lin, q_k_lin, states, R_tri, out=b["hess"], **sweep)
            self._lm_betweens(states, betweens or (), b["idx_i"], b["idx_j"], b["hess"], None)
            self.chain_solve(b["hess"], prior=rows, lam=b["lam"], damping=damping, out=b["delta"], status=b["status"],
                             workspace=b["workspace"], **chain)
            self.retract(states, b["delta"], out=b["trial"])
            self.factor_cost(model, meas, lin, q_k_lin, b["trial"], R_tri, want_total=False, out={"chi2": b["chi2_new"]}, **sweep)
            self._lm_betweens(b["trial"], betweens or (), b["idx_i"], b["idx_j"], None, b["chi2_new"])
            if priors:
                self.prior_relinearize(b["trial"], anchor, prior0, idx=prior_idx, pcost=b["pcost_new"], want_prior=False)
            pcost_new = self._lm_fixes(b["trial"], fixes or (), b.get("fix_pcost"), b.get("pcost_new"), False)
            self.chain_accept(b["chi2_new"], pcost_new, b["trial"], b["cost"], states, b["lam"], b["phase"], chi2=b["chi2"],
                              accepted=b["accepted"], params=params, **chain)
            if cost_history is not None:
                cost_history[it + 1].copy_(b["cost"])
        return states, b["cost"], b["lam"], b["phase"]


def unpack_factor(packed, meas):
    """Dense (err [F,15], H1 [F,225], H2 [F,225], column-major) from the packed evaluation and the measurement it was
    computed from -- the block table of include/cpi_amd.h (ImuFactorCPIv1.cpp:109-143,169-185)."""
    F = packed.shape[0]
    dev, f64 = packed.device, packed.dtype
    blk = lambda o: packed[:, o:o + 9].reshape(F, 3, 3).transpose(1, 2)      # column-major -> [row][col]
    cm = lambda t: t.reshape(F, 3, 3).transpose(1, 2)
    H1 = torch.zeros((F, 15, 15), dtype=f64, device=dev)
    H2 = torch.zeros((F, 15, 15), dtype=f64, device=dev)
    eye = torch.eye(3, dtype=f64, device=dev).expand(F, 3, 3)
    Rk = blk(51)
    H1[:, 0:3, 0:3], H1[:, 6:9, 0:3], H1[:, 12:15, 0:3], H1[:, 0:3, 3:6] = blk(15), blk(24), blk(33), blk(42)
    H1[:, 3:6, 3:6] = -eye
    H1[:, 9:12, 9:12] = -eye
    H1[:, 6:9, 3:6], H1[:, 6:9, 6:9], H1[:, 6:9, 9:12] = -cm(meas["J_b"]), -Rk, -cm(meas["H_b"])
    H1[:, 12:15, 3:6], H1[:, 12:15, 6:9] = -cm(meas["J_a"]), -meas["DT"][:, None, None] * Rk
    H1[:, 12:15, 9:12], H1[:, 12:15, 12:15] = -cm(meas["H_a"]), -Rk
    H2[:, 0:3, 0:3] = blk(60)
    H2[:, 3:6, 3:6] = eye
    H2[:, 6:9, 6:9] = Rk
    H2[:, 9:12, 9:12] = eye
    H2[:, 12:15, 12:15] = Rk
    return (packed[:, 0:15].contiguous(), H1.transpose(1, 2).reshape(F, 225).contiguous(),
            H2.transpose(1, 2).reshape(F, 225).contiguous())


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine()
    return _default_engine


def retract(states, delta, out=None):
    """Engine.retract on the default engine."""
    return default_engine().retract(states, delta, out)


def local_coordinates(x, other, out=None):
    """Engine.local_coordinates on the default engine."""
    return default_engine().local_coordinates(x, other, out)


def factor_cost(*args, **kw):
    """Engine.factor_cost on the default engine."""
    return default_engine().factor_cost(*args, **kw)


def chain_solve(*args, **kw):
    """Engine.chain_solve on the default engine."""
    return default_engine().chain_solve(*args, **kw)


def chain_marginals(*args, **kw):
    """Engine.chain_marginals on the default engine."""
    return default_engine().chain_marginals(*args, **kw)


def chain_marginalize(*args, **kw):
    """Engine.chain_marginalize on the default engine."""
    return default_engine().chain_marginalize(*args, **kw)


def chain_condense(*args, **kw):
    """Engine.chain_condense on the default engine."""
    return default_engine().chain_condense(*args, **kw)


def chain_expand(*args, **kw):
    """Engine.chain_expand on the default engine."""
    return default_engine().chain_expand(*args, **kw)


def chain_solve_segmented(*args, **kw):
    """Engine.chain_solve_segmented on the default engine."""
    return default_engine().chain_solve_segmented(*args, **kw)


def prior_relinearize(*args, **kw):
    """Engine.prior_relinearize on the default engine."""
    return default_engine().prior_relinearize(*args, **kw)


def chain_cost(*args, **kw):
    """Engine.chain_cost on the default engine."""
    return default_engine().chain_cost(*args, **kw)


def chain_accept(*args, **kw):
    """Engine.chain_accept on the default engine."""
    return default_engine().chain_accept(*args, **kw)


def chain_lm(*args, **kw):
    """Engine.chain_lm on the default engine."""
    return default_engine().chain_lm(*args, **kw)


def state_fix(*args, **kw):
    """Engine.state_fix on the default engine."""
    return default_engine().state_fix(*args, **kw)


def state_fix_host(*args, **kw):
    """Engine.state_fix_host on the default engine."""
    return default_engine().state_fix_host(*args, **kw)


def fix_offsets(idx, S):
    """Engine.fix_offsets."""
    return Engine.fix_offsets(idx, S)


def state_between(*args, **kw):
    """Engine.state_between on the default engine."""
    return default_engine().state_between(*args, **kw)


def state_between_host(*args, **kw):
    """Engine.state_between_host on the default engine."""
    return default_engine().state_between_host(*args, **kw)


# ---------------------------------------------------------------------- reference-shaped classes
class _CpiBase:
    """Mirror of CpiBase (CpiBase.h:40-145).  feed_IMU() records the interval; reading any result
    field runs the whole window through cpi_preintegrate_batch on the GPU (one window = one batch).
    Unlike the reference's feed_IMU (which integrates a negative dt; only its caller skips it, GraphSolver_IMU.cpp:52),
    an interval with t_1 - t_0 <= 0 is skipped."""
    _model = 0

    def __init__(self, sigma_w, sigma_wb, sigma_a, sigma_ab, imu_avg_=False, engine=None):
        self._sig = (sigma_w, sigma_wb, sigma_a, sigma_ab)
        self.imu_avg = bool(imu_avg_)
        self.state_transition_jacobians = True
        self.b_w_lin = np.zeros(3); self.b_a_lin = np.zeros(3)
        self.q_k_lin = np.zeros(4); self.grav = np.zeros(3)
        self._iv = []      # (t0, t1, w0, a0, w1, a1)
        self._res = None
        self._engine = engine
        self._incremental = False
        self._carry = None   # incremental: the carry record (device tensor [1, carry_doubles]) of the intervals run so far
        self._tail = None    # incremental: the last knot of the intervals run so far

    def set_incremental(self, on=True):
        """Incremental mode (Engine.preintegrate_resume): a read runs only the intervals fed since the previous read,
        continuing from the carried state, and keeps only the last knot.  Before the first feed_IMU only; the linearisation
        point cannot change once intervals were run.  Default off."""
        if on and self._model == 3:
            raise ValueError("set_incremental: the Forster comparator cannot be resumed")
        if self._iv or self._tail is not None:
            raise RuntimeError("set_incremental: call it before the first feed_IMU")
        self._incremental = bool(on)

    def setLinearizationPoints(self, b_w_lin_, b_a_lin_, q_k_lin_=None, grav_=None):
        if self._incremental and self._tail is not None:   # (a read before any feed_IMU integrates nothing)
            raise RuntimeError("setLinearizationPoints: an incremental preintegrator has already run intervals at the old point")
        self.b_w_lin = np.asarray(b_w_lin_, dtype=np.float64).reshape(3)
        self.b_a_lin = np.asarray(b_a_lin_, dtype=np.float64).reshape(3)
        self.q_k_lin = np.zeros(4) if q_k_lin_ is None else np.asarray(q_k_lin_, dtype=np.float64).reshape(4)
        self.grav = np.zeros(3) if grav_ is None else np.asarray(grav_, dtype=np.float64).reshape(3)
        self._res = None

    def feed_IMU(self, t_0, t_1, w_m_0, a_m_0, w_m_1=None, a_m_1=None):
        z = np.zeros(3)
        self._iv.append((float(t_0), float(t_1), np.asarray(w_m_0, float).reshape(3), np.asarray(a_m_0, float).reshape(3),
                         z if w_m_1 is None else np.asarray(w_m_1, float).reshape(3),
                         z if a_m_1 is None else np.asarray(a_m_1, float).reshape(3)))
        self._res = None

    def _knots(self, closing=None):
        """Intervals -> knot records (closing: a list that receives, per fed interval, the index of its closing knot).  Consecutive intervals that chain (t1 == next t0 and the next
        reading equals this interval's w1/a1) share a knot.  The reference's feed_IMU only ever uses
        t1 - t0, so intervals need not chain: a knot whose time is NaN acts as a separator (both
        intervals touching it have a NaN dt and are skipped by the kernels)."""
        rows = [] if self._tail is None else [self._tail.copy()]
        for (t0, t1, w0, a0, w1, a1) in self._iv:
            if rows and not self.imu_avg and rows[-1][0] == t0:
                # imu_avg == False: closing readings take no part in the arithmetic (CpiV1.h:77-86); when the TIMES chain the
                # previous closing knot simply takes this interval's opening reading (one knot per interval, as in cpi_host.hpp)
                rows[-1] = np.concatenate([[t0], w0, a0])
            chained = bool(rows) and rows[-1][0] == t0 and np.array_equal(rows[-1][1:4], w0) and np.array_equal(rows[-1][4:7], a0)
            if not chained:
                if rows:
                    rows.append(np.concatenate([[np.nan], np.zeros(6)]))
                rows.append(np.concatenate([[t0], w0, a0]))
            rows.append(np.concatenate([[t1], w1, a1]))
            if closing is not None:
                closing.append(len(rows) - 1)
        return np.stack(rows) if rows else np.zeros((1, 7))

    def _run(self):
        if self._res is not None:
            return self._res
        eng = self._engine or default_engine()
        kn = self._knots()
        dev = eng.device
        knots = torch.from_numpy(kn[None]).to(dev)
        lin = torch.from_numpy(np.concatenate([self.b_w_lin, self.b_a_lin])[None]).to(dev)
        q = torch.from_numpy(self.q_k_lin[None]).to(dev)
        prm = eng.make_params(self._model, self.imu_avg, self.state_transition_jacobians, self._sig, tuple(self.grav))
        if self._incremental:
            # every output requested, so that the carry holds every part a later read may need
            out, self._carry = eng.preintegrate_resume(knots, lin, q, prm, carry_in=self._carry)
            eng.synchronize()
            if self._iv:
                self._tail, self._iv = kn[-1], []
            self._res = {k: v.cpu().numpy()[0] for k, v in out.items()}
            return self._res
        out = eng.preintegrate(knots, lin, q, prm)
        eng.synchronize()
        self._res = {k: v.cpu().numpy()[0] for k, v in out.items()}
        return self._res

    def read_rows(self):
        """Incremental preintegrators only: run the intervals fed since the previous read through
        Engine.preintegrate_running_resume and return one result dict per interval fed since then -- the members as they
        stand after that feed_IMU (a skipped interval repeats the entry before it; the separator knots _knots() inserts
        produce no entry).  The carry and the tail knot advance as in a member read, and the ordinary members (alpha_tau,
        P_meas, ...) then equal the last entry.  Model 2: no Jacobians in the entries (read J_q ... from the members)."""
        if not self._incremental:
            raise RuntimeError("read_rows: set_incremental(True) first (the rows continue from the carried state)")
        if self._model == 3:
            raise ValueError("read_rows: the Forster comparator has no running form")
        if self._model == 2 and not self.state_transition_jacobians:
            raise ValueError("read_rows: model 2's analytic Jacobians (state_transition_jacobians = False) have no running form")
        if not self._iv:
            return []
        eng = self._engine or default_engine()
        closing = []
        kn = self._knots(closing)
        dev = eng.device
        knots = torch.from_numpy(kn[None]).to(dev)
        lin = torch.from_numpy(np.concatenate([self.b_w_lin, self.b_a_lin])[None]).to(dev)
        q = torch.from_numpy(self.q_k_lin[None]).to(dev)
        prm = eng.make_params(self._model, self.imu_avg, self.state_transition_jacobians, self._sig, tuple(self.grav))
        # every running field, so that the carry holds every part a later read (of rows or of members) needs
        rows, self._carry = eng.preintegrate_running_resume(knots, lin, q, prm, carry_in=self._carry)
        eng.synchronize()
        self._tail, self._iv = kn[-1], []
        host = {k: v.cpu().numpy()[0] for k, v in rows.items()}
        res = [{k: v[c - 1] for k, v in host.items()} for c in closing]
        # model 2: the members' Jacobians are read out of the carried state-transition columns by a zero-interval resume
        self._res = res[-1] if self._model == 1 else None
        return res

    def at(self, times):
        """Incremental preintegrators only: the measurement AT each of `times` (a camera frame stamped inside the chunk that has
        just been fed).  Runs the intervals fed since the previous read (Engine.preintegrate_running_resume_stj) -- the carry and
        the tail knot advance exactly as in read_rows() -- and queries them with the state at the previous read as the base row
        (Engine.query_open).  Returns one result dict per time: the means, P, and model 1's five Jacobians or model 2's seven.  A
        time on a fed stamp gives the members as they stood there, a time inside an interval that state advanced with the
        interval's opening reading held, a time before the first pending interval the state at the previous read, a time at or
        past the last stamp the current state.  The pending intervals must chain (no separator knots)."""
        if not self._incremental:
            raise RuntimeError("at: set_incremental(True) first (the queries continue from the carried state)")
        if self._model == 3:
            raise ValueError("at: the Forster comparator has no running form")
        if self._model == 2 and not self.state_transition_jacobians:
            raise ValueError("at: model 2's analytic Jacobians (state_transition_jacobians = False) have no running form")
        times = np.asarray(times, dtype=np.float64).reshape(-1)
        if times.size == 0:
            return []
        kn = self._knots()
        if np.isnan(kn[:, 0]).any():
            raise ValueError("at: the intervals fed since the previous read do not chain (a query needs finite, non-decreasing stamps)")
        eng = self._engine or default_engine()
        dev = eng.device
        knots = torch.from_numpy(kn[None]).to(dev)
        lin = torch.from_numpy(np.concatenate([self.b_w_lin, self.b_a_lin])[None]).to(dev)
        q = torch.from_numpy(self.q_k_lin[None]).to(dev)
        prm = eng.make_params(self._model, self.imu_avg, self.state_transition_jacobians, self._sig, tuple(self.grav))
        # the state at the previous read as one ordinary row: a segment of one interval that is not counted
        base, _ = eng.preintegrate_running_resume_stj(knots[:, :1].repeat(1, 2, 1).contiguous(), lin, q, prm,
                                                      count=torch.zeros(1, dtype=torch.int32, device=dev), carry_in=self._carry)
        rows = {}
        if self._iv:
            # every running field, so that the carry holds every part a later read (of rows or of members) needs
            rows, self._carry = eng.preintegrate_running_resume_stj(knots, lin, q, prm, carry_in=self._carry)
        out = eng.query_open(knots, lin, rows, torch.zeros(times.size, dtype=torch.int32, device=dev), torch.from_numpy(times).to(dev),
                             base, q, prm, want=("mean", "jac", "cov"))
        eng.synchronize()
        if self._iv:
            self._tail, self._iv = kn[-1], []
        self._res = None   # the members are read out of the carried state by the next member read
        host = {k: v.cpu().numpy() for k, v in out.items()}
        return [{k: v[i] for k, v in host.items()} for i in range(times.size)]

    def _m3(self, name):
        return self._run()[name].reshape(3, 3).T  # column-major -> [row][col]

    DT = property(lambda s: float(s._run()["DT"]))
    alpha_tau = property(lambda s: s._run()["alpha"])
    beta_tau = property(lambda s: s._run()["beta"])
    q_k2tau = property(lambda s: s._run()["q"])
    J_q = property(lambda s: s._m3("J_q"))
    J_a = property(lambda s: s._m3("J_a"))
    J_b = property(lambda s: s._m3("J_b"))
    H_a = property(lambda s: s._m3("H_a"))
    H_b = property(lambda s: s._m3("H_b"))
    P_meas = property(lambda s: s._run()["P"].reshape(15, 15).T)


class CpiV1(_CpiBase):
    _model = 1


class CpiV2(_CpiBase):
    _model = 2
    O_a = property(lambda s: s._m3("O_a"))
    O_b = property(lambda s: s._m3("O_b"))


class ForsterDiscrete(_CpiBase):
    """The "Forster discrete" comparator as GraphSolver::createimufactor_discrete (GraphSolver_IMU.cpp:141-232) uses
    it: GTSAM's PreintegratedCombinedMeasurements driven by integrateMeasurement(acc, omega, dt), read back through the
    call site's conversions (:204-225) into the CpiV1-shaped result fields.  GTSAM is absent from the reference tree:
    parity of this model is unpinned (oracle/forster_oracle.c)."""
    _model = 3

    def __init__(self, sigma_g, sigma_wg, sigma_a, sigma_wa, engine=None):
        super().__init__(sigma_g, sigma_wg, sigma_a, sigma_wa, False, engine)
        self._t = 0.0

    def integrateMeasurement(self, measuredAcc, measuredOmega, dt):
        if not dt > 0:
            return
        w, a = np.asarray(measuredOmega, float).reshape(3), np.asarray(measuredAcc, float).reshape(3)
        if self._iv:   # the previous interval's closing knot opens this one: it carries this reading
            t0, t1, w0, a0, _, _ = self._iv[-1]
            self._iv[-1] = (t0, t1, w0, a0, w, a)
        self._iv.append((self._t, self._t + float(dt), w, a, w, a))
        self._t += float(dt)
        self._res = None

    deltaTij = property(lambda s: s.DT)


class _ImuFactorBase:
    _model = 0

    def _setup(self, covariance, deltatime, grav, alpha, beta, q_KtoK1, ba_lin, bg_lin, J_q, J_beta, J_alpha, H_beta,
               H_alpha, q_K_lin=None, O_beta=None, O_alpha=None, engine=None):
        self.covariance = np.asarray(covariance, float)
        self._grav = tuple(np.asarray(grav, float).reshape(3))
        cm = lambda M: np.asarray(M, float).reshape(3, 3).T.reshape(9)  # -> column-major flat
        f = lambda v, n: np.asarray(v, float).reshape(n)
        self._meas = dict(DT=np.array([float(deltatime)]), alpha=f(alpha, 3)[None], beta=f(beta, 3)[None],
                          q=f(q_KtoK1, 4)[None], J_q=cm(J_q)[None], J_b=cm(J_beta)[None], J_a=cm(J_alpha)[None],
                          H_b=cm(H_beta)[None], H_a=cm(H_alpha)[None])
        if self._model == 2:
            self._meas["O_b"] = cm(O_beta)[None]; self._meas["O_a"] = cm(O_alpha)[None]
        self._lin = np.concatenate([f(bg_lin, 3), f(ba_lin, 3)])[None]
        self._qk = None if q_K_lin is None else f(q_K_lin, 4)[None]
        self._engine = engine

    def evaluateError(self, state_i, state_j, want_H=True):
        """state = 16-vector [q(4) bg(3) v(3) ba(3) p(3)].  Returns error[15] (and H1, H2 as 15x15)."""
        eng = self._engine or default_engine()
        dev = eng.device
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        meas = {k: T(v) for k, v in self._meas.items()}
        states = T(np.stack([np.asarray(state_i, float).reshape(16), np.asarray(state_j, float).reshape(16)]))
        out = eng.factor_eval(self._model, meas, T(self._lin), None if self._qk is None else T(self._qk), states,
                              want_H=want_H, grav=self._grav)
        eng.synchronize()
        e = out["err"].cpu().numpy()[0]
        if not want_H:
            return e
        return e, out["H1"].cpu().numpy()[0].reshape(15, 15).T, out["H2"].cpu().numpy()[0].reshape(15, 15).T


class ImuFactorCPIv1(_ImuFactorBase):
    """Argument order of ImuFactorCPIv1.h:78-81 (keys omitted)."""
    _model = 1

    def __init__(self, covariance, deltatime, grav, alpha, beta, q_KtoK1, ba_lin, bg_lin, J_q, J_beta, J_alpha, H_beta,
                 H_alpha, engine=None):
        self._setup(covariance, deltatime, grav, alpha, beta, q_KtoK1, ba_lin, bg_lin, J_q, J_beta, J_alpha, H_beta,
                    H_alpha, engine=engine)


class ImuFactorCPIv2(_ImuFactorBase):
    """Argument order of ImuFactorCPIv2.h:82-85 (keys omitted)."""
    _model = 2

    def __init__(self, covariance, deltatime, grav, alpha, beta, q_KtoK1, q_K_lin, ba_lin, bg_lin, J_q, J_beta, J_alpha,
                 H_beta, H_alpha, O_beta, O_alpha, engine=None):
        self._setup(covariance, deltatime, grav, alpha, beta, q_KtoK1, ba_lin, bg_lin, J_q, J_beta, J_alpha, H_beta,
                    H_alpha, q_K_lin=q_K_lin, O_beta=O_beta, O_alpha=O_alpha, engine=engine)
