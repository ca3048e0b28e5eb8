#!/usr/bin/env python
"""bench.py -- preintegration windows/sec on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload NAME] [--scaling weak|strong] [--dump-outputs DIR]
                    [--full [--no-extra] [--no-cpu]]

A "step" is one pass of the hot path (one cpi_preintegrate_batch / cpi_factor_eval_batch call) over one batch of
synthetic windows already resident in HBM.  The default workload is BASELINE.json configs[1]: 10 000 windows x 50
samples, CPI model 1, mean-only.  Successive steps walk a pool of distinct batches larger than the 256 MiB Infinity
Cache, so the inputs really stream from HBM.  The K timed steps are replayed as ONE HIP graph (K kernel nodes, captured
from the same calls; beyond GRAPH_MAX_STEPS as replays of a graph of that many steps; `config.launch_mode` says which mode
ran -- eager launches are the fall-back).  Prints ONE JSON line
(rank 0).

N > 1: one rank per GPU over RCCL.  Launched either by the driver (`python -m torch.distributed.run ... bench.py --gpus N`,
WORLD_SIZE set) or by itself: with WORLD_SIZE unset `python bench.py --gpus N` re-executes under torch.distributed.run.
Windows shard with no data-path collective ("weak": every rank runs the per-GPU workload; "strong": the workload's
windows are split N ways); the one exchange step is the gather of the output slabs TO RANK 0 (cpi_amd.dist.gather_to_root:
each peer sends ONE packed slab straight to the root over its own xGMI link).  Two schedules (`config.gather_schedule`):
  final      the K steps, then the gather of the last step's slabs (small batches: the headline).  The clock of a rank stops
             when ITS part is done -- the root's when every slab has arrived -- and the line reports the MAX over ranks; the
             closing barrier is outside the timed region.
  pipelined  every step's slab is gathered, on a side stream, while the next step computes (double-buffered outputs and
             receive buffers): the schedule for steps that last milliseconds (`--scaling strong`, cfg5_*).
  chunked    the exchange INSIDE a step (round 6; `--gather-chunks k`): the batch in k sub-blocks, each computed by its own launch into a
             slab of its own, sub-block c on the wire while c + 1 computes -- what ONE batch with "a final gather" (configs[4]) needs;
             the torch.distributed twin of cpi_group_gather_chunk.  `--workload cfg5_full_sym` sends the covariance as its packed upper
             triangle (1 408 instead of 2 248 bytes per window).
`config.predicted` (N > 1) states what the exchange SHOULD cost on xGMI -- slab bytes per peer over one link at 76.8 GB/s one way -- and the
expected wall time of the timed region under the schedule in use, from the kernel time measured in the same run.
`kernel_ms` (HIP events around the K steps), `gather_ms` (the exposed tail after the last kernel) and the rate without any
exchange (`value_without_gather`) are reported beside `value`.  `--workload cfg5_mean | cfg5_full` is BASELINE configs[4]:
1 M windows x 100 samples per GPU, generated on the device.

Output contract (rank 0): the LAST stdout line is ONE JSON object of < 6 KB.  A plain run sets up, warms up, times the K
steps, writes the outputs of the last one (`--dump-outputs DIR`: DIR/<name>.npy, float64, a fixed sample of rows beyond 64 MB)
and prints the headline: metric, value, unit, higher_is_better, dtype, ms_per_step (wall time of the K steps / K), config and
the `roofline` of the timed kernel.  `--full` measures everything else in the same run: the CPU baseline (`cpu_baseline`), the
overlapped rate of the headline workload (`overlapped`, `value_overlapped`) and the extra rows, with `value_full_integrator`
(= configs2.value: `value` is the LIGHTEST configuration, mean-only), a compact `configs2` object (BASELINE configs[2]), the
end-to-end route table of a 1 M x 50 batch held as one IMU stream (`routes_1M_x_50`) and one [launch ms, roofline fraction]
pair per extra row in the line.  The full extra rows (45 workloads incl. the SURVEY 8(f) rows, the packed-triangle rows of
ABI 3 and the reference's own window lengths -- 10 / 20 samples, keyed `...@1Mx10` --, each with its own `roofline`, counters
and `cpu_baseline`) are written to bench_extra.json beside this file; tests/test_gpu_bench.py runs the driver's command
verbatim, and with --full, and checks both.  N > 1 adds `config.rccl` (what the collective library saw), `value_kernel_only`
and `gather_verified` (rank 0 recomputes every rank's last-step batch and compares the gathered blocks bitwise).
"""
import argparse
import json
import math
import os
import socket
import sys
import time

# multi-process GPU work on this host driver needs dmabuf IPC (RCCL fails with `hipIpcGetMemHandle: invalid argument` otherwise);
# the boxes export it already -- kept here so that a launcher with a scrubbed environment still gets it, before HIP initialises
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8 TB/s HBM3E peak
FP64_PEAK_TFLOPS = 78.6         # vector FP64 (datasheet); the covariance kernels are VALU / LDS-bound
MALL_BYTES = 256 << 20
PMC_FILE = os.path.join(ROOT, "profiles", "r06_pmc.json")
# xGMI: AMD quotes 153.6 GB/s per Infinity Fabric link BIDIRECTIONAL (the "7 links x ~153 GB/s" of the MI355X platform); a gather
# moves data ONE way, each peer over its own link into the root: 76.8 GB/s per peer is the wire's ceiling, before protocol overhead
XGMI_LINK_GBS_ONE_WAY = 76.8
# steps per captured HIP graph: a longer run replays it (capturing 400 000 steps as one graph crashed the process on the
# MI355X, 100 000 did not); it is the default K, so runs up to it time ONE graph as before
GRAPH_MAX_STEPS = 5000
DUMP_LIMIT_BYTES = 64 * 1000 * 1000   # --dump-outputs: the whole dump, .npy headers included
DUMP_SAMPLE_SEED = 20190101           # --dump-outputs: the rows kept when the outputs are larger

# name -> kind, model, default units per step, samples, algorithmic HBM bytes per unit at 50 samples (SURVEY.md 8(d):
# read + write, f64, compulsory traffic only), dominant kernel.  kinds: "pre" preintegration (dense layout), "tiled" the
# mean-only recursion on the tiled layout (batches cut from ONE stream by cpi_assemble_tiles), "factor" the dense
# evaluateError sweep and its variants, "sqrt_info", "predict".
IN1, IN2 = 776, 952             # bytes a factor reads: measurement + lin (+ q_k_lin, O_a, O_b) + two states
WORKLOADS = {
    "v1_mean": dict(kind="pre", model=1, want=("mean",), W=10000, N=50, bytes=2856 + 88, kernel="cpi_mean_kernel<1,false,false,L>"),
    "v2_mean": dict(kind="pre", model=2, want=("mean",), W=10000, N=50, bytes=2888 + 88, kernel="cpi_mean_kernel<2,false,false,L>"),
    "v1_full": dict(kind="pre", model=1, want=("mean", "jac", "cov"), W=100000, N=50, bytes=2856 + 2320, kernel="cpi_cov_kernel<1,false>",
                    useful_lanes=(15, 16)),
    "v2_full": dict(kind="pre", model=2, want=("mean", "jac", "cov"), W=100000, N=50, bytes=2888 + 2392, kernel="cpi_cov_kernel<2,false>",
                    useful_lanes=(27, 32)),
    # Forster / GTSAM comparator (CPI_MODEL_FORSTER): same I/O as model 1 full
    "forster_full": dict(kind="pre", model=3, want=("mean", "jac", "cov"), W=100000, N=50, bytes=2856 + 2320, kernel="cpi_forster_kernel",
                         useful_lanes=(15, 16)),
    "factor_v1": dict(kind="factor", model=1, W=1000000, N=50, bytes=IN1 + 3720, kernel="cpi_factor_kernel<1,false,8>"),
    "factor_v2": dict(kind="factor", model=2, W=1000000, N=50, bytes=IN2 + 3720, kernel="cpi_factor_kernel<2,false,8>"),
    # packed evaluateError (state-dependent blocks only, include/cpi_amd.h): NOT the dense GTSAM-shaped output
    "factor_v1_packed": dict(kind="factor", variant="packed", model=1, W=1000000, N=50, bytes=IN1 + 576, kernel="cpi_factor_packed_kernel<1,L>"),
    "factor_v2_packed": dict(kind="factor", variant="packed", model=2, W=1000000, N=50, bytes=IN2 + 576, kernel="cpi_factor_packed_kernel<2,L>"),
    # what GTSAM does right after evaluateError -- whitening by the square-root information, Hessian blocks
    "sqrt_info": dict(kind="sqrt_info", model=1, W=1000000, N=50, bytes=1800 + 1800, kernel="cpi_sqrt_info_kernel"),
    "factor_v1_whitened": dict(kind="factor", variant="whitened", model=1, W=1000000, N=50, bytes=IN1 + 1800 + 3720, kernel="cpi_factor_kernel<1,true,16>"),
    "factor_v2_whitened": dict(kind="factor", variant="whitened", model=2, W=1000000, N=50, bytes=IN2 + 1800 + 3720, kernel="cpi_factor_kernel<2,true,16>"),
    "factor_v1_hessian": dict(kind="factor", variant="hessian", model=1, W=1000000, N=50, bytes=IN1 + 1800 + 3968, kernel="cpi_factor_hessian_kernel<1>"),
    "factor_v2_hessian": dict(kind="factor", variant="hessian", model=2, W=1000000, N=50, bytes=IN2 + 1800 + 3968, kernel="cpi_factor_hessian_kernel<2>"),
    # ABI 3 (round 6): the same three rows on PACKED TRIANGLES -- P as its upper triangle (cpi_outputs.P_sym, 960 B), R as its
    # non-zero triangle (960 B): the dense forms move 840 B of mirrored P and 840 B of zeros per factor (include/cpi_amd.h)
    "sqrt_info_packed": dict(kind="sqrt_info", tri=True, model=1, W=1000000, N=50, bytes=960 + 960, kernel="cpi_sqrt_info_kernel<true>"),
    "factor_v1_whitened_tri": dict(kind="factor", variant="whitened", tri=True, model=1, W=1000000, N=50, bytes=IN1 + 960 + 3720, kernel="cpi_factor_kernel<1,true,16,true>"),
    "factor_v2_whitened_tri": dict(kind="factor", variant="whitened", tri=True, model=2, W=1000000, N=50, bytes=IN2 + 960 + 3720, kernel="cpi_factor_kernel<2,true,16,true>"),
    "factor_v1_hessian_tri": dict(kind="factor", variant="hessian", tri=True, model=1, W=1000000, N=50, bytes=IN1 + 960 + 3968, kernel="cpi_factor_hessian_kernel<1,true>"),
    "factor_v2_hessian_tri": dict(kind="factor", variant="hessian", tri=True, model=2, W=1000000, N=50, bytes=IN2 + 960 + 3968, kernel="cpi_factor_hessian_kernel<2,true>"),
    # getpredictedstate_v1 / _v2 -- reads alpha, beta, q, DT (88 B) + a state (128 B), writes a state
    "predict_v1": dict(kind="predict", model=1, W=1000000, N=50, bytes=88 + 128 + 128, kernel="cpi_predict_kernel<1>"),
    "predict_v2": dict(kind="predict", model=2, W=1000000, N=50, bytes=88 + 128 + 128, kernel="cpi_predict_kernel<2>"),
    # the same mean-only recursion on the TILED input layout (knots of 64 windows interleaved per step; include/cpi_amd.h),
    # the batches cut from one IMU stream by the device assembler (cpi_assemble_tiles) -- no dense copy, no cpi_tile_knots
    "v1_mean_tiled": dict(kind="tiled", model=1, want=("mean",), W=1000000, N=50, bytes=2856 + 88, kernel="cpi_mean_tiled_kernel<1,false,true,SPLIT>"),
    "v2_mean_tiled": dict(kind="tiled", model=2, want=("mean",), W=1000000, N=50, bytes=2888 + 88, kernel="cpi_mean_tiled_kernel<2,false,true,SPLIT>"),
    # the zero-copy stream entry (cpi_preintegrate_stream): ONE resident IMU stream of W x N + 1 readings + W update times, the
    # kernels cut the windows in place.  A window reads N new readings (the boundary reading is shared), its update time and
    # lin.  Mean-only (round 4): the mean kernel cuts its own windows -- no cut kernel, no workspace record; it writes the
    # window's true interval count (4 B).  The *_full rows keep the workspace route: a 28-byte record per window written by the
    # cut kernel and read by the preintegration kernel(s)
    "v1_mean_stream": dict(kind="stream", model=1, want=("mean",), W=1000000, N=50, bytes=2800 + 8 + 48 + 4 + 88, kernel="cpi_mean_kernel<1,false,false,1,CUT=2,BIG> (fused cut)"),
    "v1_full_stream": dict(kind="stream", model=1, want=("mean", "jac", "cov"), W=100000, N=50, bytes=2800 + 8 + 48 + 56 + 2320, kernel="cpi_cov_kernel<1,false> (+ cut, Jacobian kernels)",
                           useful_lanes=(15, 16)),
    "v2_full_stream": dict(kind="stream", model=2, want=("mean", "jac", "cov"), W=100000, N=50, bytes=2800 + 8 + 80 + 56 + 2392, kernel="cpi_cov_kernel<2,false> (+ cut kernel)",
                           useful_lanes=(27, 32)),
    # BASELINE configs[4]: one GPU's share of 8 M windows x 100 samples (EuRoC-rate synthetic IMU), generated on the device
    "cfg5_mean": dict(kind="pre", model=1, want=("mean",), W=1000000, N=100, bytes=2856 + 88, kernel="cpi_mean_kernel<1,false,false,1>"),
    "cfg5_full": dict(kind="pre", model=1, want=("mean", "jac", "cov"), W=1000000, N=100, bytes=2856 + 2320, kernel="cpi_cov_kernel<1,false>",
                      useful_lanes=(15, 16)),
    # the same with the covariance as its packed upper triangle (cpi_outputs.P_sym, ABI 3): 1 480 instead of 2 320 bytes out per
    # window -- on one GPU nothing (the row is FP64-bound), at N > 1 the slab a peer sends to the root shrinks by 36 %
    "cfg5_full_sym": dict(kind="pre", model=1, want=("mean", "jac", "cov_sym"), W=1000000, N=100, bytes=2856 + 1480, kernel="cpi_cov_kernel<1,false>",
                          useful_lanes=(15, 16)),
    "v1_full_sym": dict(kind="pre", model=1, want=("mean", "jac", "cov_sym"), W=100000, N=50, bytes=2856 + 1480, kernel="cpi_cov_kernel<1,false>",
                        useful_lanes=(15, 16)),
    "v2_full_sym": dict(kind="pre", model=2, want=("mean", "jac", "cov_sym"), W=100000, N=50, bytes=2888 + 1552, kernel="cpi_cov_kernel<2,false>",
                        useful_lanes=(27, 32)),
}
# sparse-minimal FP64 flop per 50-sample window (0.35-0.5 M and 0.65-0.8 M; midpoints) -- an ESTIMATE, used
# only when no counter-derived figure is available for the loaded library
FLOP_EST = {"v1_full": 0.425e6, "v2_full": 0.725e6}


def bytes_per_unit(workload, samples=50):
    """a window reads samples*56 + 8 + 48 (+32 for q_k_lin) bytes; WORKLOADS holds that figure at 50
    samples.  Factor-shaped workloads do not depend on the window length."""
    w = WORKLOADS[workload]
    return w["bytes"] + (samples - 50) * 56 if w["kind"] in ("pre", "tiled", "stream") else w["bytes"]


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--workload", default="v1_mean", choices=sorted(WORKLOADS))
    ap.add_argument("--windows", type=int, default=0, help="windows (factors) per step and GPU; 0 = the workload's size")
    ap.add_argument("--samples", type=int, default=0, help="samples per window; 0 = the workload's (50; cfg5: 100)")
    ap.add_argument("--lanes", type=int, default=0, help="mean kernel lanes per window (0 = auto)")
    ap.add_argument("--scaling", default="weak", choices=("weak", "strong"),
                    help="N > 1: weak = every rank runs the per-GPU workload; strong = the workload's windows are split N ways")
    ap.add_argument("--gather", default="root", choices=("root", "all", "none"), help="N > 1: the exchange step")
    ap.add_argument("--gather-schedule", default="auto", choices=("auto", "final", "pipelined", "chunked"),
                    help="N > 1: final = one gather after the K steps; pipelined = every step's slab, overlapped with the next step "
                         "(auto: pipelined when a step lasts about a millisecond or more); chunked = the exchange INSIDE a step: the "
                         "batch in --gather-chunks sub-blocks, sub-block c on the wire while c + 1 computes (the torch.distributed twin of "
                         "cpi_group_gather_chunk)")
    ap.add_argument("--gather-chunks", type=int, default=8, help="sub-blocks per step of the chunked schedule")
    ap.add_argument("--eager", action="store_true", help="issue the K timed steps as K launches instead of replaying one HIP graph")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the CPU baseline legs, the overlapped rate and the additional "
                         "BASELINE configs (bench_extra.json)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the additional BASELINE configs")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float64; a fixed sample of rows when they exceed "
                         "%d MB)" % (DUMP_LIMIT_BYTES // 1000000))
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------ workloads
class Workload:
    """A pool of resident batches + preallocated outputs + a step() closure."""

    def __init__(self, eng, name, W, N, seed, lanes=0, pool_bytes=MALL_BYTES * 5 // 4, min_out_sets=1):
        from cpi_amd import synth
        spec = WORKLOADS[name]
        self.name, self.W, self.N, self.spec = name, W, N, spec
        self.kind, self.model, self.variant = spec["kind"], spec["model"], spec.get("variant", "dense")
        self.is_factor = self.kind not in ("pre", "tiled", "stream")       # unit = factor
        self.eng, self.i, self.assembly = eng, 0, None
        dev = eng.device
        f64 = dict(dtype=torch.float64, device=dev)
        if self.is_factor:
            model = self.model
            need_cov = self.kind == "sqrt_info" or self.variant in ("whitened", "hessian")
            tri = bool(spec.get("tri"))                  # packed triangles: P_sym in, R_tri through the sweeps
            pkey = "P_sym" if tri else "P"
            kn, lin, q = synth.make_windows(W, N, seed=seed, device=dev)
            self.meas = eng.preintegrate(kn, lin, q, eng.make_params(model), want=("mean", "jac", "cov_sym" if tri else "cov") if need_cov else ("mean", "jac"))
            torch.cuda.synchronize()
            del kn
            xi, xj = synth.make_states(self.meas["alpha"], self.meas["beta"], self.meas["q"], self.meas["DT"], lin, model, device=dev)
            self.states = torch.cat([xi, xj[-1:]], dim=0).contiguous()   # chained states: idx_i=f, idx_j=f+1
            self.lin, self.q = lin, (q if model == 2 else None)
            self.R = eng.sqrt_information(self.meas[pkey]) if need_cov else None
            if self.kind == "sqrt_info":
                self.P = self.meas[pkey]
                self.out = self.R
            elif self.kind == "predict":
                self.out = torch.empty((W, 16), **f64)
            elif self.variant == "packed":
                self.out = torch.empty((W, 72), **f64)
            elif self.variant == "hessian":
                self.out = torch.empty((W, 496), **f64)
                self.meas = {k: v for k, v in self.meas.items() if k != pkey}
            else:
                self.out = {"err": torch.empty((W, 15), **f64), "H1": torch.empty((W, 225), **f64), "H2": torch.empty((W, 225), **f64)}
                if need_cov:
                    self.meas = {k: v for k, v in self.meas.items() if k != pkey}
            torch.cuda.synchronize()
            self.nbatch = 1   # gigabytes per sweep: far beyond the Infinity Cache by itself
            return
        self.want = spec["want"]
        self.prm = eng.make_params(self.model, lanes_per_window=lanes)
        batch_bytes = W * (N + 1) * 56
        self.nbatch = max(1, min(64, -(-pool_bytes // batch_bytes)))
        # one flat buffer per output set: a rank's outputs are one contiguous slab, so the multi-GPU gather is ONE message per peer
        out_bytes = W * sum(n for _, n in eng.alloc_outputs(1, self.want, self.model, packed=True)["_fields"]) * 8
        nsets = max(min_out_sets, 1 if out_bytes > (1 << 30) else min(self.nbatch, 4))
        self.outs = [eng.alloc_outputs(W, self.want, self.model, packed=True) for _ in range(nsets)]
        period = self.nbatch * nsets // math.gcd(self.nbatch, nsets)
        self.calls = []
        if self.kind == "tiled":
            # every batch is ONE IMU stream + W update times (one every N samples, on the IMU grid: N whole intervals per
            # window) cut by the DEVICE ASSEMBLER straight into tiles: the producer a caller shaped like
            # GraphSolver_IMU.cpp:50-69 uses.  Its cost is measured here, once per batch, and reported beside the row.
            self.batches, ev = [], []
            for b in range(self.nbatch):
                stream, upd, lin, q = synth.make_stream(W, N, seed=seed + 101 * b, device=dev)
                tiles = torch.empty(((W + 63) // 64, N + 1, 7, 64), **f64)
                count = torch.empty((W,), dtype=torch.int32, device=dev)
                eng.assemble_tiles(stream, upd, N, tiles=tiles, count=count)          # warm (first launch, page faults)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); eng.assemble_tiles(stream, upd, N, tiles=tiles, count=count); e1.record()
                torch.cuda.synchronize()
                ev.append(e0.elapsed_time(e1))
                assert int(count.max().item()) == N and int(count.min().item()) == N, "the bench stream must cut into N-interval windows"
                self.batches.append((tiles, count, lin, q))
                del stream, upd
            ms = sorted(ev)[len(ev) // 2]
            self.assembly = {"what": "cpi_assemble_tiles: ONE stream of W x N + 1 readings + W update times -> tiles + count (device, one launch per batch)",
                             "ms_per_batch": ms, "GBs": (W * N * 56 + W * 8 + W * (N + 1) * 56 + W * 4) / (ms * 1e-3) / 1e9,
                             "share_of_step": None}
            for i in range(period):
                tiles, count, lin, q = self.batches[i % self.nbatch]
                call, _ = eng.preintegrate_tiled(tiles, W, lin, q, self.prm, count=count, out=self.outs[i % nsets], bind=True)
                self.calls.append(call)
            return
        if self.kind == "stream":
            # phase 0.4: every window ends in a partial tail interval (N whole intervals + the tail = N + 1 per window,
            # the reference's general case); a step = cut kernel + preintegration kernel(s), nothing copied
            self.batches = [synth.make_stream(W, N, seed=seed + 101 * b, device=dev, phase=0.4) for b in range(self.nbatch)]
            self.ws = [eng.stream_workspace(W) for _ in range(self.nbatch)]
            for i in range(period):
                stream, upd, lin, q = self.batches[i % self.nbatch]
                o, w_ = self.outs[i % nsets], self.ws[i % self.nbatch]
                self.calls.append(lambda stream=stream, upd=upd, lin=lin, q=q, o=o, w_=w_: eng.preintegrate_stream(
                    stream, upd, lin, q, self.prm, want=self.want, N=N + 1, out=o, check_counts=False, workspace=w_))
            return
        self.batches = [synth.make_windows(W, N, seed=seed + 101 * b, device=dev) for b in range(self.nbatch)]
        # every (batch, output set) pair of the walk pre-bound: a step is one foreign call (Engine.bind_preintegrate)
        for i in range(period):
            kn, lin, q = self.batches[i % self.nbatch]
            call, _ = eng.bind_preintegrate(kn, lin, q if self.model != 3 else None, self.prm, want=self.want, out=self.outs[i % nsets])
            self.calls.append(call)

    def make_chunks(self, k):
        """The chunked schedule: every batch in k sub-blocks of cper = ceil(W / k) windows (cpi_shard_chunk_bounds' rule applied to
        this rank's block), each with a packed output slab of its own per output set -- sub-block c is computed by its own launch and
        its slab travels while sub-block c + 1 computes.  Dense-layout preintegration workloads only."""
        assert self.kind == "pre", "the chunked schedule shards the dense layout"
        self.k, self.cper = k, -(-self.W // k)
        self.chunk_outs, self.chunk_calls = [], []
        nsets = len(self.outs)
        for s_ in range(nsets):
            self.chunk_outs.append([self.eng.alloc_outputs(max(1, min(self.cper, self.W - c * self.cper)) if c * self.cper < self.W else 1,
                                                           self.want, self.model, packed=True) for c in range(k)])
        for i in range(len(self.calls)):
            kn, lin, q = self.batches[i % self.nbatch]
            row = []
            for c in range(k):
                lo, hi = min(self.W, c * self.cper), min(self.W, (c + 1) * self.cper)
                if hi <= lo:
                    row.append(None)
                    continue
                call, _ = self.eng.bind_preintegrate(kn[lo:hi], lin[lo:hi], q[lo:hi] if self.model != 3 else None, self.prm, want=self.want,
                                                     out=self.chunk_outs[i % nsets][c])
                row.append(call)
            self.chunk_calls.append(row)

    def chunk_step(self, c):
        """Launch sub-block c of the current step; returns its output set (advance self.i after the last sub-block)."""
        call = self.chunk_calls[self.i % len(self.chunk_calls)][c]
        if call is not None:
            call()
        return self.chunk_outs[self.i % len(self.outs)][c]

    def out_of(self, i):
        """The outputs step number i writes."""
        return self.out if self.is_factor else self.outs[i % len(self.outs)]

    def outputs_of(self, i):
        """What a caller of step number i receives: output name -> device tensor, one row per window / factor."""
        out = self.out_of(i)
        if isinstance(out, dict):
            return {k: v for k, v in out.items() if not k.startswith("_")}
        return {{"sqrt_info": "R", "predict": "x_j"}.get(self.kind, self.variant): out}    # the packed / Hessian sweeps: "packed", "hessian"

    def step(self):
        if self.is_factor:
            e = self.eng
            if self.kind == "sqrt_info":
                e.sqrt_information(self.P, out=self.R)
            elif self.kind == "predict":
                e.predict(self.model, self.meas, self.states, out=self.out)
            elif self.variant == "packed":
                e.factor_eval_packed(self.model, self.meas, self.lin, self.q, self.states, out=self.out)
            elif self.variant == "hessian":
                e.factor_hessian(self.model, self.meas, self.lin, self.q, self.states, self.R, out=self.out)
            elif self.variant == "whitened":
                e.factor_eval(self.model, self.meas, self.lin, self.q, self.states, out=self.out, sqrt_info=self.R)
            else:
                e.factor_eval(self.model, self.meas, self.lin, self.q, self.states, out=self.out)
            self.i += 1
            return self.out
        out = self.outs[self.i % len(self.outs)]
        self.calls[self.i % len(self.calls)]()
        self.i += 1
        return out

    def graph_steps(self, steps):
        """Steps per captured graph for a run of `steps`: all of them up to GRAPH_MAX_STEPS, else a multiple of the walk's period
        (the pre-bound (batch, output set) pairs), so that every replay starts where the next steps of one long graph would."""
        if steps <= GRAPH_MAX_STEPS:
            return steps
        period = 1 if self.is_factor else len(self.calls)
        return max(1, GRAPH_MAX_STEPS // period) * period

    def capture(self, steps):
        """The next `steps` steps as ONE HIP graph (a kernel node per launch; "V1 full" forks its side stream inside the
        capture).  Returns the graph, or None when this workload / runtime cannot be captured (eager launches then)."""
        i0 = self.i
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.step()                                  # warm-up on a side stream, as graph capture requires
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            self.i = i0
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(steps):
                    self.step()
            self.i = i0
            return g
        except Exception as ex:                              # pragma: no cover - depends on the runtime
            sys.stderr.write("bench.py: HIP graph capture failed (%r): eager launches\n" % (ex,))
            self.i = i0
            torch.cuda.synchronize()
            return None


# ------------------------------------------------------------------------------------------------ multi-GPU exchange
def final_gather(out, W_local, mode="root", dst=0, recv=None):
    """The path's one exchange step: the per-rank output slabs of a step.  mode "root": to rank `dst` only
    (every peer sends straight to the root); "all": all-gather.  Returns the gathered blocks
    (name -> [world, W_local, n]) on the ranks that hold them, else None.  Works on any backend (gloo in the CPU tests)."""
    from cpi_amd.dist import gather_packed, gather_to_root
    if mode == "none":
        return None
    assert "_flat" in out, "the gather moves ONE packed slab per rank (Engine.alloc_outputs(packed=True))"
    if mode == "all":
        return gather_packed(out["_flat"], out["_fields"], W_local)
    return gather_to_root(out["_flat"], out["_fields"], W_local, dst=dst, out=recv)


def time_steps(wl, steps, warmup, dist_on=False, gather="root", schedule="final", graph=True):
    """W untimed warm-up steps, then EXACTLY `steps` timed steps.  Both sides of the timed region are bracketed by
    barrier + synchronize; a rank's clock stops when its own part (steps + its share of the exchange) is complete, BEFORE
    the closing barrier -- the caller reduces the wall times with MAX over ranks.
    Returns dict(wall seconds, kernel_ms = HIP events around the K steps on the launch stream, gather_ms = the exposed
    exchange tail after the last kernel, mode = "graph" | "eager")."""
    import torch.distributed as dist
    out = None
    for _ in range(warmup):
        out = wl.step()
    torch.cuda.synchronize()
    do_gather = dist_on and gather != "none" and not wl.is_factor
    pipelined = do_gather and schedule == "pipelined" and len(wl.outs) >= 2
    chunked = do_gather and schedule == "chunked" and getattr(wl, "k", 0) >= 1 and gather == "root"
    plan = []                                                # [(graph, replays)]: the K steps as replays of at most two graphs
    if graph and not pipelined and not chunked:
        per = wl.graph_steps(steps)
        plan = [(wl.capture(n), reps) for n, reps in ((per, steps // per), (steps % per, 1)) if n]
        if any(g is None for g, _ in plan):
            plan = []                                        # a capture failed: eager launches
    for g, _ in plan:
        g.replay()                                           # untimed: the first replay of a graph uploads it
    torch.cuda.synchronize()
    recv, side, gathered = [None, None], None, None
    if dist_on:
        if do_gather:
            if out is None:
                out = wl.step()
            # untimed: first use of the collective (RCCL channel set-up), and the root's receive buffers
            if chunked:
                # one receive buffer per (output set, sub-block): a sub-block's slab is overwritten only by the same sub-block two steps later
                nsets = len(wl.outs)
                crecv = [[None] * wl.k for _ in range(nsets)]
                if dist.get_rank() == 0:
                    for s_ in range(nsets):
                        for c in range(wl.k):
                            crecv[s_][c] = torch.empty((dist.get_world_size(), wl.chunk_outs[s_][c]["_flat"].numel()), dtype=torch.float64,
                                                       device=out["_flat"].device)
                co = wl.chunk_outs[0][0]
                final_gather(co, co["_flat"].numel() // sum(n for _, n in co["_fields"]), gather, recv=crecv[0][0])
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
            else:
                if gather == "root" and dist.get_rank() == 0:
                    shape = (dist.get_world_size(), out["_flat"].numel())
                    recv = [torch.empty(shape, dtype=torch.float64, device=out["_flat"].device) for _ in range(2 if pipelined else 1)]
                    if not pipelined:
                        recv = recv * 2
                final_gather(out, wl.W, gather, recv=recv[0])
                torch.cuda.synchronize()
                if pipelined:
                    side = torch.cuda.Stream()
        dist.barrier()
        torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    i0 = wl.i
    t0 = time.perf_counter()
    e0.record()
    if chunked:
        # the exchange INSIDE a step: sub-block c's slab travels on the side stream while sub-block c + 1 (or the next step's first
        # one) computes; a sub-block's slab and receive buffer are rewritten only after their previous gather has drained
        cur = torch.cuda.current_stream()
        nsets = len(wl.outs)
        ev_done = [[None] * wl.k for _ in range(nsets)]
        parts = None
        for kstep in range(steps):
            s_ = wl.i % nsets
            parts = []
            for c in range(wl.k):
                if ev_done[s_][c] is not None:
                    cur.wait_event(ev_done[s_][c])
                co = wl.chunk_step(c)
                ready = torch.cuda.Event(); ready.record(cur)
                if kstep == steps - 1 and c == wl.k - 1:
                    e1.record(cur)
                side.wait_event(ready)
                with torch.cuda.stream(side):
                    wc = co["_flat"].numel() // sum(n for _, n in co["_fields"])
                    parts.append(final_gather(co, wc, gather, recv=crecv[s_][c]))
                    done = torch.cuda.Event(); done.record(side)
                ev_done[s_][c] = done
            wl.i += 1
        cur.wait_stream(side)
        e2.record(cur)
        if parts and parts[0] is not None:     # the root: sub-blocks back together, [world, W, n] per field
            from cpi_amd.dist import assemble_chunks
            gathered = assemble_chunks(parts, wl.W)
    elif pipelined:
        # step k's slab travels on the side stream while step k + 1 computes into the other output set; a set is rewritten
        # only after its gather has drained (ev_done), the root's receive buffers alternate likewise
        cur = torch.cuda.current_stream()
        ev_done = [None, None]
        for k in range(steps):
            if ev_done[k & 1] is not None:
                cur.wait_event(ev_done[k & 1])
            out = wl.step()
            ready = torch.cuda.Event(); ready.record(cur)
            if k == steps - 1:
                e1.record(cur)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                gathered = final_gather(out, wl.W, gather, recv=recv[k & 1])
                done = torch.cuda.Event(); done.record(side)
            ev_done[k & 1] = done
        cur.wait_stream(side)
        e2.record(cur)
    else:
        if plan:
            for g, reps in plan:
                for _ in range(reps):
                    g.replay()
            wl.i = i0 + steps
        else:
            for _ in range(steps):
                wl.step()
        e1.record()                                  # HIP events on the launch stream: kernel time only
        gathered = final_gather(wl.out_of(i0 + steps - 1), wl.W, gather, recv=recv[0]) if do_gather else None
        e2.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0                  # this rank's part is complete (the root: every slab has arrived)
    if dist_on:
        dist.barrier()                               # closing barrier: outside the timed region
        torch.cuda.synchronize()
    return {"wall": wall, "kernel_ms": e0.elapsed_time(e1), "gather_ms": e1.elapsed_time(e2) if do_gather else 0.0,
            "mode": ("chunked-eager" if chunked else ("pipelined-eager" if pipelined else ("graph" if plan else "eager"))),
            "graph_steps": wl.graph_steps(steps) if plan else 0, "gathered": gathered, "last_step": i0 + steps - 1}


def dump_outputs(arrays, path, limit=DUMP_LIMIT_BYTES, seed=DUMP_SAMPLE_SEED):
    """--dump-outputs: every array (name -> tensor, one row per window / factor, the same number of rows in all) as
    path/<name>.npy in float64.  When the arrays together exceed `limit` bytes, the same fixed, seeded sample of rows (in
    ascending order) is kept from each, so that two builds run with the same arguments write files that compare row for row."""
    import numpy as np
    rows = {t.shape[0] for t in arrays.values()}
    assert len(rows) == 1, "the outputs of one step have one row per window / factor: %r" % {k: tuple(t.shape) for k, t in arrays.items()}
    R = rows.pop()
    row_bytes = sum(t[:1].numel() * 8 for t in arrays.values())
    keep = min(R, (limit - 256 * len(arrays)) // row_bytes)          # 256 bytes per file for the .npy header (128 in practice)
    idx = None if keep == R else torch.from_numpy(np.sort(np.random.default_rng(seed).choice(R, keep, replace=False)))
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        if idx is not None:
            t = t.index_select(0, idx.to(t.device))
        np.save(os.path.join(path, name + ".npy"), t.to(torch.float64).cpu().numpy())
    return keep


# ------------------------------------------------------------------------------------------------ CPU legs
def usable_cpus():
    """Threads worth starting: the affinity mask capped by the cgroup CPU quota.  (The GPU boxes of this pool show 256
    logical CPUs but run the container under cpu.max = 16 CPUs; with 256 threads the same code is 2x SLOWER than with
    16 -- measured with tests/tools/cpu_scale.py: 42 k windows/s at 16 threads, 20 k at 256.)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                quota, period = int(f.read()), int(g.read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except Exception:
            pass
    return n


def _cpu_factor_rows(wl, min_seconds, cores):
    """CPU legs of the factor-shaped rows (kind "port": the reference's factor TUs need GTSAM, which is absent).
    evaluateError itself = the C restatement, threaded over factors; what GTSAM does next (square-root information,
    whitening, Hessian blocks) = numpy / LAPACK on one core, as the tests' checker does it."""
    import numpy as np
    from oracle import oracle_py as op
    orc = op.oracle()
    F = min(wl.W, 20000)
    meas = {k: v[:F].cpu().numpy() for k, v in wl.meas.items() if k != "P"}
    rec = op.factor_records(meas, wl.lin[:F].cpu().numpy(), wl.q[:F].cpu().numpy() if wl.q is not None else None)
    st = wl.states[:F + 1].cpu().numpy()
    xi, xj = np.ascontiguousarray(st[:-1]), np.ascontiguousarray(st[1:])
    if wl.kind == "predict":
        n = min(F, 20000)
        orc.predict(wl.model, rec[:64], xi[:64])
        t0, done = time.perf_counter(), 0
        while True:
            orc.predict(wl.model, rec[:n], xi[:n])
            done += n
            el = time.perf_counter() - t0
            if el >= min_seconds:
                break
        return {"value": done / el, "unit": "factors/s", "cores": 1, "kind": "port", "single_core_value": done / el,
                "sample": "%d passes over %d of the row's factors through the C restatement of getpredictedstate_v%d "
                          "(GraphSolver_IMU.cpp:263-307), one thread" % (done // n, n, wl.model)}
    if wl.kind == "sqrt_info":
        n = min(F, 4000)
        import cpi_amd
        P = (cpi_amd.unpack_sym(wl.P[:n]) if wl.P.shape[1] == 120 else wl.P[:n]).cpu().numpy().reshape(n, 15, 15)
        t0, done = time.perf_counter(), 0
        while True:
            np.linalg.cholesky(np.linalg.inv(P))             # R^T (GTSAM: Covariance -> Information(P^-1) -> LLT)
            done += n
            el = time.perf_counter() - t0
            if el >= min_seconds:
                break
        return {"value": done / el, "unit": "factors/s", "cores": 1, "kind": "port", "single_core_value": done / el,
                "sample": "%d passes over %d of the row's covariances through numpy / LAPACK: chol(inv(P)), batched, one thread "
                          "(GTSAM's Gaussian::Covariance is not in the reference tree)" % (done // n, n)}
    buf = (np.ones((F, 15)), np.ones((F, 225)), np.ones((F, 225)))
    orc.factor_batch(wl.model, rec[:256], xi[:256], xj[:256], nthreads=cores)
    extra = None
    if wl.variant in ("whitened", "hessian"):
        nR = min(F, 4000)
        import cpi_amd
        R = (cpi_amd.unpack_tri(wl.R[:nR]) if wl.R.shape[1] == 120 else wl.R[:nR]).cpu().numpy().reshape(nR, 15, 15).transpose(0, 2, 1)

        def extra(e, H1, H2):
            A1, A2, b = R @ H1[:nR].reshape(nR, 15, 15).transpose(0, 2, 1), R @ H2[:nR].reshape(nR, 15, 15).transpose(0, 2, 1), -(R @ e[:nR, :, None])
            if wl.variant == "hessian":
                A = np.concatenate([A1, A2, b], axis=2)
                return A.transpose(0, 2, 1) @ A
            return A1
    t0, done, t_extra, n_extra = time.perf_counter(), 0, 0.0, 0
    while True:
        orc.factor_batch(wl.model, rec, xi, xj, nthreads=cores, out=buf)
        done += F
        if extra is not None:
            t1 = time.perf_counter(); extra(*buf); t_extra += time.perf_counter() - t1; n_extra += min(F, 4000)
        el = time.perf_counter() - t0
        if el >= min_seconds:
            break
    per_factor = (el - t_extra) / done + (t_extra / n_extra if n_extra else 0.0)
    fs = min(F, 5000)
    t1 = time.perf_counter(); orc.factor_batch(wl.model, rec[:fs], xi[:fs], xj[:fs], nthreads=1); t1 = time.perf_counter() - t1
    what = {"dense": "", "packed": "", "whitened": " + numpy whitening (R e, R H1, R H2; one thread, %d factors per pass)" % min(F, 4000),
            "hessian": " + numpy whitening and [A1 A2 b]^T [A1 A2 b] (one thread, %d factors per pass)" % min(F, 4000)}[wl.variant]
    return {"value": 1.0 / per_factor, "unit": "factors/s", "cores": cores, "kind": "port", "single_core_value": fs / t1,
            "sample": "%d passes over %d of the sweep's factors (residual + dense H1 / H2, the C restatement of "
                      "ImuFactorCPIv%d::evaluateError -- the reference's factor TUs need GTSAM), %d threads%s"
                      % (done // F, F, wl.model, cores, what)}


def cpu_baseline(wl, min_seconds=8.0):
    """The CPU path timed beside a row, on this box's host cores, on a bounded sample of the SAME inputs.
    Preintegration rows: the reference's own CpiV1 / CpiV2 (oracle/_ref, kind "reference") -- which always integrates means
    + bias Jacobians + covariance, so it is like-for-like for the *_full rows and does MORE than the GPU for the
    mean-only rows (the reference has no mean-only mode; said in `sample`).  Forster comparator, the evaluateError
    sweeps and the SURVEY 8(f) rows: the C restatement / numpy (kind "port"; GTSAM / the factor TUs cannot be built here)."""
    import numpy as np
    from oracle import oracle_py as op
    from oracle.oracle_py import OUT_DOUBLES
    cores = usable_cpus()
    if wl.is_factor:
        return _cpu_factor_rows(wl, min_seconds, cores)
    ref = op.reference()
    lib, kind = (ref, "reference") if ref is not None else (op.oracle(), "port")
    if wl.model == 3:   # the Forster comparator lives in GTSAM (absent): only the restatement exists
        lib, kind = op.oracle(), "port"
    if wl.kind == "tiled":   # the CPU leg reads the same windows in the dense order: un-tile the first tiles of batch 0
        tiles, _, lin, q = wl.batches[0]
        nb = min(tiles.shape[0], 157)
        kn = tiles[:nb].permute(0, 3, 1, 2).reshape(nb * 64, wl.N + 1, 7)[:min(wl.W, nb * 64)].contiguous().cpu().numpy()
        lin, q = lin[:kn.shape[0]].cpu().numpy(), q[:kn.shape[0]].cpu().numpy()
    else:
        kn, lin, q = [t[:10000].cpu().numpy() for t in wl.batches[0]]
    Wc = kn.shape[0]
    prm = op.make_params(wl.model, 0, 1)
    raw = np.ones((Wc, OUT_DOUBLES))                               # reused, already touched output buffer
    lib.run(prm, kn[:256], lin[:256], q[:256], nthreads=cores)     # warm
    t0, done = time.perf_counter(), 0
    while True:
        lib.run(prm, kn, lin, q, nthreads=cores, raw=raw)
        done += Wc
        el = time.perf_counter() - t0
        if el >= min_seconds:
            break
    port = None
    if wl.model in (1, 2):
        port = sparse_port_rate(wl, kn, lin, q, cores, min(2.0, min_seconds / 3))
    ws = min(Wc, (1500 if wl.model == 1 else 600) * 50 // max(50, wl.N))
    t1 = time.perf_counter(); lib.run(prm, kn[:ws], lin[:ws], q[:ws], nthreads=1); t1 = time.perf_counter() - t1
    what = {1: "CpiV1::feed_IMU", 2: "CpiV2::feed_IMU (stj = 1)", 3: "the Forster restatement"}[wl.model]
    note = "" if "cov" in wl.want else "; no mean-only mode in the reference: CPU figure incl. Jacobians + covariance"
    res = {"value": done / el, "unit": "windows/s", "cores": cores, "kind": kind, "single_core_value": ws / t1,
           "sample": ("%d passes x %d of the row's %d-sample windows via %s, %d threads (cgroup quota; %d CPUs)%s"
                      % (done // Wc, Wc, wl.N, what, cores, os.cpu_count() or 1, note))[:200]}
    if port:
        res["sparse_port"] = port
    return res


def sparse_port_rate(wl, kn, lin, q, cores, seconds):
    """Second CPU figure beside the dense reference (SURVEY.md 8(d) asks for both): the kernels' OWN sparse arithmetic
    (cpi_amd/csrc/cpi_math.hpp compiled for the host by tests/hostsim -- column-lane covariance recursion, or the mean-only
    recursion for mean-only rows, which is the LIKE-FOR-LIKE CPU figure the reference cannot give: it has no mean-only
    mode), on the same windows, all usable cores and one core.  g++ -O2, no hand vectorisation: a port, not a tuned CPU code."""
    from concurrent.futures import ThreadPoolExecutor
    from tests import hostsim_py as hs
    mean_only = "cov" not in wl.want
    Wc = kn.shape[0]

    def run(lo, hi):
        if mean_only:
            hs.mean(wl.model, 0, 0, 1, kn[lo:hi], lin[lo:hi], q[lo:hi])
        else:
            hs.cov(wl.model, 0, kn[lo:hi], lin[lo:hi], q[lo:hi])
            if wl.model == 1:
                hs.mean(1, 1, 0, 1, kn[lo:hi], lin[lo:hi], q[lo:hi])      # model 1: the analytic Jacobians are a second pass
    hs.lib()
    n1 = min(Wc, 2000 if mean_only else 200)
    t = time.perf_counter(); run(0, n1); t = time.perf_counter() - t
    single = n1 / t
    Wp = int(min(Wc, max(cores * 16, single * cores * seconds)))
    cuts = [Wp * i // cores for i in range(cores + 1)]
    passes = 0
    with ThreadPoolExecutor(cores) as ex:
        t0 = time.perf_counter()
        while True:
            list(ex.map(lambda i: run(cuts[i], cuts[i + 1]), range(cores)))
            passes += 1
            t = time.perf_counter() - t0
            if t >= seconds:
                break
    Wp *= passes
    return {"value": Wp / t, "unit": "windows/s", "cores": cores, "kind": "port", "single_core_value": single,
            "what": ("mean-only recursion (like for like with the GPU row)" if mean_only else
                     "sparse column-lane covariance recursion" + (" + analytic Jacobians" if wl.model == 1 else " with the state-transition Jacobians")),
            "sample": "%d window evaluations (%d passes) over %d threads; %d windows on one thread" % (Wp, passes, cores, n1)}


# ------------------------------------------------------------------------------------------------ counters
def load_pmc(build_id):
    """profiles/r05_pmc.json: rocprofv3 --pmc passes of tools/pmc_collect.sh, stamped with the build id of the library
    they were collected on.  Used only when that stamp equals the LOADED library's cpi_build_id(); otherwise the
    counter-derived fields are null (the file is stale for this library)."""
    try:
        with open(PMC_FILE) as f:
            d = json.load(f)
    except Exception:
        return {}, "no %s" % os.path.relpath(PMC_FILE, ROOT)
    if d.get("build_id") != build_id:
        return {}, "%s was collected on build %s, the loaded library is %s" % (os.path.relpath(PMC_FILE, ROOT), d.get("build_id"), build_id)
    return d.get("rows", {}), "%s (build %s)" % (os.path.relpath(PMC_FILE, ROOT), build_id)


def roofline_of(name, W, N, launch_s, pmc_rows, pmc_note):
    """The contract's roofline object for one row: achieved = ALGORITHMIC bytes per launch / launch duration."""
    bpu = bytes_per_unit(name, N)
    achieved = bpu * W / launch_s / 1e9
    row = pmc_rows.get("%s:%d:%d" % (name, W, N))
    r = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
         "traffic": row.get("traffic_bytes") if row else None,
         "traffic_unit": "HBM bytes per launch = (2*FETCH_SIZE + WRITE_SIZE) KiB, rocprofv3 --pmc; " + pmc_note,
         "algorithmic_bytes_per_launch": bpu * W, "algorithmic_bytes_per_unit": bpu,
         "kernel": WORKLOADS[name]["kernel"], "launch_us": launch_s * 1e6}
    ul = WORKLOADS[name].get("useful_lanes")
    if row and row.get("fp64_flop"):
        # FP64 work counted by the SQ instruction counters of the same library: (2 FMA + MUL + ADD + TRANS) x 64 lanes
        tf = row["fp64_flop"] / launch_s / 1e12
        r["fp64"] = {"TFLOPs": tf, "peak": FP64_PEAK_TFLOPS, "frac": tf / FP64_PEAK_TFLOPS, "source": "counters",
                     "flop_per_launch": row["fp64_flop"], "valu_insts_per_launch": row.get("valu_insts"),
                     "fp64_insts_per_launch": row.get("fp64_insts")}
    elif name in FLOP_EST:
        tf = FLOP_EST[name] * W / launch_s / 1e12
        r["fp64"] = {"TFLOPs": tf, "peak": FP64_PEAK_TFLOPS, "frac": tf / FP64_PEAK_TFLOPS,
                     "source": "estimate (SURVEY.md 8(d) sparse-minimal flop midpoints; no counters for this build)"}
    if ul and "fp64" in r and r["fp64"]["source"] == "counters":
        # the instruction counters count 64 lanes per instruction; the column-lane recursion keeps ul[0] of every ul[1]
        # lanes on a useful column (the rest run as harmless zero columns): the useful share of the counted work
        r["fp64"]["useful_lanes"] = "%d of %d" % ul
        r["fp64"]["useful_frac"] = r["fp64"]["frac"] * ul[0] / ul[1]
        if name in ("v1_full", "cfg5_full"):
            r["fp64"]["useful_note"] = "applied to the whole row: a lower bound -- the analytic-Jacobian kernel of this row keeps all lanes busy"
    return r


def overlapped_rate(W, N, nctxs, steps):
    """Whole-job rate when independent batches are issued round-robin through several engine contexts (one HIP stream each,
    cpi_amd.EnginePool), so that consecutive launches overlap -- the one route to north_star's 40 % of the HBM roof at
    configs[1]'s 10 000 windows per launch.  With overlapping launches the duration of one launch is no longer the inverse of the
    throughput (which is what `roofline` is defined on), so this is reported as its own object (`overlapped`): seconds per
    batch = wall time of `steps` batches / steps, for every context count of `nctxs`.  Same pool of > 256 MiB of distinct batches
    as the headline."""
    import cpi_amd
    from cpi_amd import synth
    dev = torch.device("cuda", torch.cuda.current_device())
    nmax = max(nctxs)
    pool = cpi_amd.EnginePool(nmax, device=dev)
    nb = max(nmax, -(-(MALL_BYTES * 5 // 4) // (W * (N + 1) * 56)))
    batches = [synth.make_windows(W, N, seed=977 + b, device=dev) for b in range(nb)]
    # every context (stream) writes into a ring of output sets of its OWN: launches on one stream are ordered, so a set is only ever
    # rewritten behind its previous writer -- a schedule a correct caller can run (round 5 shared one ring across the streams:
    # unordered launches on different streams could be handed the same set)
    RING = 3
    outs = [[pool.engines[0].alloc_outputs(W, ("mean",), 1) for _ in range(RING)] for _ in range(nmax)]
    prm = pool.engines[0].make_params(1)
    per = {}
    for nctx in nctxs:
        def go(k):
            for i in range(k):
                kn, lin, q = batches[i % nb]
                pool.engines[i % nctx].preintegrate(kn, lin, q, prm, want=("mean",), out=outs[i % nctx][(i // nctx) % RING])
        torch.cuda.synchronize()
        go(max(50, steps // 10))
        torch.cuda.synchronize()
        best = 1e30
        for _ in range(2):
            t0 = time.perf_counter()
            go(steps)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / steps)
        per[nctx] = best
    # The same round-robin as ONE HIP graph (fork from the capture stream into the contexts' streams, join at the end): no host
    # launch cost between the batches -- what a caller that replays a fixed schedule gets, and the figure that says what the GPU
    # itself does with overlapping launches (the eager figure above can be bound by ~3-4 us of host work per launch).
    graph = {}
    try:
        nsteps = 600
        for nctx in nctxs:
            cap = torch.cuda.Stream(device=dev)
            cap.wait_stream(torch.cuda.current_stream(dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=cap):
                for st in pool.streams[:nctx]:
                    st.wait_stream(cap)
                for i in range(nsteps):
                    kn, lin, q = batches[i % nb]
                    pool.engines[i % nctx].preintegrate(kn, lin, q, prm, want=("mean",), out=outs[i % nctx][(i // nctx) % RING])
                for st in pool.streams[:nctx]:
                    cap.wait_stream(st)
            g.replay()
            torch.cuda.synchronize()
            best = 1e30
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(5):
                    g.replay()
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t0) / (5 * nsteps))
            graph[nctx] = best
            del g
    except Exception as ex:             # pragma: no cover - depends on the runtime's cross-stream capture
        sys.stderr.write("bench.py: multi-stream graph capture failed (%r): eager figures only\n" % (ex,))
        graph = {}
    pool.close()
    return per, graph


# ------------------------------------------------------------------------------------------------ launch
def respawn(gpus):
    """`python bench.py --gpus N` with no launcher: become the launcher (one rank per GPU, RCCL)."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execve(sys.executable, cmd, env)


EXTRA_PRERAMP_MS = 100.0   # the extra rows: their kernels are heavier in arithmetic than the headline's, the controller takes longer to settle


def preramp(wl, ms):
    """Untimed clock pre-ramp, separate from the W warm-up steps: an idle MI355X needs tens of milliseconds of load to reach
    its steady shader clock, so a short (K, W) would otherwise time the ramp (K = 20: 14.9 us per launch instead of 12.0)."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        for _ in range(50 if wl.W <= 100000 else 2):
            wl.step()
        torch.cuda.synchronize()


EXTRA_ROWS = (("v1_mean", 30000, 1000), ("v1_mean", 100000, 300), ("v1_mean", 1000000, 40),
              ("v1_full", 100000, 30), ("v2_full", 100000, 30), ("forster_full", 100000, 30),
              ("factor_v1", 1000000, 40), ("factor_v2", 1000000, 40),
              ("factor_v1_packed", 1000000, 40), ("factor_v2_packed", 1000000, 40),
              ("sqrt_info", 1000000, 20), ("factor_v1_whitened", 1000000, 20), ("factor_v2_whitened", 1000000, 20),
              ("factor_v1_hessian", 1000000, 20), ("factor_v2_hessian", 1000000, 20),
              ("predict_v1", 1000000, 40), ("predict_v2", 1000000, 40),
              ("cfg5_mean", 1000000, 10), ("cfg5_full", 1000000, 3),
              ("v1_mean_tiled", 1000000, 40), ("v2_mean_tiled", 1000000, 40), ("v1_mean_tiled", 10000, 1000),
              ("v1_mean_stream", 1000000, 40), ("v1_full_stream", 100000, 30), ("v2_full_stream", 100000, 30),
              # round 6, ABI 3: the SURVEY 8(f1) rows on packed triangles (P_sym in, R_tri through the sweeps) and the packed covariance output
              ("sqrt_info_packed", 1000000, 20), ("factor_v1_whitened_tri", 1000000, 20), ("factor_v2_whitened_tri", 1000000, 20),
              ("factor_v1_hessian_tri", 1000000, 20), ("factor_v2_hessian_tri", 1000000, 20),
              ("v1_full_sym", 100000, 30), ("v2_full_sym", 100000, 30),
              # round 6: the window lengths the reference itself runs -- imurate / camrate = 10 (100 Hz IMU) and 20 (200 Hz):
              # cpi_compare/launch/synthetic_test.launch:27-28; (name, windows, steps, samples)
              ("v1_mean", 1000000, 40, 10), ("v1_mean", 1000000, 40, 20), ("v1_mean", 10000, 1000, 10), ("v1_mean", 10000, 1000, 20),
              ("v1_full", 1000000, 5, 10), ("v1_full", 1000000, 3, 20), ("v2_full", 1000000, 3, 10), ("v2_full", 1000000, 3, 20),
              ("v1_mean_tiled", 1000000, 40, 10), ("v1_mean_tiled", 1000000, 40, 20), ("v1_mean_stream", 1000000, 40, 10), ("v1_mean_stream", 1000000, 40, 20))


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        respawn(a.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist_on = world > 1 or bool(os.environ.get("CPI_BENCH_FORCE_DIST"))  # env: exercise the RCCL path with one rank
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the engine has no CPU path)")
    if rank == 0 and world != a.gpus:
        sys.stderr.write("bench.py: --gpus %d but the launcher started %d rank(s); reporting n_gpus = %d\n" % (a.gpus, world, world))
    # CPI_BENCH_SINGLE_DEVICE=1: rehearsal of the N-rank flow on a box with ONE GPU (tests/test_gpu_group.py) -- every rank
    # computes on cuda:0 and the exchange goes through gloo (RCCL refuses two ranks on one device).  Not a measurement.
    rehearsal = bool(os.environ.get("CPI_BENCH_SINGLE_DEVICE"))
    if rehearsal:
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        sys.exit("bench.py: rank %d needs device %d but this node shows %d GPU(s) -- one rank per GPU (--gpus N <= devices); "
                 "CPI_BENCH_SINGLE_DEVICE=1 rehearses the N-rank flow on one device" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    if dist_on:
        import torch.distributed as dist
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    import cpi_amd
    from cpi_amd.dist import shard_bounds, unshard
    eng = cpi_amd.Engine(device=local_rank)
    build_id = (eng.lib.cpi_build_id() or b"").decode()
    pmc_rows, pmc_note = load_pmc(build_id)
    spec = WORKLOADS[a.workload]
    N = a.samples or spec["N"]
    W_job = a.windows or spec["W"]                   # per GPU (weak) or in total (strong)
    if a.scaling == "strong" and world > 1:
        lo, hi, W = shard_bounds(W_job, rank, world)  # equal padded block per rank; W = block size
        total_units = W_job
    else:
        W = W_job
        total_units = W_job * world
    is_factor = spec["kind"] not in ("pre", "tiled", "stream")
    do_gather = dist_on and a.gather != "none" and not is_factor
    # schedule of the exchange: per-step, overlapped gathers pay when a step lasts long enough to hide one (>= ~1 ms:
    # covariance rows, million-window batches); the 10 k-window headline keeps the single final gather
    step_bytes = bytes_per_unit(a.workload, N) * W
    schedule = a.gather_schedule
    if schedule == "auto":
        schedule = "pipelined" if (do_gather and a.gather == "root" and ("cov" in spec.get("want", ()) or step_bytes > (256 << 20))) else "final"
    base_seed = lambda r: 20190101 + 7919 * r
    if schedule == "chunked" and not (do_gather and a.gather == "root" and spec["kind"] == "pre"):
        schedule = "final"                            # nothing to chunk: one rank, no exchange, or not the dense layout
    wl = Workload(eng, a.workload, W, N, seed=base_seed(rank), lanes=a.lanes, min_out_sets=2 if (do_gather and schedule in ("pipelined", "chunked")) else 1)
    if schedule == "chunked":
        wl.make_chunks(max(1, a.gather_chunks))
    PRERAMP_MS = float(os.environ.get("CPI_BENCH_PRERAMP_MS", "60"))     # (the override is for A/B runs of the pre-ramp itself)
    preramp(wl, PRERAMP_MS)
    wl.i = 0     # the pre-ramp runs for a TIME, i.e. a rank-dependent number of steps: every rank walks the batch pool from the same index
    tm = time_steps(wl, a.steps, a.warmup, dist_on, a.gather, schedule, graph=not a.eager)
    if a.dump_outputs and rank == 0:
        # what the caller of the timed path holds after its last step: the gathered blocks at the root, else this rank's outputs
        got = tm["gathered"]
        dump_outputs(unshard(got, total_units) if got else wl.outputs_of(tm["last_step"]), a.dump_outputs)
    wall, kern_ms, gather_ms = tm["wall"], tm["kernel_ms"], tm["gather_ms"]
    wall_ng = None
    if do_gather:     # the same K steps without the exchange step, beside it
        wall_ng = time_steps(wl, a.steps, min(a.warmup, 5), dist_on, "none", "final", graph=not a.eager)["wall"]
    if dist_on:
        import torch.distributed as dist
        t = torch.tensor([wall, kern_ms, gather_ms, wall_ng or 0.0], dtype=torch.float64, device="cpu" if rehearsal else eng.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, kern_ms, gather_ms, wall_ng = t[0].item(), t[1].item(), t[2].item(), (t[3].item() if wall_ng is not None else None)
    value = total_units * a.steps / wall
    launch_s = kern_ms * 1e-3 / a.steps
    unit = "factors" if is_factor else "windows"
    cfg_note = ""
    if a.workload == "v1_mean" and W_job == 10000 and N == 50:
        cfg_note = ", CPI model 1, mean-only (BASELINE.json configs[1])"
    elif a.workload.startswith("cfg5"):
        cfg_note = ", BASELINE.json configs[4]: 8 M windows x 100 samples over 8 GPUs = this per-GPU share, generated on the device"
    res = {
        "metric": "evaluateError factors/sec" if is_factor else "preintegration windows/sec (%d-sample windows)" % N,
        "value": value, "unit": unit + "/s",
        # filled below when this run measures them: `value` is the LIGHTEST configuration (mean-only); the full integrator's rate
        # (configs[2]: CPI-v2 + covariance + Jacobians) and the overlapped rate of the same headline workload stand beside it
        "value_full_integrator": None, "value_overlapped": None,
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": wall * 1e3 / a.steps,
        "higher_is_better": True, "scaling": a.scaling if world > 1 else "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic" if not rehearsal else "synthetic (REHEARSAL: all ranks on one GPU, gloo exchange -- not a measurement)",
        "config": {"workload": "%s: %d %s x %d samples per GPU per step%s" % (a.workload, W, unit, N, cfg_note),
                   "pool_batches": wl.nbatch, "clock_preramp_ms": PRERAMP_MS, "library_build": build_id,
                   "launch_mode": {"graph": ("%d timed steps replayed as ONE HIP graph (one kernel node per step)" % a.steps if tm["graph_steps"] == a.steps else
                                             "%d timed steps replayed as HIP graphs of %d steps (one kernel node per step)" % (a.steps, tm["graph_steps"])),
                                   "eager": "%d eager launches" % a.steps,
                                   "pipelined-eager": "%d eager launches, each followed by its gather on a side stream" % a.steps,
                                   "chunked-eager": "%d steps of %d sub-block launches, each sub-block's slab gathered on a side stream while the next "
                                                    "one computes" % (a.steps, getattr(wl, "k", 1))}[tm["mode"]],
                   "parallelism": ("1 GPU" if world == 1 else
                                   "%s scaling: %d %s per step on each of %d GPUs, no data-path collective; exchange = %s (%s schedule); "
                                   "value = MAX over ranks of each rank's own wall time, closing barrier outside the timed region" % (
                                       a.scaling, W, unit, world, {"root": "gather of ONE packed slab per peer to rank 0",
                                                                   "all": "all_gather", "none": "skipped"}[a.gather], schedule))},
        "roofline": roofline_of(a.workload, W, N, launch_s, pmc_rows, pmc_note),
    }
    if a.workload == "v1_mean" and N == 50:
        # north_star: >= 40 % of the HBM-read roofline.  One launch of 10 000 windows cannot reach it on this chip (reading the
        # batch alone takes 8.2 us = 0.45); said here, in the line, not only in prose
        res["goal_40pct_hbm"] = bool(res["roofline"]["frac"] >= 0.40)
        res["goal_note"] = ("north_star asks >= 0.40 of 8 TB/s: reached from ~17 k windows per launch (30 k: 0.47, 1 M: 0.57) or with several "
                            "batches in flight (`overlapped`, measured with --full); one 10 k-window launch is launch / first-burst bound")
        if rank == 0 and world == 1 and a.full and not a.no_extra and W == 10000:
            # the same workload issued through 2 / 3 / 4 engine contexts (HIP streams): consecutive launches overlap
            try:
                per, gper = overlapped_rate(W, N, (2, 3, 4), 3000)
                bpb = bytes_per_unit("v1_mean", N) * W
                best = gper if gper else per                 # the graph replay when the runtime captured it, else the eager issue (`mode` says which; both are kept)
                res["overlapped"] = {"contexts": 3, "value": W / best[3], "unit": "windows/s", "ms_per_batch": best[3] * 1e3,
                                     "frac": bpb / best[3] / 1e9 / HBM_PEAK_GBS, "batches": 3000,
                                     "mode": "graph" if gper else "eager",
                                     "frac_by_contexts": {str(k): round(bpb / v / 1e9 / HBM_PEAK_GBS, 4) for k, v in best.items()},
                                     "frac_eager_by_contexts": {str(k): round(bpb / v / 1e9 / HBM_PEAK_GBS, 4) for k, v in per.items()},
                                     "how": "independent batches round-robin over N contexts (one HIP stream + own output ring each); graph: 600 batches "
                                            "as ONE HIP graph, 5 replays; eager: 3000 host launches; wall / batches = an aggregate rate"}
                res["goal_40pct_hbm_overlapped"] = bool(res["overlapped"]["frac"] >= 0.40)
                res["value_overlapped"] = res["overlapped"]["value"]
            except Exception as ex:       # an additional object must never cost the line
                res["overlapped"] = {"error": repr(ex)}
    if dist_on:
        import torch.distributed as dist
        res["config"]["gather_schedule"] = schedule if do_gather else "none"
        res["config"]["kernel_ms"] = kern_ms
        res["config"]["gather_ms"] = gather_ms
        res["config"]["wall_ms"] = wall * 1e3
        # whole-job rate of the K steps alone: sum of units / MAX over ranks of the HIP-event time around the K steps -- the
        # collective tail of a 0.3 ms timed region is separable from the kernels this way
        res["config"]["value_kernel_only"] = total_units * a.steps / (kern_ms * 1e-3)
        try:
            res["config"]["rccl"] = rccl_info(rehearsal, eng)
        except Exception as ex:      # an informational field must never cost the line
            res["config"]["rccl"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "error": repr(ex)}
    if wall_ng is not None:
        res["config"]["value_without_gather"] = total_units * a.steps / wall_ng
        res["config"]["ms_final_gather"] = max(0.0, (wall - wall_ng) * 1e3)
    if dist_on and do_gather:
        # kernel time per step for the prediction: the same K steps WITHOUT the exchange (`wall_ng`) -- in the chunked / pipelined
        # schedules the HIP-event time around the K steps includes the waits for a slab's previous gather
        k_ms = wall_ng * 1e3 if wall_ng else kern_ms
        res["config"]["predicted"] = predicted_exchange(wl, world, a.steps, schedule, k_ms, total_units, getattr(wl, "k", 1))
    if world > 1:
        # a collective-latency-shaped `value` explains itself: how long the timed region is, and how much of it is the exchange
        share = (gather_ms / (wall * 1e3)) if (do_gather and wall > 0) else 0.0
        res["config"]["scaling_note"] = (
            "timed region %.3f ms = %d steps (%.3f ms of kernels, HIP events) + %.3f ms of exposed exchange (%.0f %% of the region; %s schedule): "
            "%s  Scaling efficiency of the hot path itself: value_kernel_only / (n_gpus x the 1-GPU value); with the exchange: value." % (
                wall * 1e3, a.steps, kern_ms, gather_ms, 100.0 * share, schedule if do_gather else "no",
                ("the exchange is a third or more of a region of a few milliseconds, so `value` is shaped by the collective's latency, not by the "
                 "kernels -- the millisecond-per-step rows (`--workload cfg5_mean`, `--scaling strong --workload v2_full`) are the ones a curve means something on."
                 if share >= 0.3 else "the steps dominate the region.")))
    if do_gather and a.gather == "root":
        res["config"].update(verify_gather(eng, wl, tm, world, rank, base_seed, rehearsal))
    extra = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu:
        res["cpu_baseline"] = cpu_baseline(wl, 8.0)
    if rank == 0 and world == 1 and a.full and not a.no_extra:
        extra = []
        del wl
        torch.cuda.empty_cache()
        for name, Wx, steps, *rest in EXTRA_ROWS:
            try:
                Nx = rest[0] if rest else WORKLOADS[name]["N"]
                w2 = Workload(eng, name, Wx, Nx, seed=4242)
                # untimed, like the headline's: a row that starts on an idle GPU (the previous row's CPU leg) would otherwise time the power
                # controller's transient -- the launches of `sqrt_info_packed` in one 260-launch trace: 345-363 us at the idle clock, 600 us a
                # dozen launches later, 395-400 us from the hundredth on (profiles/r06_raw/r06_seq.txt); the steady state is the rate of a sweep
                preramp(w2, EXTRA_PRERAMP_MS)
                t2 = time_steps(w2, steps, max(2, steps // 10), graph=not a.eager)
                ls = t2["kernel_ms"] * 1e-3 / steps
                row = {"workload": name, "units_per_step": Wx, "samples": Nx, "value": Wx * steps / t2["wall"],
                       "unit": ("factors" if w2.is_factor else "windows") + "/s", "launch_ms": ls * 1e3, "launch_mode": t2["mode"], "clock_preramp_ms": EXTRA_PRERAMP_MS,
                       "roofline": roofline_of(name, Wx, Nx, ls, pmc_rows, pmc_note)}
                if w2.assembly:
                    asm = dict(w2.assembly)
                    asm["share_of_step"] = asm["ms_per_batch"] / (ls * 1e3)
                    row["assembly"] = asm
                skip_cpu = (name.endswith("_packed") and name != "sqrt_info_packed") or name.endswith("_stream") or name.endswith("_tri") or name.endswith("_sym") or \
                    (name == "v1_mean" and Wx != 1000000) or (name.endswith("_tiled") and (Wx != 1000000 or Nx != 50))
                if not a.no_cpu and not skip_cpu:
                    row["cpu_baseline"] = cpu_baseline(w2, 2.5)     # bounded: ~2.5 s of CPU work per row
                extra.append(row)
                del w2
                torch.cuda.empty_cache()
            except Exception as ex:  # an extra config must never take the headline down
                extra.append({"workload": name, "units_per_step": Wx, "samples": rest[0] if rest else WORKLOADS[name]["N"], "error": repr(ex)})
        ov = res.get("overlapped", {})
        if "value" in ov:
            extra.append({"workload": "v1_mean_3ctx", "units_per_step": 10000, "value": ov["value"], "unit": "windows/s", "contexts": 3,
                          "us_per_batch": ov["ms_per_batch"] * 1e3, "hbm_GBs": ov["frac"] * HBM_PEAK_GBS, "hbm_frac": ov["frac"],
                          "note": "the headline's `overlapped` object: " + ov["how"]})
    if dist_on:
        import torch.distributed as dist
        dist.destroy_process_group()
    if rank == 0:
        emit(res, extra)


def predicted_exchange(wl, world, steps, schedule, kern_ms, total_units, chunks=1):
    """What the exchange SHOULD cost on xGMI, stated before anyone measures it: every peer sends its slab over
    its OWN link straight to the root, so the wire time of a gather is one slab / one link's one-way rate, whatever N is.  From
    that and the kernel time measured in THIS run the expected wall time of the timed region under the schedule in use:
      final      K steps of kernels, then one slab                               K k + e
      pipelined  step i's slab under step i + 1's kernels                        k + (K - 1) max(k, e) + e
      chunked    c sub-blocks per step, sub-block j's slab under sub-block j + 1 K max(k, e) + min(k, e) / c
    A prediction to judge the first real-RCCL run against (and the rehearsals' gloo exchange says nothing about it)."""
    fields = wl.outs[0]["_fields"]
    slab = wl.W * sum(n for _, n in fields) * 8
    e = slab / (XGMI_LINK_GBS_ONE_WAY * 1e9) * 1e3            # ms per slab
    k = kern_ms / steps                                        # ms of kernels per step, measured
    if schedule == "pipelined":
        region = k + (steps - 1) * max(k, e) + e
    elif schedule == "chunked":
        region = steps * max(k, e) + min(k, e) / max(1, chunks)
    else:
        region = steps * k + e
    return {"slab_bytes_per_peer": slab, "slab_doubles_per_window": sum(n for _, n in fields), "peers": max(0, world - 1),
            "link_GBs_one_way": XGMI_LINK_GBS_ONE_WAY,
            "link_source": "AMD: 153.6 GB/s per Infinity Fabric link, bidirectional; one direction = 76.8 GB/s; one link per peer into the root",
            "root_ingress_GBs": XGMI_LINK_GBS_ONE_WAY * max(0, world - 1),
            "exchange_ms_per_slab": e, "kernel_ms_per_step_measured": k, "schedule": schedule, "chunks": chunks if schedule == "chunked" else None,
            "expected_region_ms": region, "expected_value": total_units * steps / (region * 1e-3),
            "expected_value_without_gather": total_units * steps / (steps * k * 1e-3),
            "exchange_bound": bool(e > k) if schedule != "final" else None,
            "note": "wire ceiling only: no protocol / launch overhead (RCCL's small-message latency is tens of microseconds)"}


def rccl_info(rehearsal, eng):
    """What the collective library actually saw (the driver's "did RCCL see N ranks" check): backend, world size, one
    (rank, device index, PCI bus id) triple per rank -- collected over the process group itself -- and the library version."""
    import torch.distributed as dist
    dev = eng.device.index or 0
    props = torch.cuda.get_device_properties(dev)
    mine = [dist.get_rank(), dev, "%04x:%02x:%02x" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0), getattr(props, "pci_device_id", 0))]
    every = [None] * dist.get_world_size()
    dist.all_gather_object(every, mine)
    try:
        ver = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:
        ver = None
    return {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "ranks": every,
            "distinct_devices": len({(e[1], e[2]) for e in every}), "nccl_version": ver if not rehearsal else None,
            "link_types": link_types() if dist.get_rank() == 0 else None}


def link_types():
    """What connects the GPUs of this node (`rocm-smi --showtopotype`: XGMI / PCIE per pair), so that the first scaling record says
    whether the gather really went over xGMI.  {"GPU0": {"GPU1": "XGMI", ...}, ...}, or a short error string; never raises."""
    import re
    import subprocess
    try:
        p = subprocess.run(["rocm-smi", "--showtopotype"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=20)
        return parse_link_types(p.stdout) or {"raw": " ".join(p.stdout.split())[:300]}
    except Exception as ex:
        return "unavailable: %r" % (ex,)


def parse_link_types(text):
    """The matrix `rocm-smi --showtopotype` prints (header row "GPU0 GPU1 ...", then one row per device: "GPU0 0 XGMI ...") ->
    {"GPU0": {"GPU1": "XGMI", ...}, ...}; the diagonal ("0") is dropped; a 1-GPU box gives {"GPU0": {}}."""
    import re
    head, out = None, {}
    for ln in text.splitlines():
        w = ln.split()
        if w and all(re.fullmatch(r"GPU\d+", x) for x in w):
            head = w
        elif head and w and re.fullmatch(r"GPU\d+", w[0]) and len(w) == len(head) + 1:
            out[w[0]] = {h: v for h, v in zip(head, w[1:]) if h != w[0]}
    return out


def verify_gather(eng, wl, tm, world, rank, base_seed, rehearsal):
    """After the timed region: rank 0 regenerates EVERY rank's batch of the last timed step (the synthetic generator is
    seeded per rank and batch), computes it on its own GPU with the launch geometry the owning rank used, and asserts that
    the block that arrived through the exchange is BITWISE equal; then the same windows as ONE unsharded call of world x W
    windows (the auto lane split of the mean kernel may differ there: compared at the 2e-13 regression gate, not bitwise)."""
    import torch.distributed as dist
    from cpi_amd import synth
    ok, maxdiff, why = None, None, None
    if wl.kind != "pre":
        why = "not verified: only the dense-layout workloads regenerate another rank's batch"
    elif rank == 0:
        try:
            g = tm.get("gathered")
            b = tm["last_step"] % wl.nbatch
            ok, maxdiff = g is not None, 0.0
            parts = []
            k = getattr(wl, "k", 1) if tm.get("mode") == "chunked-eager" else 1

            def recompute(kn, lin, q):
                """with the launch geometry the owning rank used: the chunked schedule launches W / k windows at a time (the mean
                kernel's automatic lane split depends on the launch size)"""
                if k <= 1:
                    return eng.preintegrate(kn, lin, q if wl.model != 3 else None, wl.prm, want=wl.want)
                from cpi_amd.dist import chunk_bounds
                pieces = []
                for c in range(k):
                    lo, hi, _ = chunk_bounds(wl.W, c, k)
                    if hi > lo:
                        pieces.append(eng.preintegrate(kn[lo:hi], lin[lo:hi], q[lo:hi] if wl.model != 3 else None, wl.prm, want=wl.want))
                return {name: torch.cat([p_[name] for p_ in pieces], dim=0) for name in pieces[0]}
            for r in range(world if g is not None else 0):
                kn, lin, q = synth.make_windows(wl.W, wl.N, seed=base_seed(r) + 101 * b, device=eng.device)
                out = recompute(kn, lin, q)
                torch.cuda.synchronize()
                for name, n in wl.outs[0]["_fields"]:
                    ok = ok and torch.equal(g[name][r].reshape(out[name].shape), out[name])
                parts.append((kn, lin, q))
                del out
            if ok and world * wl.W * (wl.N + 1) * 56 <= (64 << 30):
                kn = torch.cat([p[0] for p in parts]); lin = torch.cat([p[1] for p in parts]); q = torch.cat([p[2] for p in parts])
                del parts
                out = eng.preintegrate(kn, lin, q if wl.model != 3 else None, wl.prm, want=wl.want)
                torch.cuda.synchronize()
                for name, n in wl.outs[0]["_fields"]:
                    got, ref = g[name].reshape(out[name].shape), out[name]
                    scale = ref.abs().amax().clamp_min(1.0) if name != "P" else ref.abs().amax().clamp_min(1e-300)
                    maxdiff = max(maxdiff, float(((got - ref).abs().amax() / scale).item()))
                ok = ok and maxdiff <= 2e-13
        except Exception as ex:      # the verification must never cost the timing record (e.g. no memory for N regenerated batches)
            ok, why = None, "not verified: %r" % (ex,)
            torch.cuda.empty_cache()
    flag = torch.tensor([1.0 if ok else (0.0 if ok is not None else -1.0)], dtype=torch.float64, device="cpu" if rehearsal else eng.device)
    dist.broadcast(flag, src=0)
    if flag.item() == 0.0:
        # a mismatch is reported IN the line (gather_verified: false) so that the timing record survives; CPI_BENCH_STRICT=1 (the
        # tests) turns it into a non-zero exit on every rank
        sys.stderr.write("bench.py: the gathered outputs of the last timed step DIFFER from rank 0's recomputation\n")
        if os.environ.get("CPI_BENCH_STRICT"):
            raise SystemExit(3)
    how = why or ("rank 0 recomputed every rank's last-step batch: gathered blocks %s; one unsharded call over all %d x %d windows "
                  "agrees to %.1e (relative; gate 2e-13)" % ("bitwise equal" if ok else "DIFFER (or the unsharded call is off the gate)", world, wl.W, maxdiff or 0.0))
    return {"gather_verified": (bool(ok) if ok is not None else None) if rank == 0 else None, "gather_verified_how": how}


def row_key(r):
    """Key of an extra row in the line's compact `extra_rows`: workload@units ("1M", "100k" ... for round counts), "xN" appended for the
    short-window rows (samples != the workload's own N)."""
    u = r["units_per_step"]
    us = "%dM" % (u // 1000000) if u % 1000000 == 0 and u else ("%dk" % (u // 1000) if u % 1000 == 0 and u else "%d" % u)
    own = WORKLOADS.get(r["workload"], {}).get("N")
    return "%s@%s%s" % (r["workload"], us, "" if r.get("samples") in (None, own) else "x%d" % r["samples"])


def emit(res, extra):
    """Rank 0.  The LAST stdout line is ONE JSON object of < 6 KB: the headline with its roofline and cpu_baseline, a compact
    `configs2` object (BASELINE configs[2]: the row the >= 10 M windows/s goal sits on), the end-to-end route table of a
    1 M x 50 batch and one [launch_ms, roofline frac] pair per extra row.  The full rows (each with roofline, counters and CPU
    leg) go to bench_extra.json beside this file (and a copy under gpurun_out/ when that directory exists)."""
    if extra is not None:
        rows = {row_key(r): r for r in extra}
        c2 = rows.get("v2_full@100k")
        if c2 and "error" not in c2:
            fp, cb = c2["roofline"].get("fp64", {}), c2.get("cpu_baseline", {})
            res["value_full_integrator"] = c2["value"]
            res["configs2"] = {"workload": "v2_full: 100000 windows x 50 samples, CPI-v2 + 15x15 covariance + bias Jacobians (BASELINE configs[2])",
                               "value": c2["value"], "unit": "windows/s", "goal_10M_windows_per_s": bool(c2["value"] >= 1e7),
                               "launch_ms": c2["launch_ms"], "kernel": c2["roofline"]["kernel"], "bound": "fp64 valu / lds",
                               "fp64": {"frac": fp.get("frac"), "useful_frac": fp.get("useful_frac"), "TFLOPs": fp.get("TFLOPs"), "peak": FP64_PEAK_TFLOPS,
                                        "source": fp.get("source")},
                               "hbm_frac": c2["roofline"]["frac"], "traffic": c2["roofline"]["traffic"],
                               "cpu_baseline": {k: cb.get(k) for k in ("value", "cores", "kind", "single_core_value")}}
        ms = lambda k: (rows[k]["launch_ms"] if k in rows and "error" not in rows[k] else None)
        asm = (rows.get("v1_mean_tiled@1M") or {}).get("assembly", {}).get("ms_per_batch")
        res["routes_1M_x_50"] = {"what": "ms per batch of 1 M windows x 50 samples held as ONE IMU stream + update times (GraphSolver_IMU.cpp:50-69), means out",
                                 "stream_in_place": ms("v1_mean_stream@1M"),
                                 "assemble_tiles": asm, "tiled_kernel": ms("v1_mean_tiled@1M"),
                                 "assemble_plus_tiled_first_use": (asm + ms("v1_mean_tiled@1M")) if asm and ms("v1_mean_tiled@1M") else None,
                                 "dense_kernel_preassembled": ms("v1_mean@1M")}
        sig = lambda x: float("%.4g" % x)
        res["extra_rows"] = {k: ([sig(r["launch_ms"]), round(r["roofline"]["frac"], 3)] if "roofline" in r else
                                 ([sig(r["us_per_batch"] * 1e-3), round(r["hbm_frac"], 3)] if "hbm_frac" in r else "error"))
                             for k, r in rows.items()}
        res["extra_rows_key"] = "[launch ms, algorithmic bytes / launch / 8 TB/s]"
        doc = {"headline": {k: v for k, v in res.items() if k not in ("extra_rows", "extra_rows_key")}, "rows": extra}
        paths = [os.path.join(ROOT, "bench_extra.json")]
        if os.path.isdir(os.path.join(ROOT, "gpurun_out")):
            paths.append(os.path.join(ROOT, "gpurun_out", "bench_extra.json"))
        for pth in paths:
            try:
                with open(pth, "w") as f:
                    json.dump(doc, f, indent=1)
            except OSError as ex:
                sys.stderr.write("bench.py: could not write %s (%r)\n" % (pth, ex))
        res["extra_file"] = "bench_extra.json (%d rows, each with roofline / counters / cpu_baseline)" % len(extra)
    line = json.dumps(res)
    for drop in ("extra_rows", "routes_1M_x_50", "goal_note", "extra_rows_key"):   # the contract: one line the driver can parse (< 6 KB)
        if len(line) < 6000:
            break
        res.pop(drop, None)
        line = json.dumps(res)
    # RCCL prints its banner through C stdio: flush that first so the JSON line is the LAST line of stdout
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    print(line, flush=True)


if __name__ == "__main__":
    main()
