"""The covariance at arbitrary times: what cpi_query_cov_batch costs, beside what a caller had to do before.  Needs a GPU.

  python tools/query_cov_bench.py [--out profiles/query_cov_bench.json] [--reps 21] [--queries 200000] [--windows 10000] [--intervals 50]

Workload: Q queries (default 200 k) spread uniformly over the time spans of W x N windows (default 10 k x 50), the queries sorted by
(window, time), for models 1 and 2; request: P_sym (the form cpi_sqrt_information_packed_batch reads).  Per model, timed with
device events around each call after a warm-up, --reps times, the two routes ALTERNATING call by call; median, minimum, maximum:
  query_cov      cpi_query_cov_batch: P_sym out from rows that hold q and P_sym
  prefix_batch   the route without the entry: ONE ragged cpi_preintegrate_batch with P_sym over Q windows assembled on the host,
                 window k = [knot 0 .. knot i, {t_q, w_i, a_i}] of the queried window (tools/query_bench.py: prefix_windows) -- a copy
                 of the knots and O(N) intervals of the covariance recursion per query.  Its assembly and upload are reported
                 separately and are NOT part of its kernel time.
  running        the cpi_preintegrate_running call (means + P_sym) that produces the rows, once per batch of windows
Bytes a query moves: its (window, time) pair (12), knot i (56), the linearisation point (48 + 32 for model 2), the row's q (32) and
P_sym (960) in, P_sym out (960).  Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from query_bench import prefix_windows   # noqa: E402


def alternating(fns, reps, warm=3):
    """Times the calls of fns (name -> callable) in turn, reps rounds: {name: {median, min, max}} in microseconds."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_cov_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--queries", type=int, default=200_000)
    ap.add_argument("--windows", type=int, default=10_000)
    ap.add_argument("--intervals", type=int, default=50)
    a = ap.parse_args()
    assert a.reps >= 20, "20 or more repeats"
    import cpi_amd
    from cpi_amd import synth
    assert torch.cuda.is_available(), "needs a GPU"
    eng = cpi_amd.Engine()
    W, N, Q = a.windows, a.intervals, a.queries
    kn, lin, q = synth.make_windows(W, N, seed=2024, device=eng.device, edge_cases=False)
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    qw = torch.randint(0, W, (Q,), generator=g, dtype=torch.int32).numpy()
    kn_h = kn.cpu().numpy()
    t0, t1 = kn_h[:, 0, 0], kn_h[:, N, 0]
    qt = t0[qw] + torch.rand((Q,), generator=g, dtype=torch.float64).numpy() * (t1 - t0)[qw]
    order = np.lexsort((qt, qw))
    qw, qt = qw[order], qt[order]
    dqw, dqt = torch.from_numpy(qw).to(eng.device), torch.from_numpy(qt).to(eng.device)
    c0 = time.perf_counter()
    pk, pf, pc = prefix_windows(kn_h, qw, qt)
    assembly = time.perf_counter() - c0
    c0 = time.perf_counter()
    dk, df, dc = (torch.from_numpy(x).to(eng.device) for x in (pk, pf, pc))
    dlin, dq = lin[dqw.long()].contiguous(), q[dqw.long()].contiguous()
    torch.cuda.synchronize()
    upload = time.perf_counter() - c0
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "W": W, "N": N,
           "Q": Q, "request": "P_sym", "order": "sorted by (window, time)", "prefix_assembly_s": assembly, "prefix_upload_s": upload,
           "prefix_knot_bytes": int(pk.nbytes), "models": {}}
    for model in (1, 2):
        prm = eng.make_params(model)
        rows = eng.preintegrate_running(kn, lin, q, prm, want=("mean", "cov_sym"))
        src = {"q": rows["q"], "P_sym": rows["P_sym"]}
        out = eng.alloc_outputs(Q, ("cov_sym",), model)
        pout = eng.alloc_outputs(Q, ("cov_sym",), model)
        m = alternating({
            "query_cov_us": lambda: eng.query(kn, lin, src, dqw, dqt, q_k_lin=q, params=prm, want=("cov_sym",), out=out),
            "prefix_batch_us": lambda: eng.preintegrate(dk, dlin, dq, prm, want=("cov_sym",), first=df, count=dc, N=N + 1, out=pout),
            "running_us": lambda: eng.preintegrate_running(kn, lin, q, prm, want=("mean", "cov_sym"), out=rows),
        }, a.reps)
        m["prefix_batch_over_query_cov"] = m["prefix_batch_us"]["median"] / m["query_cov_us"]["median"]
        m["bytes_per_query"] = 12 + 56 + 48 + (32 if model == 2 else 0) + 32 + 960 + 960
        m["query_cov_bytes_per_s"] = Q * m["bytes_per_query"] / (m["query_cov_us"]["median"] * 1e-6)
        scale = pout["P_sym"].abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
        m["largest_difference_over_largest_entry"] = float(((out["P_sym"] - pout["P_sym"]).abs() / scale).max())
        doc["models"][str(model)] = m
        print(json.dumps({"model": model, **m}), flush=True)
    print(json.dumps(doc), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
