"""The measurement at arbitrary times: what cpi_query_batch costs, beside the only way the library had before.  Needs a GPU.

  python tools/query_bench.py [--out profiles/query_bench.json] [--reps 21] [--queries 1000000] [--windows 10000] [--intervals 50]

Workload: Q queries (default 1 M) spread uniformly over the time spans of W x N windows (default 10 k x 50), model 1, means only.
Timed with device events around each call, after a warm-up, --reps times; median, minimum and maximum:
  query_sorted   cpi_query_batch, the queries sorted by (window, time) -- a lidar sweep as it comes off the sensor
  query_random   cpi_query_batch, the same queries in random order
  running        the cpi_preintegrate_running call that produced the rows the queries read (once per batch, not per query)
  prefix_batch   the alternative without the entry: ONE ragged cpi_preintegrate_batch over Q windows assembled on the host, window k =
                 [knot 0 .. knot i, {t_q, w_i, a_i}] of the queried window -- a copy of the knots and O(N) intervals per query.
                 The assembly (numpy, host clock) and the upload are reported separately and are NOT part of its kernel time.
Bytes: a query needs its (window, time) pair (12), knot i (56), the window's linearisation point (48), one row in (88) and one row
out (88) = 292 bytes; the stamps the bisection probes (ceil(log2(N + 1)) x 8, served by the caches for sorted queries) are not
counted.  Q x 292 bytes over the median time is given as a share of 8 TB/s.  Prints one JSON document (with the library's build
id) and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
QUERY_BYTES = 12 + 56 + 48 + 88 + 88


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return {"median": 1e6 * float(np.median(ts)), "min": 1e6 * float(np.min(ts)), "max": 1e6 * float(np.max(ts))}


def prefix_windows(kn, qw, qt):
    """The ragged batch a caller without cpi_query_batch assembles: window k = knots 0 .. i of window qw[k] and the tail knot
    {qt[k], w_i, a_i}.  Returns (knots [K, 7], first [Q], count [Q])."""
    W, n1, _ = kn.shape
    t = kn[:, :, 0]
    i = np.clip((t[qw] <= qt[:, None]).sum(axis=1) - 1, 0, n1 - 1)     # the largest knot index with t_i <= t_q
    count = (i + 1).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(i + 2)[:-1]]).astype(np.int64)
    K = int((i + 2).sum())
    within = np.arange(K) - np.repeat(first, i + 2)
    src = np.minimum(within, np.repeat(i, i + 2))               # the tail knot repeats knot i ...
    knots = kn[np.repeat(qw, i + 2), src]
    knots[first + i + 1, 0] = qt                                # ... with the query's stamp
    return knots, first, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--queries", type=int, default=1_000_000)
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
    prm = eng.make_params(1)
    rows = eng.preintegrate_running(kn, lin, q, prm, want=("mean",))
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    qw_r = torch.randint(0, W, (Q,), generator=g, dtype=torch.int32)
    kn_h = kn.cpu().numpy()
    t0, t1 = kn_h[:, 0, 0], kn_h[:, N, 0]
    qt_r = torch.from_numpy(t0[qw_r.numpy()] + torch.rand((Q,), generator=g, dtype=torch.float64).numpy() * (t1 - t0)[qw_r.numpy()])
    order = np.lexsort((qt_r.numpy(), qw_r.numpy()))
    sets = {"query_random": (qw_r, qt_r), "query_sorted": (qw_r[order], qt_r[order])}
    out = eng.alloc_outputs(Q, ("mean",), 1)
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "W": W, "N": N, "Q": Q, "model": 1, "request": "mean", "bytes_per_query": QUERY_BYTES}
    doc["running_us"] = timed(lambda: eng.preintegrate_running(kn, lin, q, prm, want=("mean",), out=rows), a.reps)
    results = {}
    for name, (qw, qt) in sets.items():
        dqw, dqt = qw.to(eng.device), qt.to(eng.device)
        doc[name + "_us"] = timed(lambda: eng.query(kn, lin, rows, dqw, dqt, params=prm, out=out), a.reps)
        doc[name + "_share_of_8TBps"] = Q * QUERY_BYTES / (doc[name + "_us"]["median"] * 1e-6) / HBM
        results[name] = {k: v.clone() for k, v in out.items()}
        print(json.dumps({name + "_us": doc[name + "_us"]}), flush=True)
    # the alternative: Q prefix windows with tail knots, assembled on the host (the queries in sorted order)
    qw, qt = (x.numpy() for x in sets["query_sorted"])
    c0 = time.perf_counter()
    pk, pf, pc = prefix_windows(kn_h, qw, qt)
    doc["prefix_assembly_s"] = time.perf_counter() - c0
    doc["prefix_knot_bytes"] = int(pk.nbytes)
    c0 = time.perf_counter()
    dk, df, dc = (torch.from_numpy(x).to(eng.device) for x in (pk, pf, pc))
    dlin = lin[sets["query_sorted"][0].to(eng.device).long()].contiguous()
    torch.cuda.synchronize()
    doc["prefix_upload_s"] = time.perf_counter() - c0
    pout = eng.alloc_outputs(Q, ("mean",), 1)
    doc["prefix_batch_us"] = timed(lambda: eng.preintegrate(dk, dlin, None, prm, want=("mean",), first=df, count=dc, N=N + 1, out=pout), a.reps)
    doc["prefix_batch_over_query_sorted"] = doc["prefix_batch_us"]["median"] / doc["query_sorted_us"]["median"]
    doc["largest_difference"] = {k: float((pout[k] - results["query_sorted"][k]).abs().max()) for k in pout}
    print(json.dumps(doc), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
