"""Running preintegration: what the measurement after EVERY interval costs (cpi_preintegrate_running).  Needs a GPU.

  python tools/running_bench.py [--out profiles/running_bench.json] [--reps 7] [--quick]

Per shape (W windows x N intervals) and request -- means only (model 1), model 1 everything (means + Jacobians + P), model 2
means + P -- four ways to the same W * N rows are timed in one process, in alternation, with device events around each:
  running   one cpi_preintegrate_running call
  clamped   what the library offered before, (a): N cpi_preintegrate_batch calls with count clamped to 1, 2, ... N
  chain     what the library offered before, (b): a chain of N one-interval cpi_preintegrate_resume calls over carry records
  batch     ONE plain cpi_preintegrate_batch call on the same windows (final states only): running / batch is the price of the rows
(the two older ways write each step's [W] outputs into one scratch set: the copy into rows a caller would still need is not
charged to them).  For the means-only request the bytes the call writes (88 per row) over its time are given as a share of
8 TB/s.  Median, minimum and maximum of --reps runs after a warm-up.  Prints one JSON document (with the library's build id)
and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REQUESTS = {   # name -> (model, want of the running call, want of the older entries, bytes written per row)
    "mean_m1": (1, ("mean",), ("mean",), 88),
    "all_m1": (1, ("mean", "jac", "cov"), ("mean", "jac", "cov"), 88 + 360 + 1800),
    "mean_cov_m2": (2, ("mean", "cov"), ("mean", "cov"), 88 + 1800),
}
HBM = 8.0e12


def timed(fn, reps):
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
    return ts


def bench_shape(eng, name, W, N, reps):
    from cpi_amd import synth
    model, want, want_old, row_bytes = REQUESTS[name]
    kn, lin, q = synth.make_windows(W, N, seed=505 + model, device=eng.device)
    prm = eng.make_params(model)
    rows = eng.preintegrate_running(kn, lin, q, prm, want=want)
    scratch = eng.alloc_outputs(W, want_old, model)
    flat = kn.view(W * (N + 1), 7)
    base = torch.arange(W, dtype=torch.int64, device=eng.device) * (N + 1)
    firsts = [(base + i).contiguous() for i in range(N)]
    counts = [torch.full((W,), i + 1, dtype=torch.int32, device=eng.device) for i in range(N)]
    cd = eng.carry_doubles(model)
    ca = torch.empty((W, cd), dtype=torch.float64, device=eng.device)
    cb = torch.empty_like(ca)

    def running():
        eng.preintegrate_running(kn, lin, q, prm, want=want, out=rows)

    def clamped():
        for i in range(N):
            eng.preintegrate(kn, lin, q, prm, want=want_old, count=counts[i], out=scratch)

    def chain():
        cin, cout = None, ca
        for i in range(N):
            eng.preintegrate_resume(flat, lin, q, prm, want=want_old, first=firsts[i], count=counts[0], N=1, carry_in=cin,
                                    carry_out=cout, out=scratch)
            cin, cout = cout, (cb if cout is ca else ca)

    def batch():
        eng.preintegrate(kn, lin, q, prm, want=want_old, out=scratch)

    fns = {"running": running, "clamped": clamped, "chain": chain, "batch": batch}
    ts = {k: [] for k in fns}
    for k, fn in fns.items():      # warm-up of every variant, then alternate
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k] += timed(fn, 1)
    rec = {"request": name, "model": model, "W": W, "N": N, "rows": W * N, "bytes_written": W * N * row_bytes}
    for k, v in ts.items():
        rec[k + "_us"] = {"median": 1e6 * float(np.median(v)), "min": 1e6 * float(np.min(v)), "max": 1e6 * float(np.max(v))}
    med = {k: float(np.median(v)) for k, v in ts.items()}
    rec["clamped_over_running"] = med["clamped"] / med["running"]
    rec["chain_over_running"] = med["chain"] / med["running"]
    rec["running_over_batch"] = med["running"] / med["batch"]
    rec["write_rate_TBps"] = rec["bytes_written"] / med["running"] / 1e12
    if name == "mean_m1":
        rec["write_share_of_8TBps"] = rec["bytes_written"] / med["running"] / HBM
    rec["faster_than_both"] = bool(med["running"] < med["clamped"] and med["running"] < med["chain"])
    del rows, scratch, kn, firsts, counts, ca, cb
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "running_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the two smallest batch sizes only")
    a = ap.parse_args()
    import cpi_amd
    assert torch.cuda.is_available(), "needs a GPU"
    eng = cpi_amd.Engine()
    shapes = []
    for W in ((549, 27_450) if a.quick else (549, 27_450, 100_000)):
        for N in (20, 50):
            for name in REQUESTS:
                shapes.append((name, W, N))
    if not a.quick:
        shapes += [("mean_m1", 1_000_000, 20), ("mean_m1", 1_000_000, 50)]
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    for name, W, N in shapes:
        rec = bench_shape(eng, name, W, N, a.reps)
        doc["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    doc["running_faster_than_both_everywhere"] = all(r["faster_than_both"] for r in doc["shapes"])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({"out": a.out, "running_faster_than_both_everywhere": doc["running_faster_than_both_everywhere"]}))


if __name__ == "__main__":
    main()
