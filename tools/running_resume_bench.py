"""Running preintegration from a carry record: what IMU-rate rows cost for a window that ARRIVES IN CHUNKS
(cpi_preintegrate_running_resume).  Needs a GPU.

  python tools/running_resume_bench.py [--out profiles/running_resume_bench.json] [--reps 7] [--quick]

A window of N = 50 intervals arrives in C = N / n chunks of n = 5, 10, 25 intervals.  Per batch size W and request -- means only
(model 1), model 1 everything (means + Jacobians + P), model 2 means + P -- four ways to the same W * N rows are timed in one
process, in alternation, with device events around the whole window:
  new       C cpi_preintegrate_running_resume calls, one per chunk, over two carry records used in turn
  rerun     what gives the same rows without it, (a): cpi_preintegrate_running on the prefix so far at every chunk (the rows of
            earlier chunks are computed and written again each time: C (C + 1) / 2 chunks of work)
  chain     what gives the same rows without it, (b): n one-interval cpi_preintegrate_resume calls per chunk (each step's [W]
            outputs go into one scratch set: the copy into rows a caller would still need is not charged)
  one_shot  ONE cpi_preintegrate_running call on the whole window: new / one_shot is the price of chunked arrival
Also given per shape: the bytes of carry record a `new` chunk moves (read + written, per window) beside the bytes of rows it
writes -- at n = 5 a model-2 window moves 2 x 4.5 KB of record for 9.4 KB of rows.  Median, minimum and maximum of --reps runs
after a warm-up of every variant.  Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REQUESTS = {   # name -> (model, want, bytes written per row, doubles of the carry record the request reads and writes)
    "mean_m1": (1, ("mean",), 88, 17),
    "all_m1": (1, ("mean", "jac", "cov"), 88 + 360 + 1800, 287),
    "mean_cov_m2": (2, ("mean", "cov"), 88 + 1800, 17 + 27 * 18),
}
N = 50
CHUNKS = (5, 10, 25)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def bench_shape(eng, name, W, n, reps):
    from cpi_amd import synth
    model, want, row_bytes, rec_doubles = REQUESTS[name]
    kn, lin, q = synth.make_windows(W, N, seed=505 + model, device=eng.device)
    prm = eng.make_params(model)
    C = N // n
    store = eng.alloc_outputs(W * N, want, model)                                      # one set of row arrays: one_shot's, and every prefix of rerun

    def view(Np):
        return {k: v[:W * Np].view((W, Np) + tuple(v.shape[1:])) for k, v in store.items()}
    rows = view(N)
    seg = [kn[:, c * n:(c + 1) * n + 1].contiguous() for c in range(C)]               # the chunks as they arrive (shared boundary knots)
    seg_rows = eng.preintegrate_running_resume(seg[0], lin, q, prm, want=want)[0]      # [W, n, ...]: a chunk's rows
    prefix = [kn[:, :(c + 1) * n + 1].contiguous() for c in range(C)]
    prefix_rows = [view((c + 1) * n) for c in range(C)]
    scratch = eng.alloc_outputs(W, want, model)
    flat = kn.view(W * (N + 1), 7)
    base = torch.arange(W, dtype=torch.int64, device=eng.device) * (N + 1)
    firsts = [(base + i).contiguous() for i in range(N)]
    ones = torch.ones((W,), dtype=torch.int32, device=eng.device)
    cd = eng.carry_doubles(model)
    ca = torch.empty((W, cd), dtype=torch.float64, device=eng.device)
    cb = torch.empty_like(ca)

    def new():
        cin, cout = None, ca
        for c in range(C):
            eng.preintegrate_running_resume(seg[c], lin, q, prm, want=want, carry_in=cin, carry_out=cout, out=seg_rows)
            cin, cout = cout, (cb if cout is ca else ca)

    def rerun():
        for c in range(C):
            eng.preintegrate_running(prefix[c], lin, q, prm, want=want, out=prefix_rows[c])

    def chain():
        cin, cout = None, ca
        for i in range(N):
            eng.preintegrate_resume(flat, lin, q, prm, want=want, first=firsts[i], count=ones, N=1, carry_in=cin, carry_out=cout,
                                    out=scratch)
            cin, cout = cout, (cb if cout is ca else ca)

    def one_shot():
        eng.preintegrate_running(kn, lin, q, prm, want=want, out=rows)

    fns = {"new": new, "rerun": rerun, "chain": chain, "one_shot": one_shot}
    ts = {k: [] for k in fns}
    for fn in fns.values():        # warm-up of every variant, then alternate
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    rec = {"request": name, "model": model, "W": W, "N": N, "n": n, "chunks": C, "rows_bytes_per_window_per_chunk": n * row_bytes,
           "record_bytes_per_window_per_chunk": 2 * 8 * rec_doubles}
    for k, v in ts.items():
        rec[k + "_us"] = {"median": 1e6 * float(np.median(v)), "min": 1e6 * float(np.min(v)), "max": 1e6 * float(np.max(v))}
    med = {k: float(np.median(v)) for k, v in ts.items()}
    spread = float(np.max(ts["new"]) - np.min(ts["new"]))
    rec["rerun_over_new"] = med["rerun"] / med["new"]
    rec["chain_over_new"] = med["chain"] / med["new"]
    rec["new_over_one_shot"] = med["new"] / med["one_shot"]
    rec["new_spread_us"] = 1e6 * spread
    rec["not_slower_than_rerun"] = bool(med["new"] <= med["rerun"] + spread)
    rec["not_slower_than_chain"] = bool(med["new"] <= med["chain"] + spread)
    # what the record requires: not slower than rerun from 4 chunks on, not slower than the chain anywhere
    rec["meets_requirement"] = bool((C < 4 or rec["not_slower_than_rerun"]) and rec["not_slower_than_chain"])
    del rows, store, seg, seg_rows, prefix, prefix_rows, scratch, kn, firsts, ca, cb
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "running_resume_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the two smallest batch sizes only")
    a = ap.parse_args()
    import cpi_amd
    assert torch.cuda.is_available(), "needs a GPU"
    eng = cpi_amd.Engine()
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    for W in ((549, 27_450) if a.quick else (549, 27_450, 100_000)):
        for n in CHUNKS:
            for name in REQUESTS:
                rec = bench_shape(eng, name, W, n, a.reps)
                doc["shapes"].append(rec)
                print(json.dumps(rec), flush=True)
    doc["meets_requirement_everywhere"] = all(r["meets_requirement"] for r in doc["shapes"])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({"out": a.out, "meets_requirement_everywhere": doc["meets_requirement_everywhere"]}))


if __name__ == "__main__":
    main()
