"""Resumable preintegration: what incremental use costs (cpi_preintegrate_resume).  Needs a GPU.

  python tools/resume_bench.py [--out profiles/resume_bench.json] [--reps 5]

(a) Per-read latency of the Python mirror (CpiV1) that reads the measurement after EVERY feed_IMU, for windows of
    n = 20, 200, 2000 intervals: re-run mode (the default: every read runs the whole window so far) against incremental
    mode (set_incremental: every read runs the one new interval from the carried state).  Host clock around reads that end
    in a device synchronise; mean over the window's reads.
(b) Device entry, 100 k windows x 50 intervals, models 1 and 2, everything out: one cpi_preintegrate_batch call against a
    chain of two cpi_preintegrate_resume calls of 25 intervals each (the second continuing from the first's carry record).
    Device events; the two variants alternate inside one process, median of --reps runs after a warm-up.
Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_read(eng, n, incremental, reads_cap=400):
    import cpi_amd
    from cpi_amd import synth
    kn, lin, q = synth.make_windows(1, n, seed=11, edge_cases=False)
    kn, lin, q = kn.numpy()[0], lin.numpy()[0], q.numpy()[0]
    cpi = cpi_amd.CpiV1(0.005, 4e-6, 0.01, 2e-4, engine=eng)
    if incremental:
        cpi.set_incremental(True)
    cpi.setLinearizationPoints(lin[:3], lin[3:], q, (0.0, 0.0, 9.8))
    times = []
    # every read is timed; for the re-run mode of long windows only the LAST reads_cap reads (the most expensive) are,
    # the earlier intervals are fed without a read in between
    first_timed = max(0, n - reads_cap) if not incremental else 0
    for i in range(n):
        a, b = kn[i], kn[i + 1]
        cpi.feed_IMU(a[0], b[0], a[1:4], a[4:7], b[1:4], b[4:7])
        if incremental or i >= first_timed:
            t0 = time.perf_counter()
            _ = cpi.P_meas   # the read runs the pending intervals and synchronises
            times.append(time.perf_counter() - t0)
    return {"n": n, "mode": "incremental" if incremental else "re-run", "reads_timed": len(times),
            "mean_us": 1e6 * float(np.mean(times)), "median_us": 1e6 * float(np.median(times)),
            "last_read_us": 1e6 * float(times[-1])}


def device_chain(eng, model, reps):
    from cpi_amd import synth
    W, N = 100_000, 50
    kn, lin, q = synth.make_windows(W, N, seed=404 + model, device=eng.device)
    prm = eng.make_params(model)
    out = eng.alloc_outputs(W, ("mean", "jac", "cov"), model)
    cd = eng.carry_doubles(model)
    ca = torch.empty((W, cd), dtype=torch.float64, device=eng.device)
    cb = torch.empty_like(ca)
    k1, k2 = kn[:, :26].contiguous(), kn[:, 25:].contiguous()

    def one():
        eng.preintegrate(kn, lin, q, prm, out=out)

    def chain():
        eng.preintegrate_resume(k1, lin, q, prm, out=out, carry_out=ca)
        eng.preintegrate_resume(k2, lin, q, prm, out=out, carry_in=ca, carry_out=cb)

    def timed(f):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        f()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for f in (one, chain, one, chain):
        timed(f)
    t_one, t_chain = [], []
    for _ in range(reps):
        t_one.append(timed(one))
        t_chain.append(timed(chain))
    m1, m2 = float(np.median(t_one)), float(np.median(t_chain))
    return {"model": model, "W": W, "N": N, "one_shot_ms": m1, "two_call_chain_ms": m2, "ratio": m2 / m1,
            "one_shot_runs_ms": t_one, "chain_runs_ms": t_chain,
            "carry_bytes_per_window": 8 * cd,
            "carry_GB_moved": 3 * W * 8 * cd / 1e9}   # written by call 1, read and written by call 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resume_bench measures the GPU: no device found"
    import cpi_amd
    eng = cpi_amd.Engine()
    lib = cpi_amd._lib.load()
    lib.cpi_build_id.restype = ctypes.c_char_p
    rec = {"build_id": lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(0),
           "per_read": [], "device_chain": []}
    for n in (20, 200, 2000):
        for inc in (False, True):
            rec["per_read"].append(per_read(eng, n, inc))
    for model in (1, 2):
        rec["device_chain"].append(device_chain(eng, model, args.reps))
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
