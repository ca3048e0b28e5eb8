"""Joining consecutive windows: what cpi_merge_batch costs, beside the call it replaces.  Needs a GPU.

  python tools/merge_bench.py [--out profiles/merge_bench.json] [--reps 21] [--windows 200000] [--small-windows 10000]

Workload: W windows of 50 intervals (make_windows, default rate), each cut into 5 segments of 10 intervals that are preintegrated
one by one (model 1, imu_avg) into W * 5 measurement rows, window-major -- the camera-rate rows a caller holds.  Cases:
  full         W = 200 k: 1 M input rows, G = 5, everything out (means, Jacobians, P), P read and written dense
  full_packed  the same with the covariance as P_sym in and out
  mean         the same rows, the means alone (the kernel never touches P or the Jacobians)
  small_full   W = 10 k: 10 k x 50 split into 5 segments, everything out
Each case is timed against the call that merge replaces -- cpi_preintegrate_batch on the W joined windows of 50 intervals from the
raw IMU readings, same request -- with device events around each call after a warm-up, --reps times, the two ALTERNATING call by
call; median, minimum, maximum.  Bytes the merge moves: 2 248 B per operand row dense (88 means + 360 Jacobians + 1 800 P), 1 408 B
packed, 88 B for the means alone, plus one output row of the same size per group; reported with its fraction of 8 TB/s.
Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from query_cov_bench import alternating   # noqa: E402

SEG, G, PEAK = 10, 5, 8e12
ROW_BYTES = {"mean": 88, "jac": 360, "cov": 1800, "cov_sym": 960}


def operand_rows(eng, kn, lin, prm, want):
    """The W * G rows of the G segments of every window, window-major."""
    W = kn.shape[0]
    parts = [eng.preintegrate(kn[:, s * SEG:s * SEG + SEG + 1].contiguous(), lin, params=prm, want=want) for s in range(G)]
    rows = {}
    for k in parts[0]:
        a = torch.stack([p[k].reshape(W, -1) for p in parts], dim=1).reshape(W * G, -1)
        rows[k] = a.reshape(-1).contiguous() if k == "DT" else a.contiguous()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--windows", type=int, default=200_000)
    ap.add_argument("--small-windows", type=int, default=10_000)
    a = ap.parse_args()
    assert a.reps >= 20, "20 or more repeats"
    import cpi_amd
    from cpi_amd import synth
    eng = cpi_amd.Engine()
    prm = eng.make_params(1, True)
    doc = {"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "reps": a.reps, "G": G,
           "intervals_per_segment": SEG, "cases": {}}
    for size, W in (("", a.windows), ("small_", a.small_windows)):
        kn, lin, _ = synth.make_windows(W, SEG * G, device=eng.device, edge_cases=False)
        rows = operand_rows(eng, kn, lin, prm, ("mean", "jac", "cov", "cov_sym"))
        for name, want, keep in (("full", ("mean", "jac", "cov"), lambda k: k != "P_sym"),
                                 ("full_packed", ("mean", "jac", "cov_sym"), lambda k: k != "P"),
                                 ("mean", ("mean",), lambda k: k in ("DT", "alpha", "beta", "q"))):
            if size and name != "full":
                continue
            src = {k: v for k, v in rows.items() if keep(k)}
            out_m = eng.alloc_outputs(W, want)
            out_p = eng.alloc_outputs(W, want)
            t = alternating({"merge": lambda: eng.merge(src, G=G, want=want, out=out_m),
                             "reintegrate": lambda: eng.preintegrate(kn, lin, params=prm, want=want, out=out_p)}, a.reps)
            per_row = sum(ROW_BYTES[w] for w in want)
            moved = per_row * (W * G + W)
            med = t["merge"]["median"]
            doc["cases"][size + name] = {"input_rows": W * G, "groups": W, "want": list(want), "merge_us": t["merge"],
                                         "reintegrate_us": t["reintegrate"], "merge_over_reintegrate": med / t["reintegrate"]["median"],
                                         "merge_bytes": moved, "merge_fraction_of_8TBps": moved / (med * 1e-6) / PEAK}
        del rows, kn
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
