"""Many trajectories at once (cpi_preintegrate_streams) against the ways a caller could preintegrate them before.  Needs a GPU.

  python tools/streams_bench.py [--out-dir profiles] [--reps 7]

The reference's Monte-Carlo evaluation replays 50 datasets per IMU rate (run_mc.sh), ~549 windows each.  Here: 50 synthetic
runs from synth.make_stream, one seed per run, 200 Hz IMU, 10 Hz updates (20 samples per window, updates off the IMU grid),
549 windows per run -- every run starts at the same stamp, so the stamps go backwards at every run boundary.  Timed, for
model 1 mean-only, v1_full and v2_full (means + Jacobians + covariance):
  streams      ONE cpi_preintegrate_streams call
  per_run      50 back-to-back cpi_preintegrate_stream calls on one context (ctypes, arguments prepared beforehand)
  ragged       cpi_preintegrate_batch on the windows the host assembler (cpi_amd/stream.py) cut out of every run: the device
               call alone, and with the assembly + upload (host clock) in front of it
and R = 1 against cpi_preintegrate_stream on 1 M windows x 50 samples, mean-only: what the run lookup costs.
Device times are HIP events around the call(s); before every measurement 100 ms of untimed calls ramp the clock up (as
bench.py does for its extra rows); the variants alternate inside one process and the medians of --reps runs are reported.
Writes <out-dir>/streams_bench.json and streams_bench.md, stamped with build.source_id()."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (("v1_mean", 1, ("mean",)), ("v1_full", 1, ("mean", "jac", "cov")), ("v2_full", 2, ("mean", "jac", "cov")))
PRERAMP_MS = 100.0


def timed_ms(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    f()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def preramp(f):
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < PRERAMP_MS:
        f()
        torch.cuda.synchronize()


def alternate(fns, reps):
    """{name: median ms} of the callables, run alternately, each after its own pre-ramp."""
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            preramp(f)
            runs[k].append(timed_ms(f))
    return {k: float(np.median(v)) for k, v in runs.items()}, runs


def fifty_runs(eng, R, windows, n):
    from cpi_amd import synth
    runs = [synth.make_stream(windows, n, seed=1000 + r, rate=200.0, device=eng.device, phase=0.37) for r in range(R)]
    return runs


def bench_runs(eng, reps, R=50, windows=549, n=20):
    from cpi_amd import stream as st
    lib = eng.lib
    runs = fifty_runs(eng, R, windows, n)
    stream = torch.cat([s for s, _, _, _ in runs]).contiguous()
    ut = torch.cat([u for _, u, _, _ in runs]).contiguous()
    lin = torch.cat([l for _, _, l, _ in runs]).contiguous()
    q = torch.cat([qq for _, _, _, qq in runs]).contiguous()
    so = torch.tensor(np.concatenate([[0], np.cumsum([s.shape[0] for s, _, _, _ in runs])]), dtype=torch.int64, device=eng.device)
    uo = torch.tensor(np.concatenate([[0], np.cumsum([u.shape[0] for _, u, _, _ in runs])]), dtype=torch.int64, device=eng.device)
    U, K = ut.shape[0], stream.shape[0]
    N = eng.streams_bound(stream, so, ut, uo)
    host_runs = [(s.cpu().numpy(), u.cpu().numpy()) for s, u, _, _ in runs]
    rows = []
    for name, model, want in CONFIGS:
        prm = eng.make_params(model)
        out = eng.alloc_outputs(U, want, model)
        ws = eng.streams_workspace(R, U)
        P = lambda t: C.c_void_p(t.data_ptr())
        # per-run calls: outputs are row slices of the same arrays, arguments prepared once
        per = []
        for r, (s, u, _, _) in enumerate(runs):
            a, b = int(uo[r]), int(uo[r + 1])
            o = eng._outputs_struct({k: v[a:b] for k, v in out.items()})
            w1 = eng.stream_workspace(b - a)
            per.append((o, w1, (eng.ctx, C.byref(prm), s.shape[0], P(s), b - a, P(u), N, P(lin[a:b]), P(q[a:b]) if model == 2 else None,
                                P(w1))))

        def f_streams():
            eng.preintegrate_streams(stream, so, ut, uo, lin, q if model == 2 else None, prm, want=want, N=N, out=out,
                                     check_counts=False, workspace=ws)

        def f_per_run():
            for o, _, args in per:
                lib.cpi_preintegrate_stream(*args, C.byref(o))

        # the host-assembled ragged batch
        t0 = time.perf_counter()
        parts = [st.assemble_windows(s, u) for s, u in host_runs]
        base = np.concatenate([[0], np.cumsum([len(k) for k, _, _ in parts])])
        knots = torch.from_numpy(np.concatenate([k for k, _, _ in parts])).to(eng.device)
        first = torch.from_numpy(np.concatenate([f + base[i] for i, (_, f, _) in enumerate(parts)])).to(eng.device)
        count = torch.from_numpy(np.concatenate([c for _, _, c in parts])).to(eng.device)
        torch.cuda.synchronize()
        assembly_ms = 1e3 * (time.perf_counter() - t0)

        def f_ragged():
            eng.preintegrate(knots, lin, q if model == 2 else None, prm, want=want, first=first, count=count, N=N, out=out)

        med, all_runs = alternate({"streams": f_streams, "per_run": f_per_run, "ragged": f_ragged}, reps)
        rows.append({"config": name, "model": model, "want": list(want), "runs": R, "windows": U, "knots": K, "N": N,
                     "streams_ms": med["streams"], "per_run_ms": med["per_run"], "ragged_batch_ms": med["ragged"],
                     "ragged_assembly_ms": assembly_ms, "ragged_with_assembly_ms": med["ragged"] + assembly_ms,
                     "per_run_over_streams": med["per_run"] / med["streams"], "runs_ms": all_runs})
    return rows


def bench_r1(eng, reps, W=1_000_000, n=50):
    from cpi_amd import synth
    s, u, lin, _ = synth.make_stream(W, n, seed=2024, device=eng.device, phase=0.37)
    prm = eng.make_params(1)
    out = eng.alloc_outputs(W, ("mean",), 1)
    ws1, wsr = eng.stream_workspace(W), eng.streams_workspace(1, W)
    so = torch.tensor([0, s.shape[0]], dtype=torch.int64, device=eng.device)
    uo = torch.tensor([0, W], dtype=torch.int64, device=eng.device)
    N = n + 1

    def f_stream():
        eng.preintegrate_stream(s, u, lin, None, prm, want=("mean",), N=N, out=out, check_counts=False, workspace=ws1)

    def f_streams():
        eng.preintegrate_streams(s, so, u, uo, lin, None, prm, want=("mean",), N=N, out=out, check_counts=False, workspace=wsr)

    med, all_runs = alternate({"stream": f_stream, "streams_r1": f_streams}, reps)
    return {"windows": W, "samples_per_window": n, "N": N, "stream_ms": med["stream"], "streams_r1_ms": med["streams_r1"],
            "ratio": med["streams_r1"] / med["stream"], "runs_ms": all_runs}


def write_md(rec, path):
    L = ["# Many trajectories in one call (cpi_preintegrate_streams)", "",
         "tools/streams_bench.py; library source id `%s`, build `%s`, %s.  Medians of %d alternating runs, each after a 100 ms "
         "pre-ramp; device times from HIP events." % (rec["source_id"], rec["build_id"], rec["device"], rec["reps"]), "",
         "## 50 runs x 549 windows (200 Hz IMU, 10 Hz updates, 20 samples per window)", "",
         "| config | one streams call (ms) | 50 stream calls (ms) | ragged batch (ms) | ragged + host assembly (ms) | 50 calls / one call |",
         "|---|---|---|---|---|---|"]
    for r in rec["fifty_runs"]:
        L.append("| %s | %.3f | %.3f | %.3f | %.1f | %.2f x |" % (r["config"], r["streams_ms"], r["per_run_ms"], r["ragged_batch_ms"],
                                                              r["ragged_with_assembly_ms"], r["per_run_over_streams"]))
    r1 = rec["r1"]
    L += ["", "## R = 1 against cpi_preintegrate_stream (1 M windows x 50 samples, model 1 mean-only)", "",
          "| cpi_preintegrate_stream (ms) | cpi_preintegrate_streams, R = 1 (ms) | ratio |", "|---|---|---|",
          "| %.3f | %.3f | %.3f |" % (r1["stream_ms"], r1["streams_r1_ms"], r1["ratio"]), ""]
    sp = [r["per_run_over_streams"] for r in rec["fifty_runs"]]
    L += ["## Result", "",
          "One multi-run call is %.1f-%.1f x %s than 50 back-to-back single-stream calls on one context; the host-assembled ragged "
          "batch needs %.0f-%.0f ms of assembly in front of its kernels.  At R = 1 the run lookup costs %+.1f %% against "
          "cpi_preintegrate_stream (1 M x 50, mean-only)." % (min(sp), max(sp), "faster" if min(sp) > 1 else "slower or equal",
                                                              min(r["ragged_assembly_ms"] for r in rec["fifty_runs"]),
                                                              max(r["ragged_assembly_ms"] for r in rec["fifty_runs"]),
                                                              100 * (r1["ratio"] - 1)), ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "streams_bench measures the GPU: no device found"
    import cpi_amd
    from cpi_amd import build
    eng = cpi_amd.Engine()
    lib = cpi_amd._lib.load()
    lib.cpi_build_id.restype = C.c_char_p
    rec = {"source_id": build.source_id(), "build_id": lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "preramp_ms": PRERAMP_MS}
    rec["fifty_runs"] = bench_runs(eng, args.reps)
    rec["r1"] = bench_r1(eng, args.reps)
    print(json.dumps({k: v for k, v in rec.items()}, indent=1))
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "streams_bench.json"), "w") as f:
        json.dump(rec, f, indent=1)
    write_md(rec, os.path.join(args.out_dir, "streams_bench.md"))


if __name__ == "__main__":
    if "--md-from" in sys.argv:   # re-render the table of a saved record
        i = sys.argv.index("--md-from")
        write_md(json.load(open(sys.argv[i + 1])), sys.argv[i + 2])
    else:
        main()
