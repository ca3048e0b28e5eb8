"""Running preintegration from IMU stream(s), cut in place: what cpi_preintegrate_stream[s]_running costs beside the only route
to the same rows there was before.  Needs a GPU.

  python tools/stream_running_bench.py [--out profiles/stream_running_bench.json] [--reps 7] [--quick]

Per shape (R runs x U windows x N intervals) and request -- means only (model 1), model 1 everything (means + Jacobians + P),
model 2 means + P -- these are timed in one process, the device variants in alternation with device events around each:
  stream_running   (a) ONE cpi_preintegrate_stream_running / cpi_preintegrate_streams_running call on the resident stream(s)
  ragged_running   (b, device part) cpi_preintegrate_running on the host-assembled knots / first / count, already resident
  host_assembly    (b, host part) assemble_windows (cpi_amd/stream.py) on every run + the upload of the ragged copy: wall clock,
                   measured ONCE per shape (it is seconds long in Python; profiles/streams_bench.md has the C++ assembler's time)
  stream           (c) plain cpi_preintegrate_stream[s] on the same arguments: the final states only
  cut              the cut kernel alone (a stream call that asks for no output still owes the counts)
Median, minimum and maximum of --reps runs after a warm-up of each.  Prints one JSON document (with the library's build id) and
writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REQUESTS = {   # name -> (model, want of the running calls, want of the plain stream call)
    "mean_m1": (1, ("mean",), ("mean",)),
    "all_m1": (1, ("mean", "jac", "cov"), ("mean", "jac", "cov")),
    "mean_cov_m2": (2, ("mean", "cov"), ("mean", "cov")),
}
PHASE = 0.37    # every window but a run's first ends in a partial tail interval


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def make_shape(eng, R, U, N):
    """R runs of U windows x N intervals (N - 1 whole + the tail), every clock restarting at 0; the host-assembled ragged copy."""
    from cpi_amd import stream as st
    from cpi_amd import synth
    runs, lins, qs = [], [], []
    for r in range(R):
        s, u, lin, q = synth.make_stream(U, N - 1, seed=900 + r, phase=PHASE)
        t0 = s[0, 0].item()
        s[:, 0] -= t0
        u -= t0
        runs.append((s, u))
        lins.append(lin)
        qs.append(q)
    t = time.perf_counter()
    ks, fs, cs, base = [], [], [], 0
    for s, u in runs:
        k, f, c = st.assemble_windows(s.numpy(), u.numpy())
        ks.append(k); fs.append(f + base); cs.append(c)
        base += len(k)
    knots, first, count = np.concatenate(ks), np.concatenate(fs), np.concatenate(cs)
    dk, df, dc = (torch.from_numpy(a).to(eng.device) for a in (knots, first, count))
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t
    assert int(count.max()) == N
    d = lambda ts: torch.cat(ts).contiguous().to(eng.device)
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in runs])]).astype(np.int64)
    uo = np.concatenate([[0], np.cumsum([u.shape[0] for _, u in runs])]).astype(np.int64)
    return dict(R=R, stream=d([s for s, _ in runs]), ut=d([u for _, u in runs]), lin=d(lins), q=d(qs), knots=dk, first=df, count=dc,
                so=torch.from_numpy(so).to(eng.device), uo=torch.from_numpy(uo).to(eng.device), host_s=host_s,
                ragged_bytes=int(knots.nbytes + first.nbytes + count.nbytes))


def bench(eng, sh, name, N, reps):
    model, want, want_plain = REQUESTS[name]
    prm = eng.make_params(model)
    U = sh["ut"].shape[0]
    many = sh["R"] > 1
    ws = eng.streams_workspace(sh["R"], U)
    kw = dict(N=N, check_counts=False, workspace=ws)
    if many:
        a_call = lambda **k: eng.preintegrate_streams_running(sh["stream"], sh["so"], sh["ut"], sh["uo"], sh["lin"], sh["q"], prm, **kw, **k)
        c_call = lambda **k: eng.preintegrate_streams(sh["stream"], sh["so"], sh["ut"], sh["uo"], sh["lin"], sh["q"], prm, **kw, **k)
    else:
        a_call = lambda **k: eng.preintegrate_stream_running(sh["stream"], sh["ut"], sh["lin"], sh["q"], prm, **kw, **k)
        c_call = lambda **k: eng.preintegrate_stream(sh["stream"], sh["ut"], sh["lin"], sh["q"], prm, **kw, **k)
    rows_a = a_call(want=want)
    rows_b = eng.preintegrate_running(sh["knots"], sh["lin"], sh["q"], prm, want=want, first=sh["first"], count=sh["count"], N=N)
    torch.cuda.synchronize()
    identical = all(torch.equal(rows_a[k], rows_b[k]) for k in rows_b)
    fin = c_call(want=want_plain)
    fns = {
        "stream_running": lambda: a_call(want=want, out=rows_a),
        "ragged_running": lambda: eng.preintegrate_running(sh["knots"], sh["lin"], sh["q"], prm, want=want, first=sh["first"],
                                                           count=sh["count"], N=N, out=rows_b),
        "stream": lambda: c_call(want=want_plain, out=fin),
        "cut": lambda: c_call(want=(), out={}),
    }
    for fn in fns.values():         # warm-up of every variant, then alternate
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    rec = {"request": name, "model": model, "runs": sh["R"], "U": U, "N": N, "rows": U * N, "bit_identical_to_ragged_route": bool(identical),
           "host_assembly_and_upload_ms": 1e3 * sh["host_s"], "ragged_copy_bytes": sh["ragged_bytes"]}
    for k, v in ts.items():
        rec[k + "_us"] = {"median": 1e6 * float(np.median(v)), "min": 1e6 * float(np.min(v)), "max": 1e6 * float(np.max(v))}
    med = {k: float(np.median(v)) for k, v in ts.items()}
    rec["stream_running_over_ragged_running"] = med["stream_running"] / med["ragged_running"]
    rec["excess_over_ragged_minus_cut"] = (med["stream_running"] - med["cut"]) / med["ragged_running"]
    rec["stream_running_over_stream"] = med["stream_running"] / med["stream"]
    rec["old_route_total_over_stream_running"] = (sh["host_s"] + med["ragged_running"]) / med["stream_running"]
    del rows_a, rows_b, fin
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_running_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the multi-stream shape only")
    a = ap.parse_args()
    import cpi_amd
    assert torch.cuda.is_available(), "needs a GPU"
    eng = cpi_amd.Engine()
    shapes = [(50, 549, 20)] + ([] if a.quick else [(1, 27_450, 50), (1, 100_000, 20)])
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "phase": PHASE,
           "shapes": []}
    for R, U, N in shapes:
        sh = make_shape(eng, R, U, N)
        for name in REQUESTS:
            rec = bench(eng, sh, name, N, a.reps)
            doc["shapes"].append(rec)
            print(json.dumps(rec), flush=True)
        del sh
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
