"""The query by absolute time over one IMU stream: what cpi_query_stream_batch costs beside the only route without it.  Needs a GPU.

  python tools/query_stream_bench.py [--out profiles/query_stream_bench.json] [--reps 21] [--windows 10000] [--queries 200000]
  rocprofv3 --kernel-trace --stats -- python tools/query_stream_bench.py --route stream|assembled --model 1|2 --want mean|all

Workload: ONE stream cut into 10 k windows of 50 intervals with a tail (synth.make_stream, phase 0.37) and 200 k SORTED absolute
query times, uniform over the stream -- the sizes of profiles/query_cov_bench.md and profiles/stj_bench.md.  Models 1 and 2, imu_avg
0; want = means only, or everything out (means, Jacobians -- five for model 1, seven for model 2 --, P).
  stream      cpi_query_stream_batch on rows that are resident (the cut kernel, the window lookup and the query kernels; the rows come
              from cpi_stream_running_stj_batch, which is not part of the figure -- as the rows of query_stj are not part of its own).
  assembled   the route without the entry, its host part and its kernel part counted SEPARATELY: assemble_windows on the host, the
              upload of the copy, np.searchsorted for qwin and its upload (wall time, once), then cpi_query_stj_batch on rows computed
              from the assembled copy (kernel time).
Without --route: both routes in one process, the kernel parts timed with device events around each call after a warm-up, --reps
times, ALTERNATING call by call; median, minimum, maximum (microseconds), the host part in seconds, and the outputs of the two
routes compared bit for bit.  With --route: 20 calls of that route and nothing else, for a kernel trace.
Prints one JSON document (with the library's build id) and writes it to --out."""
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

from query_cov_bench import alternating         # noqa: E402

WANTS = {"mean": ("mean",), "all": ("mean", "jac", "cov")}


def workload(eng, U, N, Q):
    from cpi_amd import synth
    s, ut, lin, q = synth.make_stream(U, N, seed=2024, phase=0.37)
    t = s[:, 0]
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    qt = torch.sort(t[0] + torch.rand((Q,), generator=g, dtype=torch.float64) * (ut[-1] - t[0]))[0].contiguous()
    return s, ut, lin, q, qt


def assembled_route(eng, prm, s, ut, lin, q, qt, want):
    """The host part of the parent's route, timed step by step (seconds); returns the device arguments of cpi_query_stj_batch."""
    from cpi_amd import stream as st
    host = {}
    c0 = time.perf_counter()
    knots, first, count = st.assemble_windows(s.numpy(), ut.numpy())
    host["assemble_windows_s"] = time.perf_counter() - c0
    c0 = time.perf_counter()
    dk, df, dc = (torch.from_numpy(x).to(eng.device) for x in (knots, first, count))
    torch.cuda.synchronize()
    host["upload_s"] = time.perf_counter() - c0
    c0 = time.perf_counter()
    qwin = np.minimum(np.searchsorted(ut.numpy(), qt.numpy(), side="left"), len(ut) - 1).astype(np.int32)
    dqw = torch.from_numpy(qwin).to(eng.device)
    torch.cuda.synchronize()
    host["searchsorted_s"] = time.perf_counter() - c0
    host["copied_knot_bytes"] = int(knots.nbytes)
    N = int(count.max())
    dl, dq = lin.to(eng.device), q.to(eng.device)
    rows = eng.preintegrate_running_stj(dk, dl, dq, prm, want=want, first=df, count=dc, N=N)
    return host, dict(knots=dk, first=df, count=dc, lin=dl, q=dq, qwin=dqw, rows=rows, N=N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_stream_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--windows", type=int, default=10_000)
    ap.add_argument("--queries", type=int, default=200_000)
    ap.add_argument("--route", choices=("stream", "assembled"))
    ap.add_argument("--model", type=int, choices=(1, 2))
    ap.add_argument("--want", choices=tuple(WANTS))
    a = ap.parse_args()
    import cpi_amd
    assert torch.cuda.is_available(), "needs a GPU"
    eng = cpi_amd.Engine()
    U, N0, Q = a.windows, 50, a.queries
    s, ut, lin, q, qt = workload(eng, U, N0, Q)
    ds, du, dqt = s.to(eng.device), ut.to(eng.device), qt.to(eng.device)
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "U": U, "Q": Q,
           "order": "sorted by time", "cases": {}}
    for model in ((a.model,) if a.model else (1, 2)):
        prm = eng.make_params(model)
        host, A = assembled_route(eng, prm, s, ut, lin, q, qt, WANTS["all"])
        N = A["N"]
        ws = eng.stream_workspace(U)
        rows = eng.preintegrate_stream_running_stj(ds, du, A["lin"], q_k_lin=A["q"], params=prm, want=WANTS["all"], N=N, workspace=ws)
        for wname in ((a.want,) if a.want else tuple(WANTS)):
            want = WANTS[wname]
            out_s = eng.alloc_outputs(Q, want, model)
            out_a = eng.alloc_outputs(Q, want, model)
            new = lambda: eng.query_stream(ds, du, A["lin"], rows, dqt, q_k_lin=A["q"], params=prm, want=want, N=N, workspace=ws, out=out_s)
            old = lambda: eng.query_stj(A["knots"], A["lin"], A["rows"], A["qwin"], dqt, q_k_lin=A["q"], params=prm, want=want,
                                        first=A["first"], count=A["count"], N=N, out=out_a)
            if a.route:
                for _ in range(20):
                    (new if a.route == "stream" else old)()
                torch.cuda.synchronize()
                print("route %s model %d want %s: 20 calls done" % (a.route, model, wname))
                continue
            m = alternating({"query_stream_us": new, "query_stj_us": old}, a.reps)
            m["query_stream_over_query_stj"] = m["query_stream_us"]["median"] / m["query_stj_us"]["median"]
            m["host_part_of_the_assembled_route"] = host
            m["host_part_total_s"] = host["assemble_windows_s"] + host["upload_s"] + host["searchsorted_s"]
            _, qwin = new()
            torch.cuda.synchronize()
            m["qwin_equal"] = bool(torch.equal(qwin, A["qwin"]))
            m["bit_equal"] = bool(all(torch.equal(out_s[k].view(torch.int64), out_a[k].view(torch.int64)) for k in out_s))
            doc["cases"]["model%d_%s" % (model, wname)] = m
            print(json.dumps({"model": model, "want": wname, **m}), flush=True)
    if not a.route:
        print(json.dumps(doc), flush=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
