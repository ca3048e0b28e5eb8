"""Model 2's bias Jacobians after every interval and at query times: what cpi_running_stj_batch and cpi_query_stj_batch cost.  Needs a GPU.

  python tools/stj_bench.py [--out profiles/stj_bench.json] [--reps 21] [--queries 200000]
  python tools/stj_bench.py --calls twin|stj      # a few calls WITHOUT a model-2 Jacobian request, for a kernel trace (see below)

Timed with device events around each call after a warm-up, --reps times, the routes of a comparison ALTERNATING call by call on the
same box; median, minimum, maximum (microseconds).  Model 2, imu_avg 0, state_transition_jacobians 1.
  read-out   W x 50 windows, W = 10 k and 100 k.  running: cpi_preintegrate_running with the means and P (what the parent commit
             offers); running_stj: cpi_running_stj_batch with the means, all seven Jacobian fields and P.  Both launch the mean kernel and
             ONE covariance kernel over the same recursion: the difference is the read-out after every interval (504 B per row more).
  query      Q queries (default 200 k) sorted by (window, time) over 10 k x 50 windows.  query_stj: cpi_query_stj_batch, everything out
             (means, seven Jacobians, P) from rows that hold everything; prefix_batch: the route without the entry -- ONE ragged
             cpi_preintegrate_batch, everything out, over Q windows assembled on the host, window k = [knot 0 .. knot i, {t_q, w_i,
             a_i}] (tools/query_bench.py: prefix_windows); its assembly and upload are reported separately and are NOT part of its
             kernel time.  query_cov: cpi_query_cov_batch with the means and P, for the share the Jacobians add.
--calls: runs three calls of the twins (cpi_preintegrate_running, cpi_query_cov_batch) or of the new entries on the same request
without a model-2 Jacobian field, models 1 and 2; under `rocprofv3 --kernel-trace --stats -- python tools/stj_bench.py --calls ...`
the two traces must list the same kernel names with the same counts.
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

from query_bench import prefix_windows          # noqa: E402
from query_cov_bench import alternating         # noqa: E402

JAC7 = ("J_q", "J_a", "J_b", "H_a", "H_b", "O_a", "O_b")


def queries(kn_h, W, N, Q, seed=7):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    qw = torch.randint(0, W, (Q,), generator=g, dtype=torch.int32).numpy()
    t0, t1 = kn_h[:, 0, 0], kn_h[:, N, 0]
    qt = t0[qw] + torch.rand((Q,), generator=g, dtype=torch.float64).numpy() * (t1 - t0)[qw]
    order = np.lexsort((qt, qw))
    return qw[order], qt[order]


def calls(eng, which):
    from cpi_amd import synth
    W, N, Q = 256, 50, 1024
    kn, lin, q = synth.make_windows(W, N, seed=5, device=eng.device, edge_cases=False)
    qw, qt = queries(kn.cpu().numpy(), W, N, Q)
    dqw, dqt = torch.from_numpy(qw).to(eng.device), torch.from_numpy(qt).to(eng.device)
    run = eng.preintegrate_running if which == "twin" else eng.preintegrate_running_stj
    qry = eng.query if which == "twin" else eng.query_stj
    for model in (1, 2):
        prm = eng.make_params(model)
        want = ("mean", "jac", "cov") if model == 1 else ("mean", "cov")
        for _ in range(3):
            rows = run(kn, lin, q, prm, want=want)
            qry(kn, lin, rows, dqw, dqt, q_k_lin=q, params=prm, want=want)
    torch.cuda.synchronize()
    print("calls %s done" % which)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stj_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--queries", type=int, default=200_000)
    ap.add_argument("--calls", choices=("twin", "stj"))
    a = ap.parse_args()
    import cpi_amd
    from cpi_amd import synth
    assert torch.cuda.is_available(), "needs a GPU"
    eng = cpi_amd.Engine()
    if a.calls:
        return calls(eng, a.calls)
    assert a.reps >= 20, "20 or more repeats"
    N, Q = 50, a.queries
    prm = eng.make_params(2)
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "N": N, "model": 2,
           "readout": {}, "query": {}}

    for W in (10_000, 100_000):
        kn, lin, q = synth.make_windows(W, N, seed=2024, device=eng.device, edge_cases=False)
        rows = eng.preintegrate_running_stj(kn, lin, q, prm, want=("mean", "jac", "cov"))
        base = {k: v for k, v in rows.items() if k not in JAC7}
        m = alternating({
            "running_us": lambda: eng.preintegrate_running(kn, lin, q, prm, want=("mean", "cov"), out=base),
            "running_stj_us": lambda: eng.preintegrate_running_stj(kn, lin, q, prm, want=("mean", "jac", "cov"), out=rows),
        }, a.reps)
        m["readout_us"] = m["running_stj_us"]["median"] - m["running_us"]["median"]
        m["readout_share"] = m["readout_us"] / m["running_us"]["median"]
        m["jacobian_bytes"] = W * N * 504
        fin = eng.preintegrate(kn, lin, q, prm, want=("jac",))
        m["last_row_bit_equal_to_batch"] = bool(all(torch.equal(rows[k][:, N - 1], fin[k]) for k in JAC7))
        m["last_row_largest_difference"] = float(max((rows[k][:, N - 1] - fin[k]).abs().max() for k in JAC7))
        doc["readout"]["%dx%d" % (W, N)] = m
        print(json.dumps({"W": W, **m}), flush=True)
        if W == 10_000:
            kn_h = kn.cpu().numpy()
            qw, qt = queries(kn_h, W, N, Q)
            dqw, dqt = torch.from_numpy(qw).to(eng.device), torch.from_numpy(qt).to(eng.device)
            c0 = time.perf_counter()
            pk, pf, pc = prefix_windows(kn_h, qw, qt)
            assembly = time.perf_counter() - c0
            dk, df, dc = (torch.from_numpy(x).to(eng.device) for x in (pk, pf, pc))
            dlin, dq = lin[dqw.long()].contiguous(), q[dqw.long()].contiguous()
            out = eng.alloc_outputs(Q, ("mean", "jac", "cov"), 2)
            cout = {k: v for k, v in out.items() if k not in JAC7}
            pout = eng.alloc_outputs(Q, ("mean", "jac", "cov"), 2)
            crows = {k: v for k, v in rows.items() if k not in JAC7}
            m = alternating({
                "query_stj_us": lambda: eng.query_stj(kn, lin, rows, dqw, dqt, q_k_lin=q, params=prm, want=("mean", "jac", "cov"), out=out),
                "query_cov_us": lambda: eng.query(kn, lin, crows, dqw, dqt, q_k_lin=q, params=prm, want=("mean", "cov"), out=cout),
                "prefix_batch_us": lambda: eng.preintegrate(dk, dlin, dq, prm, want=("mean", "jac", "cov"), first=df, count=dc, N=N + 1, out=pout),
            }, a.reps)
            m["prefix_batch_over_query_stj"] = m["prefix_batch_us"]["median"] / m["query_stj_us"]["median"]
            m["jacobians_us"] = m["query_stj_us"]["median"] - m["query_cov_us"]["median"]
            m["largest_jacobian_difference"] = float(max((out[k] - pout[k]).abs().max() for k in JAC7))
            m.update(W=W, Q=Q, order="sorted by (window, time)", prefix_assembly_s=assembly, prefix_knot_bytes=int(pk.nbytes))
            doc["query"] = m
            print(json.dumps(m), flush=True)
            del dk, df, dc, out, pout
        del rows, base, kn, lin, q
        torch.cuda.empty_cache()
    print(json.dumps(doc), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
