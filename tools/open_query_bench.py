"""Open windows: what model 2's Jacobian rows from a carry record and the queries from a base row cost.  Needs a GPU.

  python tools/open_query_bench.py [--out profiles/open_query_bench.json] [--reps 21] [--queries 200000]

Timed with device events around each call after a warm-up, --reps times, the routes of a comparison ALTERNATING call by call on the
same box; median, minimum, maximum (microseconds).  Model 2, imu_avg 0, state_transition_jacobians 1, 10 k x 50 windows.
  resume   the windows in three segments (17 | 17 | 16 intervals), each a call that continues from the record of the one before.
           running_resume: cpi_preintegrate_running_resume with the means and P -- the entry as the parent commit has it (this commit
           leaves its kernels as they were: resource_usage_running_resume.txt is unchanged); running_resume_stj:
           cpi_running_resume_stj_batch with the means, all seven Jacobian fields and P.  A timed call is the three segments.
  query    Q queries (default 200 k) sorted by (window, time) over the last two segments (33 intervals), everything out.  closed:
           cpi_query_stj_batch on rows of cpi_running_stj_batch over those 33 intervals; open: cpi_query_open_batch on the same rows
           with the first segment's rows as base (in place, base_N = 17).  The same kernels bar the gather of i == 0; the outputs
           are NOT expected to be equal (the closed rows start from the zero state).
Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from query_cov_bench import alternating         # noqa: E402
from stj_bench import queries                   # noqa: E402

SEGS = ((0, 17), (17, 34), (34, 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_query_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--queries", type=int, default=200_000)
    a = ap.parse_args()
    import cpi_amd
    from cpi_amd import synth
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.reps >= 20, "20 or more repeats"
    eng = cpi_amd.Engine()
    W, N, Q = 10_000, 50, a.queries
    prm = eng.make_params(2)
    kn, lin, q = synth.make_windows(W, N, seed=2024, device=eng.device, edge_cases=False)
    segs = [kn[:, s:e + 1].contiguous() for s, e in SEGS]
    doc = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "W": W, "N": N,
           "model": 2, "segments": [e - s for s, e in SEGS]}

    cd = eng.carry_doubles(2)
    carries = [torch.empty((W, cd), dtype=torch.float64, device=eng.device) for _ in range(4)]
    rows_old = [eng.preintegrate_running_resume(k, lin, q, prm, want=("mean", "cov"))[0] for k in segs]
    rows_new = [eng.preintegrate_running_resume_stj(k, lin, q, prm, want=("mean", "jac", "cov"))[0] for k in segs]

    def chain(fn, rows, want, off):           # the records alternate between two buffers: carry_in and carry_out may not overlap
        cin = None
        for i, k in enumerate(segs):
            fn(k, lin, q, prm, want=want, carry_in=cin, carry_out=carries[off + i % 2], out=rows[i])
            cin = carries[off + i % 2]

    m = alternating({
        "running_resume_us": lambda: chain(eng.preintegrate_running_resume, rows_old, ("mean", "cov"), 0),
        "running_resume_stj_us": lambda: chain(eng.preintegrate_running_resume_stj, rows_new, ("mean", "jac", "cov"), 2),
    }, a.reps)
    m["readout_us"] = m["running_resume_stj_us"]["median"] - m["running_resume_us"]["median"]
    m["readout_share"] = m["readout_us"] / m["running_resume_us"]["median"]
    m["mean_and_P_rows_bit_equal"] = bool(all(torch.equal(rows_new[i][k], rows_old[i][k]) for i in range(3) for k in rows_old[i]))
    doc["resume"] = m
    print(json.dumps(m), flush=True)

    tail = kn[:, 17:].contiguous()
    closed_rows = eng.preintegrate_running_stj(tail, lin, q, prm, want=("mean", "jac", "cov"))
    qw, qt = queries(tail.cpu().numpy(), W, N - 17, Q)
    dqw, dqt = torch.from_numpy(qw).to(eng.device), torch.from_numpy(qt).to(eng.device)
    out_c = eng.alloc_outputs(Q, ("mean", "jac", "cov"), 2)
    out_o = eng.alloc_outputs(Q, ("mean", "jac", "cov"), 2)
    m = alternating({
        "closed_us": lambda: eng.query_stj(tail, lin, closed_rows, dqw, dqt, q_k_lin=q, params=prm, want=("mean", "jac", "cov"), out=out_c),
        "open_us": lambda: eng.query_open(tail, lin, closed_rows, dqw, dqt, rows_new[0], q_k_lin=q, params=prm, want=("mean", "jac", "cov"), out=out_o),
    }, a.reps)
    m["open_over_closed"] = m["open_us"]["median"] / m["closed_us"]["median"]
    m.update(Q=Q, order="sorted by (window, time)")
    doc["query"] = m
    print(json.dumps(doc), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
