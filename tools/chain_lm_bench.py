"""What the Levenberg-Marquardt step per chain costs: cpi_prior_relinearize_batch, cpi_chain_cost_batch, cpi_chain_accept_batch, one whole
iteration of Engine.chain_lm eager and as a graph, beside the torch formulation of the same three steps.  Needs a GPU.

  python tools/chain_lm_bench.py [--out profiles/chain_lm.json] [--reps 11] [--shapes 50000x21,50x549] [--step-timeout 300]

Every shape runs in a child process of its own under --step-timeout; the parent stops at the first child that fails or runs out of time.
Per shape C x G -- C chains of G states back to back (the dense layout), real IMU factors (synth.make_windows, 10 intervals each), one
Gaussian prior per chain on its first state.  Alternating call by call in one process, each after 100 ms of untimed calls of its own, HIP
events around the call(s) (tools/chain_solve_bench.py: alternate):
  prior_relinearize   cpi_prior_relinearize_batch, C records, rows and pcost
  chain_cost          cpi_chain_cost_batch
  chain_accept_all    cpi_chain_accept_batch with every chain accepting (cost refilled with 1e300 inside the timed call: one fill
                      kernel of C doubles more): the trial's rows and chi2 are copied
  chain_accept_none   the same call with every chain rejecting: nothing is copied
  torch_prior         xi = eng.local_coordinates (3o's recipe), eta = eta0 + bmm(Lam, xi), the scatter into prior, pcost
  torch_cost          0.5 * chi2.view(C, G - 1).sum(1) + pcost.view(C, G).sum(1)
  torch_accept        new < cost, torch.where on states, chi2, cost and lambda (out of place, as 3l has it)
  factor_hessian, chain_solve     the two sweeps an iteration is made of, on the same box
  iteration_eager / iteration_graph   one iteration of Engine.chain_lm: issued eagerly / one captured graph replayed
The torch rows are the COMPARATOR for the dense layout (ragged chains have no view(C, G - 1)), not the code under test.
Reported: median / min / max in ms, the new entries' share of one eager iteration, the ratio to the torch comparator, and the fraction
of 8 TB/s on the bytes each kernel must move.  Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chain_solve_bench import PEAK, PRERAMP_MS, SCALES, alternate  # noqa: E402


def shape_run(eng, C, G, reps):
    from cpi_amd import synth
    dev = eng.device
    S, F = C * G, C * (G - 1)
    f64 = dict(dtype=torch.float64, device=dev)
    kn, lin, q = synth.make_windows(F, 10, device=dev, edge_cases=False)
    meas = eng.preintegrate(kn, lin, q, eng.make_params(1), want=("mean", "jac", "cov_sym"))
    Rt = eng.sqrt_information(meas["P_sym"])
    xi_, xj_ = synth.make_states(meas["alpha"], meas["beta"], meas["q"], meas["DT"], lin, 1, device=dev)
    states = torch.cat([xi_, xj_], dim=0)[:S].contiguous()
    m = {k: v for k, v in meas.items() if k != "P_sym"}
    ii, jj = (t.to(dev) for t in eng.chain_indices(C, G))
    pidx = (torch.arange(C, device=dev) * G).to(torch.int32)
    anchor = states[0::G].clone()
    anchor[:, 4:] += 1e-3 * torch.randn((C, 12), generator=torch.Generator(device=dev).manual_seed(3), **f64)
    lam0 = 0.1 * torch.tensor(SCALES, **f64) ** 2
    prior0 = torch.zeros((C, 136), **f64)
    prior0[:, [i * (i + 1) // 2 + i for i in range(15)]] = lam0
    Lam, eta0 = torch.diag(lam0).expand(C, 15, 15).contiguous(), prior0[:, 120:135].contiguous()

    bufs = {}
    run = lambda n, init: eng.chain_lm(1, m, lin, None, states, Rt, C, G, idx_i=ii, idx_j=jj, prior0=prior0, anchor=anchor, prior_idx=pidx,
                                       lam=1e-3, iterations=n, buffers=bufs, init=init)
    run(1, True)
    torch.cuda.synchronize()
    accepted = float(bufs["accepted"].double().mean().item())
    prior, pcost, chi2, chi2_new, trial = bufs["prior"], bufs["pcost"], bufs["chi2"], bufs["chi2_new"], bufs["trial"]
    cost, lam, phase = torch.zeros((C,), **f64), torch.ones((C,), **f64), torch.zeros((C,), dtype=torch.int32, device=dev)
    st2, c2 = states.clone(), chi2.clone()
    chi2_new.uniform_(1.0, 2.0)                                               # finite terms whatever the solve did: the kernels' time does not depend on them
    bufs["pcost_new"].zero_()

    def accept(cur):
        cost.fill_(cur)
        phase.zero_()
        eng.chain_accept(chi2_new, bufs["pcost_new"], trial, cost, st2, lam, phase, C=C, G=G, chi2=c2)

    def torch_prior():
        xi = eng.local_coordinates(states[0::G].contiguous(), anchor)
        eta = eta0 + torch.bmm(Lam, xi[:, :, None])[:, :, 0]
        prior[0::G, 120:135] = eta
        return 0.5 * (xi * (eta + eta0)).sum(1)

    def torch_accept():
        new = 0.5 * chi2_new.view(C, G - 1).sum(1)
        acc = new < cost
        return (torch.where(acc[:, None, None], trial.view(C, G, 16), st2.view(C, G, 16)), torch.where(acc[:, None], chi2_new.view(C, G - 1), c2.view(C, G - 1)),
                torch.where(acc, new, cost), torch.where(acc, lam * 0.1, lam * 10.0))

    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(1, False)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        run(1, False)
    hess, delta, status, ws = bufs["hess"], bufs["delta"], bufs["status"], bufs["workspace"]
    fns = {
        "prior_relinearize": lambda: eng.prior_relinearize(states, anchor, prior0, idx=pidx, out=prior, pcost=pcost),
        "chain_cost": lambda: eng.chain_cost(chi2, pcost, C=C, G=G, out=bufs["cost"]),
        "chain_accept_all": lambda: accept(1e300),
        "chain_accept_none": lambda: accept(-1e300),
        "torch_prior": torch_prior,
        "torch_cost": lambda: 0.5 * chi2.view(C, G - 1).sum(1) + pcost.view(C, G).sum(1),
        "torch_accept": torch_accept,
        "factor_hessian": lambda: eng.factor_hessian(1, m, lin, None, states, Rt, ii, jj, out=hess),
        "chain_solve": lambda: eng.chain_solve(hess, C=C, G=G, prior=prior, lam=bufs["lam"], damping="diagonal", out=delta, status=status, workspace=ws),
        "iteration_eager": lambda: run(1, False),
        "iteration_graph": graph.replay,
    }
    t = alternate(fns, reps)
    nbytes = {"prior_relinearize": 8 * C * (16 + 16 + 136 + 136 + 1), "chain_cost": 8 * (F + S + C),
              "chain_accept_all": 8 * (F + S + 2 * 16 * S + 2 * F + 3 * C) + 4 * 2 * C, "chain_accept_none": 8 * (F + S + 2 * C) + 4 * C}
    for k, b in nbytes.items():
        t[k]["bytes"] = b
        t[k]["fraction_of_8TBps"] = b / (t[k]["median"] * 1e-3) / PEAK
    it = t["iteration_eager"]["median"]
    for k in ("prior_relinearize", "chain_cost", "chain_accept_all", "factor_hessian", "chain_solve"):
        t[k]["share_of_eager_iteration"] = t[k]["median"] / it
    t["new_entries_share_of_eager_iteration"] = (2 * t["prior_relinearize"]["median"] + t["chain_accept_all"]["median"]) / it
    for mine, other in (("prior_relinearize", "torch_prior"), ("chain_cost", "torch_cost"), ("chain_accept_all", "torch_accept")):
        r = t[mine]["median"] / t[other]["median"]
        t[mine]["over_torch"] = r
        t[mine]["verdict"] = "faster than the torch comparator" if r < 1.0 else "NOT faster than the torch comparator"
    t["graph_over_eager"] = t["iteration_graph"]["median"] / it
    t["accepted_fraction_of_the_first_iteration"] = accepted
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_lm.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shapes", default="50000x21,50x549")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        assert torch.cuda.is_available(), "needs a GPU"
        import cpi_amd
        eng = cpi_amd.Engine()
        C, G = (int(v) for v in a.child.split("x"))
        print(json.dumps({"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "result": shape_run(eng, C, G, a.reps)}))
        return 0
    doc = {"reps": a.reps, "preramp_ms": PRERAMP_MS, "shapes": {}}
    for sh in a.shapes.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", sh, "--reps", str(a.reps)],
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("shape %s: the child ended with status %d; nothing more is started" % (sh, p.returncode), file=sys.stderr)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        doc["build_id"], doc["device"] = r["build_id"], r["device"]
        doc["shapes"][sh] = r["result"]
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
