"""What cpi_chain_marginalize_batch costs, beside the detour a caller has without it and the solve of the same sub-chains.
Needs a GPU.

  python tools/chain_marginalize_bench.py [--out profiles/chain_marginalize.json] [--reps 11] [--shapes 50000x21:1,50000x21:10,50x549:1]

Per shape C x G : m -- the chains of tools/chain_solve_bench.py (its generators are imported: structured IMU-like factors, a prior on
every state; status 0 everywhere, asserted) with the leading m states of every chain eliminated.  Alternating call by call in one
process, each after 100 ms of untimed calls of its own, HIP events around the call(s):
  chain_marginalize  cpi_chain_marginalize_batch, M = m, drop = NULL
  solve_subchains    cpi_chain_solve_batch (lambda = NULL) on the eliminated sub-chains, count = m + 1 on the same arrays: the same
                     forward eliminations, plus the workspace stores and a back pass -- an upper bound
  detour             the route without the entry: that solve, cpi_chain_marginals_batch on its workspace, the cov row of state m
                     through cpi_sqrt_information_packed_batch, Lam = R^T R and eta = Lam delta_m in torch (four launches and the
                     torch operations; an inverse formed to be inverted again)
Reported: median / min / max in ms, microseconds per chain, the ratios, and the fraction of 8 TB/s on the bytes the entry must move
(496 + 136 doubles in per eliminated state, 136 out per chain).  The largest difference between the detour's Lam and the entry's,
relative to sqrt(Lam_ii Lam_jj), is reported with the detour.
One chain is worked on by 16 lanes; 50 x 549 fills 13 of 1024 SIMDs and shows the LATENCY of a chain, not throughput.
Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chain_solve_bench import PEAK, PRERAMP_MS, alternate, state_prior, structured_hess, tri_rc  # noqa: E402


def shape_run(eng, C, G, m, reps):
    import cpi_amd
    dev = eng.device
    S, F = C * G, C * (G - 1)
    hess = structured_hess(F, dev)
    prior = state_prior(C, G, dev)
    first = torch.arange(C, dtype=torch.int64, device=dev) * G
    ffirst = torch.arange(C, dtype=torch.int64, device=dev) * (G - 1)
    count = torch.full((C,), m + 1, dtype=torch.int32, device=dev)
    out = torch.empty((C, 136), dtype=torch.float64, device=dev)
    status = torch.empty((C,), dtype=torch.int32, device=dev)
    st2 = torch.empty((C,), dtype=torch.int32, device=dev)
    delta = torch.zeros((S, 15), dtype=torch.float64, device=dev)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    cov = torch.zeros((S, 120), dtype=torch.float64, device=dev)
    last = first + m

    marg = lambda: eng.chain_marginalize(hess, C=C, G=G, prior=prior, drop=m, out=out, status=status)
    solve = lambda: eng.chain_solve(hess, C=C, G=G, first=first, count=count, ffirst=ffirst, prior=prior, out=delta, status=st2, workspace=ws)

    def detour():
        solve()
        eng.chain_marginals(ws, C=C, G=G, first=first, count=count, status=st2, out=cov)
        R = cpi_amd.unpack_tri(eng.sqrt_information(cov[last].contiguous())).reshape(C, 15, 15)     # column-major: [col][row] = R^T
        Lam = R @ R.transpose(1, 2)
        return Lam, (Lam @ delta[last][:, :, None])[:, :, 0]

    marg()
    Lam_d, eta_d = detour()
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0 and int(st2.abs().max()) == 0 and bool(torch.isfinite(out).all()), "the bench's chains must solve"
    r, c = tri_rc(15, dev)
    d = torch.sqrt(torch.diagonal(Lam_d, dim1=1, dim2=2))
    e_lam = ((Lam_d[:, r, c] - out[:, :120]).abs() / (d[:, r] * d[:, c])).max().item()
    t = alternate({"chain_marginalize": marg, "solve_subchains": solve, "detour": detour}, reps)
    nbytes = 8 * ((496 + 136) * m + 136) * C
    for k in t:
        t[k]["us_per_chain"] = t[k]["median"] * 1e3 / C
    t["chain_marginalize"]["fraction_of_8TBps"] = nbytes / (t["chain_marginalize"]["median"] * 1e-3) / PEAK
    t["bytes"] = nbytes
    t["marginalize_over_solve_subchains"] = t["chain_marginalize"]["median"] / t["solve_subchains"]["median"]
    t["marginalize_over_detour"] = t["chain_marginalize"]["median"] / t["detour"]["median"]
    t["detour"]["max_diff_of_Lam_to_chain_marginalize_rel"] = float(e_lam)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_marginalize.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shapes", default="50000x21:1,50000x21:10,50x549:1")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import cpi_amd
    eng = cpi_amd.Engine()
    doc = {"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "reps": a.reps, "preramp_ms": PRERAMP_MS, "shapes": {}}
    for sh in a.shapes.split(","):
        cg, m = sh.split(":")
        C, G = (int(v) for v in cg.split("x"))
        doc["shapes"][sh] = shape_run(eng, C, G, int(m), a.reps)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
