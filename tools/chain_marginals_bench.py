"""What cpi_chain_marginals_batch costs, beside the solve whose workspace it reads and the dense route a caller has without it.
Needs a GPU.

  python tools/chain_marginals_bench.py [--out profiles/chain_marginals.json] [--reps 11] [--shapes 50000x21,50x549] [--dense-max-gb 24]

Per shape C x G: the chains of tools/chain_solve_bench.py (its generators are imported: structured IMU-like factors, a prior on every
state, lambda [C] on the device, identity damping; status 0 everywhere, asserted).  cpi_chain_solve_batch runs once to leave the
workspace; then, alternating call by call in one process, each after 100 ms of untimed calls of its own, HIP events around the call:
  chain_marginals   cpi_chain_marginals_batch with cov and cross
  cov_only          the same call with cross = NULL
  chain_solve       cpi_chain_solve_batch on the same chains (the yardstick: the recursion has about the arithmetic of its forward
                    pass and a quarter of its traffic)
  dense             the route without the entry: scatter hess and prior into [C', 15 G, 15 G], torch.linalg.cholesky,
                    torch.cholesky_inverse, and the diagonal and first off-diagonal blocks sliced out -- on the C' <= C chains whose
                    matrices fit --dense-max-gb, matrices of at most 1024 rows; 3 repetitions
Reported: median / min / max in ms, per-chain and per-state microseconds, the ratio to the solve, and the fraction of 8 TB/s on the
algorithmic bytes of the call (per state: 360 workspace doubles read, 120 cov + 225 cross doubles written).  The largest difference to
the dense route's blocks, relative to the standard deviations, is reported with the dense row.
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

from chain_solve_bench import DENSE_MAX_ROWS, PEAK, PRERAMP_MS, alternate, dense_system, state_prior, structured_hess, tri_rc  # noqa: E402

BYTES_PER_STATE = 8 * (360 + 120 + 225)
BYTES_PER_STATE_COV_ONLY = 8 * (360 + 120)


def dense_route(hess, prior, lam, C, G):
    """The caller's route: the dense inverse of every chain's matrix -> (cov [C G, 15, 15], cross [C, G - 1, 15, 15])."""
    A, _ = dense_system(hess, prior, lam, C, G)
    Sig = torch.cholesky_inverse(torch.linalg.cholesky(A)).reshape(C, G, 15, G, 15)
    s = torch.arange(G, device=hess.device)
    cov = Sig[:, s, :, s, :].permute(1, 0, 2, 3).reshape(C * G, 15, 15)      # advanced indices first: [G, C, 15, 15]
    cross = Sig[:, s[:-1], :, s[1:], :].permute(1, 0, 2, 3)
    return cov.contiguous(), cross.contiguous()


def shape_run(eng, C, G, reps, dense_max_gb):
    dev = eng.device
    S, F = C * G, C * (G - 1)
    hess = structured_hess(F, dev)
    prior = state_prior(C, G, dev)
    lam = torch.full((C,), 1e-3, dtype=torch.float64, device=dev)
    delta = torch.empty((S, 15), dtype=torch.float64, device=dev)
    status = torch.empty((C,), dtype=torch.int32, device=dev)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    cov = torch.empty((S, 120), dtype=torch.float64, device=dev)
    cross = torch.zeros((S, 225), dtype=torch.float64, device=dev)
    solve = lambda: eng.chain_solve(hess, C=C, G=G, prior=prior, lam=lam, out=delta, status=status, workspace=ws)
    marg = lambda: eng.chain_marginals(ws, C=C, G=G, status=status, out=cov, cross=cross)
    solve()
    marg()
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0 and bool(torch.isfinite(cov).all()), "the bench's chains must solve"
    t = alternate({"chain_marginals": marg, "cov_only": lambda: eng.chain_marginals(ws, C=C, G=G, status=status, out=cov), "chain_solve": solve}, reps)
    for k, nbytes in (("chain_marginals", BYTES_PER_STATE), ("cov_only", BYTES_PER_STATE_COV_ONLY)):
        t[k]["us_per_chain"] = t[k]["median"] * 1e3 / C
        t[k]["us_per_state"] = t[k]["median"] * 1e3 / S
        t[k]["fraction_of_8TBps"] = nbytes * S / (t[k]["median"] * 1e-3) / PEAK
    t["marginals_over_solve"] = t["chain_marginals"]["median"] / t["chain_solve"]["median"]
    # the dense route, on as many chains as fit
    per_chain = 4 * 8 * (15 * G) ** 2                                        # A, L, the inverse and the workspace of the factorisation
    Cd = int(min(C, max(1, dense_max_gb * 2 ** 30 // per_chain)))
    if not hasattr(torch, "linalg") or not hasattr(torch.linalg, "cholesky"):
        t["dense"] = {"note": "torch.linalg.cholesky is not available in this torch build"}
    elif 15 * G > DENSE_MAX_ROWS:
        t["dense"] = {"note": "not run: %d rows per matrix (the dense route is timed up to %d rows)" % (15 * G, DENSE_MAX_ROWS)}
    else:
        hd, pd, ld = hess[:Cd * (G - 1)], prior[:Cd * G], lam[:Cd]
        dcov, dcross = dense_route(hd, pd, ld, Cd, G)
        torch.cuda.synchronize()
        r, c = tri_rc(15, dev)
        sd = torch.sqrt(torch.diagonal(dcov, dim1=1, dim2=2))
        e_cov = ((cov[:Cd * G] - dcov[:, r, c]).abs() / (sd[:, r] * sd[:, c])).max()
        mine = cross[:Cd * G].reshape(Cd, G, 15, 15).transpose(2, 3)[:, :-1]   # column-major rows -> [row][col]
        sdc = sd.reshape(Cd, G, 15)
        e_cross = ((mine - dcross).abs() / (sdc[:, :-1, :, None] * sdc[:, 1:, None, :])).max()
        d = alternate({"dense": lambda: dense_route(hd, pd, ld, Cd, G)}, 3)["dense"]
        d.update(chains=Cd, us_per_chain=d["median"] * 1e3 / Cd, max_diff_to_chain_marginals_in_sigmas=float(max(e_cov.item(), e_cross.item())))
        d["chain_marginals_us_per_chain_over_dense"] = t["chain_marginals"]["us_per_chain"] / d["us_per_chain"]
        t["dense"] = d
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_marginals.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shapes", default="50000x21,50x549")
    ap.add_argument("--dense-max-gb", type=float, default=24.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import cpi_amd
    eng = cpi_amd.Engine()
    doc = {"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "reps": a.reps, "preramp_ms": PRERAMP_MS,
           "bytes_per_state": BYTES_PER_STATE, "bytes_per_state_cov_only": BYTES_PER_STATE_COV_ONLY, "shapes": {}}
    for sh in a.shapes.split(","):
        C, G = (int(v) for v in sh.split("x"))
        doc["shapes"][sh] = shape_run(eng, C, G, a.reps, a.dense_max_gb)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
