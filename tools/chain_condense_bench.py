"""What segment condensation buys for long chains and costs for short ones: cpi_chain_solve_batch alone beside the three-call path
cpi_chain_condense_batch -> cpi_chain_solve_batch (reduced) -> cpi_chain_expand_batch.  Needs a GPU.

  python tools/chain_condense_bench.py [--out profiles/chain_condense.json] [--reps 11] [--shapes 50x549,50000x21] [--ks 8,12,16,23,32]

Per shape C x G -- the chains of tools/chain_solve_bench.py (its generators are imported: structured IMU-like factors, a prior on every
state, lambda = 1e-3; status 0 everywhere, asserted).  Alternating call by call in one process on one device, each after 100 ms of
untimed calls of its own, HIP events around the call(s):
  chain_solve        cpi_chain_solve_batch on the full chains (the kernel this path leaves untouched)
  segmented_K        Engine.chain_solve_segmented at segment length K with preallocated buffers: three launches, nothing allocated
  condense_K / reduced_solve_K / expand_K   the three calls of that path one by one: the per-kernel split (HIP events around one
                     launch each; their sum exceeds segmented_K by the event overhead of two more pairs)
Reported: median / min / max in ms, the ratio segmented_K / chain_solve, the best K per shape, and the largest difference between the
two deltas relative to the largest |delta| (the two paths must agree to rounding at the sizes that are timed).
Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chain_solve_bench import PRERAMP_MS, alternate, state_prior, structured_hess  # noqa: E402


def shape_run(eng, C, G, ks, reps):
    dev = eng.device
    S, F = C * G, C * (G - 1)
    hess = structured_hess(F, dev)
    prior = state_prior(C, G, dev)
    lam = torch.full((C,), 1e-3, dtype=torch.float64, device=dev)
    delta = torch.empty((S, 15), dtype=torch.float64, device=dev)
    status = torch.empty((C,), dtype=torch.int32, device=dev)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    fns = {"chain_solve": lambda: eng.chain_solve(hess, C=C, G=G, prior=prior, lam=lam, out=delta, status=status, workspace=ws)}
    fns["chain_solve"]()
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0 and bool(torch.isfinite(delta).all()), "the bench's chains must solve"
    scale = float(delta.abs().max())
    diffs = {}
    for K in ks:
        b = eng.chain_condense_buffers(C, G, S, K)
        out = torch.empty((S, 15), dtype=torch.float64, device=dev)
        Gr = eng.chain_condense_states(G, K)

        def seg(K=K, b=b, out=out):
            eng.chain_solve_segmented(hess, K, C=C, G=G, prior=prior, lam=lam, out=out, buffers=b)

        def condense(K=K, b=b):
            eng.chain_condense(hess, K, C=C, G=G, prior=prior, lam=lam, S=S, rhess=b["rhess"], rprior=b["rprior"], rcount=b["rcount"],
                               status=b["seg_status"], workspace=b["workspace"])

        def reduced(b=b, Gr=Gr):
            eng.chain_solve(b["rhess"], C=C, G=Gr, count=b["rcount"], prior=b["rprior"], out=b["rdelta"], status=b["status"], workspace=b["solve_workspace"])

        def expand(K=K, b=b, out=out):
            eng.chain_expand(b["rdelta"], b["workspace"], K, C=C, G=G, out=out)

        seg()
        torch.cuda.synchronize()
        assert int(b["status"].abs().max()) == 0 and int(b["seg_status"].abs().max()) == 0, "the segmented path must solve"
        diffs[K] = float((out - delta).abs().max()) / scale
        fns.update({"segmented_%d" % K: seg, "condense_%d" % K: condense, "reduced_solve_%d" % K: reduced, "expand_%d" % K: expand})
    t = alternate(fns, reps)
    for K in ks:
        t["segmented_%d" % K]["over_chain_solve"] = t["segmented_%d" % K]["median"] / t["chain_solve"]["median"]
        t["segmented_%d" % K]["max_diff_to_chain_solve_rel"] = diffs[K]
        t["segmented_%d" % K]["reduced_states"] = eng.chain_condense_states(G, K)
    t["best_K"] = min(ks, key=lambda K: t["segmented_%d" % K]["median"])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_condense.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shapes", default="50x549,50000x21")
    ap.add_argument("--ks", default="8,12,16,23,32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import cpi_amd
    eng = cpi_amd.Engine()
    ks = [int(v) for v in a.ks.split(",")]
    doc = {"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "reps": a.reps, "preramp_ms": PRERAMP_MS, "shapes": {}}
    for sh in a.shapes.split(","):
        C, G = (int(v) for v in sh.split("x"))
        doc["shapes"][sh] = shape_run(eng, C, G, ks, a.reps)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
