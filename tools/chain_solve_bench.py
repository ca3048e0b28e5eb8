"""What cpi_chain_solve_batch costs, beside the Hessian sweep that feeds it and the dense route a caller would write without it.
Needs a GPU.

  python tools/chain_solve_bench.py [--out profiles/chain_solve.json] [--reps 11] [--shapes 50000x21,50x549] [--dense-max-gb 24]

Per shape C x G (C chains of G states, dense layout: first / count / ffirst NULL, a prior on every state, lambda [C] on
the device, identity damping).  The hess rows are structured IMU-like factors (tests/chain_cases.py's generator, batched in torch on
the device): symmetric positive definite chains, status 0 everywhere (asserted).  Variants, alternating call by call in one process,
each after 100 ms of untimed calls of its own (README, "clock under FP64 load"), HIP events around the call:
  chain_solve   cpi_chain_solve_batch
  hessian       cpi_factor_hessian_tri_batch on C (G - 1) factors with the chain's idx_i / idx_j (the sweep that writes hess; its
                inputs are synth.make_windows preintegrated on the device -- any valid factors: the sweep's time does not depend on them)
  dense         the route without the entry: scatter the hess rows and the prior into [C', 15 G, 15 G], torch.linalg.cholesky and
                torch.cholesky_solve -- on the C' <= C chains whose dense matrices fit --dense-max-gb (the time is reported per chain
                as well), matrices of at most 1024 rows; 3 repetitions.  When torch.linalg is unavailable in this torch build the row says so.
Reported: median / min / max in ms, per-chain and per-state microseconds, and the fraction of 8 TB/s on the algorithmic bytes of the
solve (per state: 496 hess + 136 prior + 2 x 360 workspace written and read back + 15 delta doubles).
One chain is worked on by 16 lanes; a shape of few long chains (50 x 549) fills 13 of 1024 SIMDs and shows the LATENCY of a chain,
not throughput.  Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK, PRERAMP_MS = 8e12, 100.0
DENSE_MAX_ROWS = 1024          # the dense route is timed up to 1024 rows per matrix: torch.linalg.cholesky fails to launch at 8 235 rows (50 x 549)
BYTES_PER_STATE = 8 * (496 + 136 + 2 * 360 + 15)
SCALES = [1e3] * 3 + [1e4] * 3 + [1e2] * 3 + [1e3] * 3 + [1e2] * 3


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
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            preramp(f)
            runs[k].append(timed_ms(f))
    return {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in runs.items()}


def tri_rc(n, dev):
    cols = torch.repeat_interleave(torch.arange(n, device=dev), torch.arange(1, n + 1, device=dev))
    rows = torch.arange(n * (n + 1) // 2, device=dev) - cols * (cols + 1) // 2
    return rows, cols


def structured_hess(F, dev, chunk=50_000):
    """[F, 496]: packed [A1 A2 b]^T [A1 A2 b], [A1 A2 b] = R [-Phi, I + E, r] (tests/chain_cases.py: _factor), in chunks."""
    g = torch.Generator(device=dev).manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64, device=dev)
    sc = torch.tensor(SCALES, dtype=torch.float64, device=dev)
    eye = torch.eye(15, dtype=torch.float64, device=dev)
    r, c = tri_rc(31, dev)
    out = torch.empty((F, 496), dtype=torch.float64, device=dev)
    for lo in range(0, F, chunk):
        n = min(chunk, F - lo)
        R = sc[None, :, None] * torch.triu(eye + 0.1 * rn(n, 15, 15))
        Phi = eye + 0.05 * rn(n, 15, 15)
        Phi[:, 12:15, 6:9] += 0.1 * torch.eye(3, dtype=torch.float64, device=dev)
        A = R @ torch.cat([-Phi, eye + 0.05 * rn(n, 15, 15), rn(n, 15, 1)], dim=2)
        out[lo:lo + n] = (A.transpose(1, 2) @ A)[:, r, c]
    return out


def state_prior(C, G, dev):
    """information 0.1 diag(scales)^2 on EVERY state: a chain of 549 states with a prior on its first state alone is too ill-conditioned to
    stay positive definite in float64, and the time of the solve does not depend on the values"""
    sc = torch.tensor(SCALES, dtype=torch.float64, device=dev)
    P = torch.zeros((C * G, 136), dtype=torch.float64, device=dev)
    i = torch.arange(15, device=dev)
    P[:, (i * (i + 1) // 2 + i)] = 0.1 * sc ** 2
    P[:, 120:135] = 0.1 * sc ** 2 * 0.01
    return P


def dense_system(hess, prior, lam, C, G):
    """(A [C, 15 G, 15 G], g [C, 15 G]) assembled by scatter-adds (tools/chain_marginals_bench.py inverts the same matrices)."""
    dev = hess.device
    n = 15 * G
    r, c = tri_rc(31, dev)
    H = torch.zeros((C * (G - 1), 31, 31), dtype=torch.float64, device=dev)
    H[:, r, c] = hess
    H[:, c, r] = hess
    H = H.reshape(C, G - 1, 31, 31)
    A = torch.zeros((C, n, n), dtype=torch.float64, device=dev)
    g = torch.zeros((C, n), dtype=torch.float64, device=dev)
    for k in range(G - 1):
        o = 15 * k
        A[:, o:o + 30, o:o + 30] += H[:, k, :30, :30]
        g[:, o:o + 30] += H[:, k, :30, 30]
    r16, c16 = tri_rc(16, dev)
    P = torch.zeros((C * G, 16, 16), dtype=torch.float64, device=dev)
    P[:, r16, c16] = prior
    P[:, c16, r16] = prior
    P = P.reshape(C, G, 16, 16)
    for s in range(G):
        o = 15 * s
        A[:, o:o + 15, o:o + 15] += P[:, s, :15, :15]
        g[:, o:o + 15] += P[:, s, :15, 15]
    i = torch.arange(n, device=dev)
    A[:, i, i] += lam[:, None]
    return A, g


def dense_route(hess, prior, lam, C, G):
    """The caller's route: [C, 15 G, 15 G] assembled by scatter-adds, Cholesky, two triangular solves."""
    A, g = dense_system(hess, prior, lam, C, G)
    L = torch.linalg.cholesky(A)
    return torch.cholesky_solve(g[:, :, None], L)[:, :, 0].reshape(C * G, 15)


def shape_run(eng, C, G, reps, dense_max_gb):
    from cpi_amd import synth
    dev = eng.device
    S, F = C * G, C * (G - 1)
    hess = structured_hess(F, dev)
    prior = state_prior(C, G, dev)
    lam = torch.full((C,), 1e-3, dtype=torch.float64, device=dev)
    delta = torch.empty((S, 15), dtype=torch.float64, device=dev)
    status = torch.empty((C,), dtype=torch.int32, device=dev)
    ws = torch.empty((eng.chain_solve_workspace_doubles(S),), dtype=torch.float64, device=dev)
    solve = lambda: eng.chain_solve(hess, C=C, G=G, prior=prior, lam=lam, out=delta, status=status, workspace=ws)
    solve()
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0 and bool(torch.isfinite(delta).all()), "the bench's chains must solve"
    # the sweep that feeds it
    kn, lin, q = synth.make_windows(F, 10, device=dev, edge_cases=False)
    meas = eng.preintegrate(kn, lin, q, eng.make_params(1), want=("mean", "jac", "cov_sym"))
    Rt = eng.sqrt_information(meas["P_sym"])
    xi, xj = synth.make_states(meas["alpha"], meas["beta"], meas["q"], meas["DT"], lin, 1, device=dev)
    states = torch.cat([xi, xj], dim=0)[:S].contiguous()
    ii, jj = (t.to(dev) for t in eng.chain_indices(C, G))
    m = {k: v for k, v in meas.items() if k != "P_sym"}
    hout = torch.empty((F, 496), dtype=torch.float64, device=dev)
    fns = {"chain_solve": solve, "hessian": lambda: eng.factor_hessian(1, m, lin, None, states, Rt, ii, jj, out=hout)}
    t = alternate(fns, reps)
    t["chain_solve"]["us_per_chain"] = t["chain_solve"]["median"] * 1e3 / C
    t["chain_solve"]["us_per_state"] = t["chain_solve"]["median"] * 1e3 / S
    t["chain_solve"]["fraction_of_8TBps"] = BYTES_PER_STATE * S / (t["chain_solve"]["median"] * 1e-3) / PEAK
    t["solve_over_hessian"] = t["chain_solve"]["median"] / t["hessian"]["median"]
    del kn, meas, Rt, states, hout
    torch.cuda.empty_cache()
    # the dense route, on as many chains as fit
    per_chain = 3 * 8 * (15 * G) ** 2                                        # A, L and the workspace of the factorisation
    Cd = int(min(C, max(1, dense_max_gb * 2 ** 30 // per_chain)))
    if not hasattr(torch, "linalg") or not hasattr(torch.linalg, "cholesky"):
        t["dense"] = {"note": "torch.linalg.cholesky is not available in this torch build"}
    elif 15 * G > DENSE_MAX_ROWS:
        t["dense"] = {"note": "not run: %d rows per matrix (the dense route is timed up to %d rows)" % (15 * G, DENSE_MAX_ROWS)}
    else:
        hd, pd, ld = hess[:Cd * (G - 1)], prior[:Cd * G], lam[:Cd]
        x = dense_route(hd, pd, ld, Cd, G)
        torch.cuda.synchronize()
        ref = delta[:Cd * G]
        d = alternate({"dense": lambda: dense_route(hd, pd, ld, Cd, G)}, 3)["dense"]
        d.update(chains=Cd, us_per_chain=d["median"] * 1e3 / Cd,
                 max_rel_diff_to_chain_solve=float(((x - ref).abs().max() / ref.abs().max()).item()))
        d["chain_solve_us_per_chain_over_dense"] = t["chain_solve"]["us_per_chain"] / d["us_per_chain"]
        t["dense"] = d
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_solve.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shapes", default="50000x21,50x549")
    ap.add_argument("--dense-max-gb", type=float, default=24.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import cpi_amd
    eng = cpi_amd.Engine()
    doc = {"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "reps": a.reps, "preramp_ms": PRERAMP_MS,
           "bytes_per_state": BYTES_PER_STATE, "shapes": {}}
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
