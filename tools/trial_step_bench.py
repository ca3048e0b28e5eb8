"""The optimiser's trial step: what cpi_factor_cost_tri_batch, cpi_retract_batch and cpi_local_batch cost.  Needs a GPU.

  python tools/trial_step_bench.py [--out profiles/trial_step.json] [--reps 21] [--factors 1000000] [--small-factors 10000]
                                   [--lanes 16,8,4]

Cost: F factors (factor_cases-free: synth.make_windows preintegrated on the device, make_states, R_tri = sqrt_information of P_sym),
states gathered through shuffled idx_i / idx_j, models 1 and 2, F = 1 M and 10 k.  Variants, alternating call by call in one
process, each after 100 ms of untimed calls of its own (README, "clock under FP64 load"), HIP events around the call(s):
  cost          cpi_factor_cost_tri_batch: chi2 + the total (two kernels; three above 32 768 factors)
  cost_werr     the same with werr out
  parent        the route without the entry: cpi_factor_eval_whitened_tri_batch with H1 = H2 = NULL, then (err * err).sum(1) and
                0.5 * chi2.sum() in torch
Reported: median / min / max in ms and the fraction of 8 TB/s on the algorithmic bytes per factor (1 720 model 1, 1 896 model 2:
88 means, 48 lin (+16 q_k_lin), 360 (+144) Jacobians, 256 states, 960 R_tri, 8 out).
Lanes per factor: --lanes runs the cost variant in child processes on libcpi_amd_exp.so (python -m cpi_amd.build --experiments) with
CPI_AMD_COST_LANES = 16 / 8 / 4 at both sizes, two rounds, alternating (medians of 7 in ms); skipped with a note when that library is not built.
Retract / local: 1 M states against torch's device copy of the same bytes (376 / 376 per state: 248 in + 128 out; 256 in + 120 out).
Prints one JSON document (with the library's build id) and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK, PRERAMP_MS = 8e12, 100.0
BYTES = {1: 1720, 2: 1896}


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


def factors(eng, model, F):
    """F factors on the device: measurement (preintegrated here), states gathered through shuffled indices, R_tri."""
    from cpi_amd import synth
    kn, lin, q = synth.make_windows(F, 10, device=eng.device, edge_cases=False)
    meas = eng.preintegrate(kn, lin, q, eng.make_params(model), want=("mean", "jac", "cov_sym"))
    Rt = eng.sqrt_information(meas["P_sym"])
    xi, xj = synth.make_states(meas["alpha"], meas["beta"], meas["q"], meas["DT"], lin, model, device=eng.device)
    st = torch.cat([xi, xj], dim=0)
    where = torch.randperm(2 * F, device=eng.device, generator=torch.Generator(device=eng.device).manual_seed(5))
    states = torch.empty_like(st)
    states[where] = st
    m = {k: v for k, v in meas.items() if k != "P_sym"}
    return dict(model=model, meas=m, lin=lin, q=(q if model == 2 else None), states=states.contiguous(), Rt=Rt,
                ii=where[:F].to(torch.int32).contiguous(), jj=where[F:].to(torch.int32).contiguous())


def cost_variants(eng, c, parent=True):
    a = (c["model"], c["meas"], c["lin"], c["q"], c["states"])
    F = c["lin"].shape[0]
    o1 = eng.factor_cost(*a, c["Rt"], c["ii"], c["jj"])
    o2 = eng.factor_cost(*a, c["Rt"], c["ii"], c["jj"], want_err=True)
    fns = {"cost": lambda: eng.factor_cost(*a, c["Rt"], c["ii"], c["jj"], out=o1),
           "cost_werr": lambda: eng.factor_cost(*a, c["Rt"], c["ii"], c["jj"], want_err=True, out=o2)}
    if parent:
        err = {"err": torch.empty((F, 15), dtype=torch.float64, device=eng.device)}

        def route():
            e = eng.factor_eval(*a, c["ii"], c["jj"], want_H=False, out=err, sqrt_info=c["Rt"])["err"]
            chi2 = (e * e).sum(1)
            return chi2, 0.5 * chi2.sum()
        fns["parent"] = route
    return fns


def child(model, F, reps):
    import cpi_amd
    eng = cpi_amd.Engine()
    c = factors(eng, model, F)
    fns = cost_variants(eng, c, parent=False)
    print(json.dumps(alternate({"cost": fns["cost"]}, reps)["cost"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trial_step.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--factors", type=int, default=1_000_000)
    ap.add_argument("--small-factors", type=int, default=10_000)
    ap.add_argument("--lanes", default="16,8,4")
    ap.add_argument("--child", nargs=2, type=int, metavar=("MODEL", "F"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.child:
        return child(a.child[0], a.child[1], a.reps)
    import cpi_amd
    from cpi_amd import build
    eng = cpi_amd.Engine()
    doc = {"build_id": eng.lib.cpi_build_id().decode(), "device": torch.cuda.get_device_name(), "reps": a.reps, "preramp_ms": PRERAMP_MS,
           "cost": {}, "lanes": {}, "states": {}}
    for F in (a.factors, a.small_factors):
        for model in (1, 2):
            c = factors(eng, model, F)
            t = alternate(cost_variants(eng, c), a.reps)
            for k in ("cost", "cost_werr"):
                t[k]["fraction_of_8TBps"] = (BYTES[model] + (120 if k == "cost_werr" else 0)) * F / (t[k]["median"] * 1e-3) / PEAK
            t["cost_over_parent"] = t["cost"]["median"] / t["parent"]["median"]
            doc["cost"]["F%d_model%d" % (F, model)] = t
            del c
            torch.cuda.empty_cache()
    # retract / local against a plain device copy of the same bytes
    S = a.factors
    g = torch.Generator(device=eng.device).manual_seed(6)
    q = torch.randn((S, 4), dtype=torch.float64, device=eng.device, generator=g)
    x = torch.cat([q / q.norm(dim=1, keepdim=True), torch.randn((S, 12), dtype=torch.float64, device=eng.device, generator=g)], dim=1).contiguous()
    d = (0.1 * torch.randn((S, 15), dtype=torch.float64, device=eng.device, generator=g)).contiguous()
    other = eng.retract(x, d)
    out_r, out_l = torch.empty_like(x), torch.empty((S, 15), dtype=torch.float64, device=eng.device)
    src, dst = torch.empty((S * 47 // 2,), dtype=torch.float64, device=eng.device), torch.empty((S * 47 // 2,), dtype=torch.float64, device=eng.device)
    t = alternate({"retract": lambda: eng.retract(x, d, out=out_r), "retract_in_place": lambda: eng.retract(other, d, out=other),
                   "local": lambda: eng.local_coordinates(x, other, out=out_l), "copy_same_bytes": lambda: dst.copy_(src)}, a.reps)
    for k in t:
        t[k]["fraction_of_8TBps"] = 376.0 * S / (t[k]["median"] * 1e-3) / PEAK
    doc["states"]["S%d" % S] = t
    # lanes per factor: children on the experiments library
    lanes = [int(v) for v in a.lanes.split(",") if v]
    if lanes and os.path.exists(build.LIB_EXP):
        for F in (a.factors, a.small_factors):
            for model in (1, 2):
                runs = {L: [] for L in lanes}
                for _ in range(2):
                    for L in lanes:
                        env = dict(os.environ, CPI_AMD_LIB=build.LIB_EXP, CPI_AMD_COST_LANES=str(L))
                        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(model), str(F), "--reps", "7"],
                                           env=env, stdout=subprocess.PIPE, text=True, timeout=300, check=True)
                        runs[L].append(json.loads(p.stdout.strip().splitlines()[-1])["median"])
                doc["lanes"]["F%d_model%d" % (F, model)] = {str(L): v for L, v in runs.items()}
    else:
        doc["lanes"]["note"] = "libcpi_amd_exp.so is not built (python -m cpi_amd.build --experiments): no lanes-per-factor A/B"
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
