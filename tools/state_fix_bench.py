"""What cpi_state_fix_batch costs: one position fix per state as rows plus cost, as cost only, and the pose kind, beside the torch
formulation of the same results and beside chain_solve on the same chains.  Needs a GPU.

  python tools/state_fix_bench.py [--out profiles/state_fix.json] [--reps 11] [--shapes 50000x21] [--step-timeout 300]

Every shape runs in a child process of its own under --step-timeout; the parent stops at the first child that fails or runs out of time.
Per shape C x G -- C chains of G states back to back, real IMU factors (synth.make_windows, 10 intervals each), one Gaussian prior per
chain on its first state, ONE fix on every state (M = S), the base row of every state the relinearised prior's.  Alternating call by
call in one process, each after 100 ms of untimed calls of its own, HIP events around the call(s) (tools/chain_solve_bench.py: alternate):
  fix_rows_cost       cpi_state_fix_batch, position, rows on a base and pcost
  fix_cost            the same call with out = NULL: pcost alone (the two cost evaluations of an iteration)
  fix_pose            the pose kind, rows and pcost
  fix_sparse_rows     the position call on a base of S / G rows only (what a sparse form would move: a lower bound for one, not an entry)
  torch_rows_cost     e = z - p, R dense from the packed triangle, G = bmm(R^T, R), rows = base.clone() with index_add_ of the six entries
                      and the three of eta, pcost = 0.5 |R e|^2 (one fix per state: the bincount is the identity)
  torch_cost          the last line alone
  chain_solve, factor_hessian     the two sweeps an iteration is made of, on the same box
  iteration_eager / iteration_fixes_eager   one iteration of Engine.chain_lm without / with the position fixes
The torch rows are the COMPARATOR, not the code under test.  Reported: median / min / max in ms, each form's ratio to its torch
comparator and to chain_solve, its share of an eager iteration, and the fraction of 8 TB/s on the bytes the kernel must move.  Prints one
JSON document (with the library's build id) and writes it to --out."""
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
    gen = torch.Generator(device=dev).manual_seed(3)
    kn, lin, q = synth.make_windows(F, 10, device=dev, edge_cases=False)
    meas = eng.preintegrate(kn, lin, q, eng.make_params(1), want=("mean", "jac", "cov_sym"))
    Rt = eng.sqrt_information(meas["P_sym"])
    xi_, xj_ = synth.make_states(meas["alpha"], meas["beta"], meas["q"], meas["DT"], lin, 1, device=dev)
    states = torch.cat([xi_, xj_], dim=0)[:S].contiguous()
    m = {k: v for k, v in meas.items() if k != "P_sym"}
    ii, jj = (t.to(dev) for t in eng.chain_indices(C, G))
    pidx = (torch.arange(C, device=dev) * G).to(torch.int32)
    anchor = states[0::G].clone()
    anchor[:, 4:] += 1e-3 * torch.randn((C, 12), generator=gen, **f64)
    prior0 = torch.zeros((C, 136), **f64)
    prior0[:, [i * (i + 1) // 2 + i for i in range(15)]] = 0.1 * torch.tensor(SCALES, **f64) ** 2

    mfirst = torch.arange(S + 1, dtype=torch.int64, device=dev)
    z = (states[:, 13:16] + 0.05 * torch.randn((S, 3), generator=gen, **f64)).contiguous()
    Rp = torch.zeros((S, 6), **f64)
    Rp[:, [0, 2, 5]] = 20.0
    Rp[:, 1] = 1.0
    zq = torch.cat([states[:, 0:4], z], dim=1).contiguous()
    Rq = torch.zeros((S, 21), **f64)
    Rq[:, [a * (a + 1) // 2 + a for a in range(6)]] = torch.tensor([100.0] * 3 + [50.0] * 3, **f64)
    fixes = [dict(kind="position", z=z, R=Rp, mfirst=mfirst)]

    bufs, bufs_f = {}, {}
    common = dict(idx_i=ii, idx_j=jj, prior0=prior0, anchor=anchor, prior_idx=pidx, lam=1e-3)
    run = lambda n, init: eng.chain_lm(1, m, lin, None, states, Rt, C, G, iterations=n, buffers=bufs, init=init, **common)
    run_f = lambda n, init: eng.chain_lm(1, m, lin, None, states, Rt, C, G, iterations=n, buffers=bufs_f, init=init, fixes=fixes, **common)
    st0 = states.clone()
    run(1, True)
    states.copy_(st0)
    run_f(1, True)
    states.copy_(st0)
    torch.cuda.synchronize()
    base, pbase = bufs["prior"], bufs["pcost"]
    out, pcost = torch.zeros((S, 136), **f64), torch.zeros((S,), **f64)
    few = S // G
    mfew = torch.arange(few + 1, dtype=torch.int64, device=dev)
    out_few, base_few, st_few = out[:few], base[:few].contiguous(), states[:few].contiguous()
    tri_r, tri_c = torch.tensor([0, 0, 1, 0, 1, 2], device=dev), torch.tensor([0, 1, 1, 2, 2, 2], device=dev)   # the packed order: column by column
    slot = lambda a, b: b * (b + 1) // 2 + a
    lam_slots = torch.tensor([slot(12 + int(a), 12 + int(b)) for a, b in zip(tri_r, tri_c)], device=dev)
    eta_slots = torch.tensor([slot(12 + a, 15) for a in range(3)], device=dev)

    def torch_cost():
        Rd = torch.zeros((S, 3, 3), **f64)
        Rd[:, tri_r, tri_c] = Rp
        e = z - states[:, 13:16]
        wh = torch.bmm(Rd, e[:, :, None])
        return Rd, wh, 0.5 * (wh * wh).sum((1, 2)) + pbase

    def torch_rows_cost():
        Rd, wh, pc = torch_cost()
        Gm = torch.bmm(Rd.transpose(1, 2), Rd)
        u = torch.bmm(Rd.transpose(1, 2), wh)[:, :, 0]
        rows = base.clone()
        rows.index_add_(1, lam_slots, Gm[:, tri_r, tri_c])
        rows.index_add_(1, eta_slots, u)
        return rows, pc

    hess, delta, status, ws = bufs["hess"], bufs["delta"], bufs["status"], bufs["workspace"]
    fns = {
        "fix_rows_cost": lambda: eng.state_fix(states, "position", z, Rp, mfirst, base=base, pcost_base=pbase, out=out, pcost=pcost),
        "fix_cost": lambda: eng.state_fix(states, "position", z, Rp, mfirst, pcost_base=pbase, pcost=pcost, want_rows=False),
        "fix_pose": lambda: eng.state_fix(states, "pose", zq, Rq, mfirst, base=base, pcost_base=pbase, out=out, pcost=pcost),
        "fix_sparse_rows": lambda: eng.state_fix(st_few, "position", z[:few], Rp[:few], mfew, base=base_few, out=out_few, want_cost=False),
        "torch_rows_cost": torch_rows_cost,
        "torch_cost": lambda: torch_cost()[2],
        "factor_hessian": lambda: eng.factor_hessian(1, m, lin, None, states, Rt, ii, jj, out=hess),
        "chain_solve": lambda: eng.chain_solve(hess, C=C, G=G, prior=base, lam=bufs["lam"], damping="diagonal", out=delta, status=status, workspace=ws),
        "iteration_eager": lambda: run(1, False),
        "iteration_fixes_eager": lambda: run_f(1, False),
    }
    t = alternate(fns, reps)
    nbytes = {"fix_rows_cost": 8 * S * (2 * 136 + 16 + 3 + 6 + 2 + 1), "fix_cost": 8 * S * (16 + 3 + 6 + 2 + 1), "fix_pose": 8 * S * (2 * 136 + 16 + 7 + 21 + 2 + 1),
              "fix_sparse_rows": 8 * few * (2 * 136 + 16 + 3 + 6 + 1)}
    for k, b in nbytes.items():
        t[k]["bytes"] = b
        t[k]["fraction_of_8TBps"] = b / (t[k]["median"] * 1e-3) / PEAK
    it = t["iteration_fixes_eager"]["median"]
    for k in ("fix_rows_cost", "fix_cost", "fix_pose", "fix_sparse_rows"):
        t[k]["over_chain_solve"] = t[k]["median"] / t["chain_solve"]["median"]
        t[k]["share_of_eager_iteration_with_fixes"] = t[k]["median"] / it
    t["fixes_share_of_eager_iteration"] = (t["fix_rows_cost"]["median"] + t["fix_cost"]["median"]) / it
    t["iteration_with_fixes_over_without"] = it / t["iteration_eager"]["median"]
    for mine, other in (("fix_rows_cost", "torch_rows_cost"), ("fix_cost", "torch_cost"), ("fix_pose", "torch_rows_cost")):
        r = t[mine]["median"] / t[other]["median"]
        t[mine]["over_torch"] = r
        t[mine]["verdict"] = "faster than the torch comparator" if r < 1.0 else "NOT faster than the torch comparator"
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_fix.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shapes", default="50000x21")
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
