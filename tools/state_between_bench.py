"""What cpi_state_between_batch costs: one pose measurement per factor -- in place, out of place and cost only --, the same with every
tenth factor measured, beside a plain copy of hess (the reference point: the in-place call touches 91 of 496 entries of a row) and
beside the Hessian sweep that feeds it.  Needs a GPU.

  python tools/state_between_bench.py [--out profiles/state_between.json] [--reps 11] [--shapes 50000x21] [--step-timeout 300]

Every shape runs in a child process of its own under --step-timeout; the parent stops at the first child that fails or runs out of time.
Per shape C x G -- C chains of G states back to back, real IMU factors (synth.make_windows, 10 intervals each), one Gaussian prior per
chain on its first state, the rows of every factor those of factor_hessian.  Alternating call by call in one process, each after
100 ms of untimed calls of its own, HIP events around the call(s) (tools/chain_solve_bench.py: alternate):
  between_inplace       cpi_state_between_batch, pose, one measurement per factor, hess == hess_base (rows only)
  between_outofplace    the same onto a second array: every row is moved whole
  between_cost          the same with hess = NULL: chi2 in place (the two cost evaluations of an iteration)
  tenth_inplace / tenth_outofplace / tenth_cost    every tenth factor measured (M = F / 10)
  position_inplace      the position kind, one measurement per factor, in place
  hess_copy             out.copy_(hess): 3968 bytes in and out per factor
  factor_hessian, chain_solve     the two sweeps an iteration is made of, on the same box
  iteration_eager / iteration_betweens_eager   one iteration of Engine.chain_lm without / with the pose measurements
Reported: median / min / max in ms, the bytes the kernel must move with their fraction of 8 TB/s, each form's ratio to the copy and to
factor_hessian and its share of an eager iteration.  Prints one JSON document (with the library's build id) and writes it to --out."""
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

    # measurements: the relative pose of the states themselves, the position part moved by 2 cm
    xi, xj = states[ii.long()], states[jj.long()]
    qi_inv = torch.cat([-xi[:, :3], xi[:, 3:4]], dim=1)
    qv, pv, qw, pw = xj[:, :3], qi_inv[:, :3], xj[:, 3:4], qi_inv[:, 3:4]    # q_j (x) inv(q_i), JPL
    zq = torch.cat([qw * pv - torch.linalg.cross(qv, pv) + pw * qv, qw * pw - (qv * pv).sum(1, keepdim=True)], dim=1)
    zq = zq / zq.norm(dim=1, keepdim=True)
    w_, v_ = xi[:, 3], xi[:, :3]                                              # y = R_i (p_j - p_i), R_i = quat_2_Rot(q_i)
    d = xj[:, 13:16] - xi[:, 13:16]
    y = (2 * w_ * w_ - 1)[:, None] * d - 2 * w_[:, None] * torch.linalg.cross(v_, d) + 2 * v_ * (v_ * d).sum(1, keepdim=True)
    z = torch.cat([zq, y + 0.02 * torch.randn((F, 3), generator=gen, **f64)], dim=1).contiguous()
    Rq = torch.zeros((F, 21), **f64)
    Rq[:, [a * (a + 1) // 2 + a for a in range(6)]] = torch.tensor([100.0] * 3 + [50.0] * 3, **f64)
    Rq[:, 4 * 5 // 2 + 1] = 5.0
    mfirst = torch.arange(F + 1, dtype=torch.int64, device=dev)
    T = F // 10
    tenth = torch.arange(0, 10 * T, 10, dtype=torch.int64, device=dev)        # the measured factors
    mtenth = eng.fix_offsets(tenth, F)
    zt, Rt10 = z[tenth].contiguous(), Rq[tenth].contiguous()
    zp, Rp = z[:, 4:].contiguous(), torch.zeros((F, 6), **f64)
    Rp[:, [0, 2, 5]] = 20.0
    betweens = [dict(kind="pose", z=z, R=Rq, mfirst=mfirst)]

    bufs, bufs_b = {}, {}
    common = dict(idx_i=ii, idx_j=jj, prior0=prior0, anchor=anchor, prior_idx=pidx, lam=1e-3)
    run = lambda n, init: eng.chain_lm(1, m, lin, None, states, Rt, C, G, iterations=n, buffers=bufs, init=init, **common)
    run_b = lambda n, init: eng.chain_lm(1, m, lin, None, states, Rt, C, G, iterations=n, buffers=bufs_b, init=init, betweens=betweens, **common)
    st0 = states.clone()
    run(1, True)
    states.copy_(st0)
    run_b(1, True)
    states.copy_(st0)
    torch.cuda.synchronize()
    hess, chi2 = bufs["hess"], bufs["chi2"]
    eng.factor_hessian(1, m, lin, None, states, Rt, ii, jj, out=hess)
    out = torch.zeros((F, 496), **f64)
    delta, status, ws, prior = bufs["delta"], bufs["status"], bufs["workspace"], bufs["prior"]

    def between(kind, zz, RR, mf, rows, inplace):
        if not rows:
            return eng.state_between(states, kind, zz, RR, mf, ii, jj, chi2_base=chi2, chi2=chi2, want_rows=False)
        return eng.state_between(states, kind, zz, RR, mf, ii, jj, hess_base=hess, out=hess if inplace else out, want_cost=False)

    fns = {
        "between_inplace": lambda: between("pose", z, Rq, mfirst, True, True),
        "between_outofplace": lambda: between("pose", z, Rq, mfirst, True, False),
        "between_cost": lambda: between("pose", z, Rq, mfirst, False, False),
        "tenth_inplace": lambda: between("pose", zt, Rt10, mtenth, True, True),
        "tenth_outofplace": lambda: between("pose", zt, Rt10, mtenth, True, False),
        "tenth_cost": lambda: between("pose", zt, Rt10, mtenth, False, False),
        "position_inplace": lambda: between("position", zp, Rp, mfirst, True, True),
        "hess_copy": lambda: out.copy_(hess),
        "factor_hessian": lambda: eng.factor_hessian(1, m, lin, None, states, Rt, ii, jj, out=out),
        "chain_solve": lambda: eng.chain_solve(out, C=C, G=G, prior=prior, lam=bufs["lam"], damping="diagonal", out=delta, status=status, workspace=ws),
        "iteration_eager": lambda: run(1, False),
        "iteration_betweens_eager": lambda: run_b(1, False),
    }
    t = alternate(fns, reps)
    per = 8 * (2 * 16 + 2 + 2)                                                # two states, two mfirst entries, two indices (as 8 bytes)
    pose, pos = 8 * (7 + 21), 8 * (3 + 6)
    nbytes = {"between_inplace": F * (per + pose + 2 * 8 * 91), "between_outofplace": F * (per + pose + 2 * 3968), "between_cost": F * (per + pose + 16),
              "tenth_inplace": F * 8 * 2 + T * (per + pose + 2 * 8 * 91), "tenth_outofplace": F * (8 * 2 + 2 * 3968) + T * (per + pose),
              "tenth_cost": F * (8 * 2 + 16) + T * (per + pose), "position_inplace": F * (per + pos + 2 * 8 * 55), "hess_copy": F * 2 * 3968}
    for k, b in nbytes.items():
        t[k]["bytes"] = b
        t[k]["fraction_of_8TBps"] = b / (t[k]["median"] * 1e-3) / PEAK
    it = t["iteration_betweens_eager"]["median"]
    for k in nbytes:
        if k != "hess_copy":
            t[k]["over_hess_copy"] = t[k]["median"] / t["hess_copy"]["median"]
            t[k]["over_factor_hessian"] = t[k]["median"] / t["factor_hessian"]["median"]
            t[k]["share_of_eager_iteration_with_betweens"] = t[k]["median"] / it
    t["betweens_share_of_eager_iteration"] = (t["between_inplace"]["median"] + t["between_cost"]["median"]) / it
    t["iteration_with_betweens_over_without"] = it / t["iteration_eager"]["median"]
    r = t["between_inplace"]["over_hess_copy"]
    t["between_inplace"]["verdict"] = "cheaper than a plain copy of hess" if r < 1.0 else "NOT cheaper than a plain copy of hess"
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_between.json"))
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
