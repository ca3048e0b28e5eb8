"""The chains of the "device's own hess" case of the chain-solve tests, shared by the CPU pre-check (tests/test_chain_cpu.py) and the GPU
test (tests/test_gpu_chain.py).  TEST INFRASTRUCTURE ONLY.

C = 8 chains of 6 states.  The 40 windows are synth.make_windows(40, 50, BASE_SEED + 31); the first state of a chain is seeded, the
others are predicted from it along the chain's measurements, and every state is then moved by a small seeded step (the sigmas of
synth.make_states: 1e-3 rad, 1e-4, 1e-2 m/s, 1e-3, 1e-2 m).  The prior of a chain's first state is centred on the UNPERTURBED state,
information 0.1 diag(scales)^2 (tests/chain_cases.py), relinearised at the perturbed one: eta = Lam local(state, centre).
cpu_case() restates the whole case in longdouble with tests/factor_cases.py: the oracle's preintegration, predict_longdouble,
hessian_longdouble, the reference solve of tests/chain_cases.py, and the whitened cost before and after the step."""
import numpy as np
import torch

from cpi_amd import synth
from tests import chain_cases as cc

C, G = 8, 6
F, S = C * (G - 1), C * G
STEP_SIGMA = [1e-3] * 3 + [1e-4] * 3 + [1e-2] * 3 + [1e-3] * 3 + [1e-2] * 3


def inputs():
    """CPU float64 tensors: knots [F, 51, 7], lin [F, 6], q_k_lin [F, 4], x0 [C, 16] (the chains' first states), step [S, 15]."""
    kn, lin, q = synth.make_windows(F, 50, seed=synth.BASE_SEED + 31, edge_cases=False)
    g = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x0 = torch.zeros((C, 16), dtype=torch.float64)
    qq = rn(C, 4)
    qq = qq / qq.norm(dim=1, keepdim=True)
    x0[:, 0:4] = torch.where(qq[:, 3:4] < 0, -qq, qq)
    first_factor = torch.arange(C) * (G - 1)
    x0[:, 4:7] = lin[first_factor, 0:3] + 1e-4 * rn(C, 3)
    x0[:, 7:10] = rn(C, 3)
    x0[:, 10:13] = lin[first_factor, 3:6] + 1e-3 * rn(C, 3)
    x0[:, 13:16] = 5 * rn(C, 3)
    step = rn(S, 15) * torch.tensor(STEP_SIGMA, dtype=torch.float64)
    return dict(knots=kn, lin=lin, q=q, x0=x0, step=step)


def indices():
    """(idx_i, idx_j) of the F factors, chain after chain."""
    ii = (np.arange(C)[:, None] * G + np.arange(G - 1)[None, :]).reshape(-1)
    return ii, ii + 1


def packed_prior(xi0):
    """[S, 136] from xi0 [C, 15] = local(perturbed first state, its unperturbed centre): the first state of every chain, zeros elsewhere."""
    lam0 = 0.1 * cc.SCALES ** 2
    P = np.zeros((S, 16, 16))
    P[0::G, np.arange(15), np.arange(15)] = lam0
    P[0::G, :15, 15] = P[0::G, 15, :15] = lam0 * np.asarray(xi0)
    return cc.pack_upper(P)


def cpu_case():
    """The case in longdouble on the CPU -> dict(before, after: the whitened cost 0.5 sum |R e|^2 at the perturbed states and after the
    reference step; cond: the largest condition number of the eight systems)."""
    from oracle import oracle_py as op
    from tests import factor_cases as fc
    from tests.tol import sqrt_info_longdouble
    x = inputs()
    kn, lin = x["knots"].numpy(), x["lin"].numpy()
    orc = op.oracle()
    out = orc.run(op.make_params(1, 0, 1), kn, lin, x["q"].numpy())
    rec = op.factor_records(out, lin, None)
    Rl = sqrt_info_longdouble(np.asarray(out["P"]).reshape(F, 15, 15))                     # P is symmetric: either storage order
    R = np.ascontiguousarray(Rl.transpose(0, 2, 1).reshape(F, 225))                         # column-major flat, as the entries take it
    pred = np.zeros((S, 16))
    pred[0::G] = x["x0"].numpy()
    for k in range(G - 1):
        rows = np.arange(C) * (G - 1) + k
        pred[k + 1::G] = np.asarray(fc.predict_longdouble(1, rec[rows], pred[k::G]), dtype=np.float64)
    states = np.stack([orc.retract(pred[s], x["step"].numpy()[s]) for s in range(S)])
    xi0 = np.stack([orc.local(states[c * G], pred[c * G]) for c in range(C)])
    prior = packed_prior(xi0)
    ii, jj = indices()

    def linearise(st):
        ref = fc.evaluate_error_longdouble(1, rec, st[ii], st[jj])
        w = fc.whitened_longdouble(ref, R)[0]
        return ref, float(0.5 * (w * w).sum())

    ref, before = linearise(states)
    hess = np.asarray(fc.hessian_longdouble(ref, R), dtype=np.float64)
    b = cc.Batch.from_arrays([G] * C, np.arange(C) * G, np.arange(C) * (G - 1), hess, prior)
    sol = cc.Reference(b)
    sol.check_inputs()
    trial = np.stack([orc.retract(states[s], sol.delta[s]) for s in range(S)])
    return dict(before=before, after=linearise(trial)[1], cond=float(sol.cond.max()))
