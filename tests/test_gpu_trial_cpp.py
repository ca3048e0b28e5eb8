"""GPU: the C++ facade of the trial step (tests/cpp/test_trial.cpp) against libcpi_amd.so, product only: cpi_host::retract,
cpi_host::local_coordinates and ImuFactorCPI::error against the values Engine.retract / local_coordinates / factor_cost_host give for
the same inputs, written out here -- bit for bit, the same kernels behind another front.  The program checks itself."""
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cpi_amd
from tests import factor_cases as fc
from tests import trial_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trial_cpp_facade():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from cpi_amd import _lib, build
    _lib.load()
    eng = cpi_amd.Engine()
    S = 65
    states, delta, other, _ = (a[:S] for a in tc.states_and_steps())
    T = lambda a: torch.from_numpy(np.array(a, order="C"))                    # a copy: the cases are read-only
    dev = lambda a: T(a).to(eng.device)
    r = eng.retract(dev(states), dev(delta)).cpu().numpy()
    l = eng.local_coordinates(dev(states), dev(other)).cpu().numpy()
    words = [S] + [a.ravel() for a in (states, delta, other, r, l)]
    per_model = 3
    words.append(2 * per_model)
    for model in (1, 2):
        rows = np.array([0, 8, 44])[:per_model]                 # three regimes of factor_cases.mixed
        b = fc.mixed(model, 64)
        bc = fc.base_cases(model)
        base = b["base"][rows]
        P = eng.preintegrate(dev(bc["knots"][base]), dev(bc["lin"][base]), dev(bc["q_k_lin"][base]), eng.make_params(model),
                             want=("cov",))["P"].cpu()
        rec = b["rec"][rows]
        meas, lin, qlin = fc.meas_of(rec)
        m = {k: T(v) for k, v in meas.items()}
        m["P"] = P.contiguous()
        for k in range(per_model):
            one = {key: v[k:k + 1].contiguous() for key, v in m.items()}
            st = T(np.stack([b["xi"][rows[k]], b["xj"][rows[k]]]))
            want = eng.factor_cost_host(model, one, T(lin[k:k + 1]), T(qlin[k:k + 1]) if model == 2 else None, st,
                                        grav=tuple(rec[k, fc.C_GRAV]))
            assert float(want["total"][0]) == 0.5 * float(want["chi2"][0]) and np.isfinite(float(want["total"][0]))
            words += [model, meas["DT"][k], meas["alpha"][k], meas["beta"][k], meas["q"][k], meas["J_q"][k], meas["J_b"][k], meas["J_a"][k],
                      meas["H_b"][k], meas["H_a"][k], qlin[k], meas["O_b"][k], meas["O_a"][k], P[k].numpy(), rec[k, fc.C_GRAV],
                      lin[k, 3:6], lin[k, 0:3], b["xi"][rows[k]], b["xj"][rows[k]], want["total"].numpy()]
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe, path = os.path.join(tmp, "test_trial"), os.path.join(tmp, "trial.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_trial.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        with open(path, "w") as f:
            for w in words:
                f.write(" ".join("%.17g" % v for v in np.atleast_1d(np.asarray(w, dtype=np.float64)).ravel()) + "\n")
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.splitlines()[-1] == "test_trial ok %d %d" % (S, 2 * per_model), p.stdout
