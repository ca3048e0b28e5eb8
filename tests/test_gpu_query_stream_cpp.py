"""GPU: cpi_host::ImuStream::at / at_cov / at_stj and ImuStreamSet::at_stj (tests/cpp/test_query_stream.cpp) against libcpi_amd.so.
The program compares the facade with the route a caller had before -- host-assembled windows, a host lookup of every time's window,
cpi_query_stj_batch_host -- bit for bit, and checks itself."""
import os
import subprocess
import tempfile

import pytest
import torch

from cpi_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runs():
    """Three runs with every clock starting at 0: tails, update times on the grid, and a run of 2 readings."""
    out = []
    for W, n, seed, phase in ((4, 9, 5, 0.37), (3, 6, 6, 0.0), (1, 1, 7, 0.5)):
        s, u, _, _ = synth.make_stream(W, n, seed=seed, phase=phase)
        s, u = s.numpy().copy(), u.numpy().copy()
        u -= s[0, 0]
        s[:, 0] -= s[0, 0]
        out.append((s, u))
    return out


@pytest.mark.parametrize("model", [1, 2])
def test_query_stream_cpp_facade(model):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    runs = _runs()
    queries = sum(len(u) + len(s) + len(s) - 1 + 2 for s, u in runs)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_query_stream")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_query_stream.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        path = os.path.join(tmp, "runs.txt")
        with open(path, "w") as f:
            f.write("%d\n" % len(runs))
            for s, u in runs:
                f.write("%d %d\n" % (len(s), len(u)))
                for row in s:
                    f.write(" ".join("%.17g" % v for v in row) + "\n")
                f.write(" ".join("%.17g" % v for v in u) + "\n")
        for avg in (0, 1):
            p = subprocess.run([exe, path, str(model), str(avg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
            assert p.returncode == 0, p.stdout + p.stderr
            assert p.stdout.splitlines()[-1] == "test_query_stream ok %d" % queries, p.stdout
