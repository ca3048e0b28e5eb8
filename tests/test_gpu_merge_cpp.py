"""GPU: cpi_host::merge (tests/cpp/test_merge.cpp) against libcpi_amd.so, end to end and product only: the windows of an IMU stream
joined five by five against ImuStream::preintegrate at every 5th update time; the program checks itself.  Update times on the IMU
grid with imu_avg 0 and 1, and off the grid (a partial tail interval in every window) without imu_avg -- off the grid WITH imu_avg the
two sides are different integrands by the reference's own cut (tests/test_gpu_merge.py)."""
import os
import subprocess
import tempfile

import pytest
import torch

from cpi_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_cpp_facade():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_merge")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_merge.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        for phase, avgs in ((0.0, (0, 1)), (0.37, (0,))):
            stream, ut, _, _ = synth.make_stream(40, 10, phase=phase)
            sp, up = os.path.join(tmp, "stream.txt"), os.path.join(tmp, "ut.txt")
            with open(sp, "w") as f:
                for row in stream.numpy():
                    f.write(" ".join("%.17g" % v for v in row) + "\n")
            with open(up, "w") as f:
                f.write(" ".join("%.17g" % v for v in ut.numpy()) + "\n")
            for avg in avgs:
                p = subprocess.run([exe, sp, up, str(avg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
                assert p.returncode == 0, (phase, avg, p.stdout + p.stderr)
                assert p.stdout.splitlines()[-1] == "test_merge ok 8", p.stdout
