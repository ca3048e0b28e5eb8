"""CPU only: cpi_amd/csrc/cpi_capture_overlap.hpp as a stand-alone program (tests/cpp/test_capture_overlap_cpu.cpp) built with
AddressSanitizer + UBSan: the conflict test of two calls' footprints (touching, nested, one-byte-overlapping and empty ranges,
NULL outputs, the unknown span of a CSR call) and the window bookkeeping with fake node ids -- the ordering invariant of
DESIGN.md 3.7 by brute-force reachability over 200 random call sequences (fixed seed).  The program checks
itself; nothing of it is loaded into this process."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_footprints_and_window_invariant_under_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_capture_overlap_cpu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "test_capture_overlap_cpu.cpp"), "-o", exe])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
        assert p.stdout.splitlines()[-1] == "test_capture_overlap_cpu ok", p.stdout[-4000:]
