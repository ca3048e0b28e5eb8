"""CPU only: the strand shape of cpi_amd/csrc/cpi_capture_overlap.hpp as a stand-alone program
(tests/cpp/test_capture_strands_cpu.cpp) built with AddressSanitizer + UBSan: RangeSet (merging of overlapping, touching and
identical ranges, empty ranges, the saturating top range, overflow reported and nothing written), the strand bookkeeping with fake
node ids -- the ordering invariant of DESIGN.md 3.7 by brute-force reachability over 200 random call sequences per strand count,
once more with 4-range summaries so that overflow joins occur -- the fixed patterns (the headline's walk without a join, one
output set, round-robin, a join) and the choice of a new context's shape from the three environment variables.  The program
checks itself; nothing of it is loaded into this process."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rangeset_strands_invariant_and_policy_under_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_capture_strands_cpu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "test_capture_strands_cpu.cpp"), "-o", exe])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
        assert p.stdout.splitlines()[-1].startswith("test_capture_strands_cpu ok"), p.stdout[-4000:]
