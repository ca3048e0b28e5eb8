"""GPU: the graph that eight captured cpi_preintegrate_batch calls leave behind on two strands (cpi_ctx_set_capture_strands), read
back with hipGraphGetNodes / hipGraphGetEdges by tests/cpp/test_capture_strands.cpp against libcpi_amd.so: disjoint calls form
two chains (node i behind node i-2 alone, 6 edges, no path between neighbours) and replay bit for bit what the eager calls write,
calls into one output set stay one chain, a call whose output overlaps the previous call's by one row follows it on its strand, one
strand is a chain, and a hipMemcpyAsync captured between two calls is ordered against everything on both sides.  The program
checks itself."""
import os
import subprocess
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_captured_graph_has_the_edges_the_footprints_ask_for():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from cpi_amd import _lib, build
    _lib.load()
    libdir = os.path.dirname(build.LIB)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_capture_strands")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               os.path.join(ROOT, "tests", "cpp", "test_capture_strands.cpp"), "-o", exe,
                               "-L" + libdir, "-lcpi_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
        assert p.stdout.splitlines()[-1].startswith("test_capture_strands ok"), p.stdout[-4000:]
