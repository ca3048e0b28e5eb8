"""CPU-only: the multi-run stream entry (cpi_preintegrate_streams) -- its symbols, its workspace arithmetic and the Python bound
(Engine.streams_bound) against a plain restatement of the reference's deque loop, run by run."""
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpi_streams_workspace_bytes", "cpi_preintegrate_streams", "cpi_preintegrate_streams_host")


def test_streams_symbols_are_declared_and_exported():
    from cpi_amd import _lib, build
    from tests.test_abi import _declared_symbols
    lib = _lib.load()
    declared = _declared_symbols("cpi_amd.h")
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in NEW:
        assert s in declared and s in exported and hasattr(lib, s), s
    assert lib.cpi_abi_version() == 3


def test_streams_workspace_is_prefix_compatible_with_the_single_stream_workspace():
    """cpi_stream_counts(workspace, U) must find the counts of a multi-run call: the layout starts with the single-stream one."""
    import ctypes as C
    from cpi_amd import _lib
    lib = _lib.load()
    for U in (1, 2, 3, 7, 64, 549, 27450, 1_000_000):
        one = lib.cpi_stream_workspace_bytes(U)
        assert one == 3 * ((U * 8 + 15) // 16 * 16) + (U * 4 + 15) // 16 * 16
        for R in (1, 2, 50, 10_000):
            many = lib.cpi_streams_workspace_bytes(R, U)
            assert many >= one and many % 16 == 0, (R, U)
        base = 1 << 20
        off = lib.cpi_stream_counts(C.c_void_p(base), U) - base
        assert off % 16 == 0 and off + 4 * U <= lib.cpi_streams_workspace_bytes(50, U)
    assert lib.cpi_streams_workspace_bytes(3, 0) == lib.cpi_stream_workspace_bytes(0)


def _deque_loop_longest(stamps, update_times):
    """GraphSolver_IMU.cpp:50-69 on one run, literally: the most whole intervals of a window over its update times, plus the
    tail interval the bound always allows for (Engine.stream_bound).  0 when the run has no reading or no update time."""
    K = len(stamps)
    if K == 0 or len(update_times) == 0:
        return 0
    front, front_t, best = 0, stamps[0], 0
    for T in update_times:
        n = 0
        while K - front > 1 and stamps[front + 1] <= T:
            front += 1
            front_t = stamps[front]
            n += 1
        if T - front_t > 0:
            front_t = T
        best = max(best, n)
    return best + 1


def _runs(rng):
    """Runs whose clocks all start near 0 (stamps go backwards at every boundary), with 0 .. 3 readings, gaps, repeated update
    times, update times before the first and after the last reading, and a run without update times."""
    runs = []
    for K, U in ((40, 5), (0, 3), (1, 2), (2, 4), (3, 3), (25, 0), (60, 9), (4, 1)):
        t = np.cumsum(rng.uniform(0.004, 0.006, K)) if K else np.zeros(0)
        if K > 10:
            t[K // 2:] += 0.3                      # a gap
        lo, hi = (t[0] if K else 0.0) - 0.01, (t[-1] if K else 0.1) + 0.02
        ut = np.sort(rng.uniform(lo, hi, U))
        if U > 2:
            ut[1] = ut[2]                          # repeated
        runs.append((t, ut))
    return runs


def test_streams_bound_is_the_per_run_deque_loop_maximum():
    from cpi_amd import Engine
    rng = np.random.default_rng(5)
    for _ in range(4):
        runs = _runs(rng)
        order = rng.permutation(len(runs))
        runs = [runs[i] for i in order]
        stamps = np.concatenate([t for t, _ in runs])
        ut = np.concatenate([u for _, u in runs])
        so = np.concatenate([[0], np.cumsum([len(t) for t, _ in runs])]).astype(np.int64)
        uo = np.concatenate([[0], np.cumsum([len(u) for _, u in runs])]).astype(np.int64)
        stream = np.zeros((len(stamps), 7))
        stream[:, 0] = stamps
        want = max(1, max(_deque_loop_longest(t, u) for t, u in runs))
        got = Engine.streams_bound(torch.from_numpy(stream), torch.from_numpy(so), torch.from_numpy(ut), torch.from_numpy(uo))
        assert got == want, (got, want)
        # the bound of ONE run is the single-stream entry's bound
        for t, u in runs:
            if len(t) and len(u):
                s1 = np.zeros((len(t), 7)); s1[:, 0] = t
                one = Engine.streams_bound(torch.from_numpy(s1), [0, len(t)], torch.from_numpy(u), [0, len(u)])
                assert one == Engine._stream_bound(torch.from_numpy(s1), torch.from_numpy(u)) == max(1, _deque_loop_longest(t, u))
    # nothing to cut: the smallest bound the entry accepts
    assert Engine.streams_bound(torch.zeros((0, 7)), [0, 0], torch.zeros(3), [0, 3]) == 1
