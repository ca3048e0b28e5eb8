"""CPU: the window lookup and the patched-stamp accessor of cpi_query_stream_batch's kernels (cpi_query_stream_kernels.hpp:
squery_window, squery_cut, squery_stamp, squery_interval), compiled with the host compiler from the kernels' own header
(tests/hostsim/hostsim_query_stream.cpp), against numpy: searchsorted(side="left") clamped to the run's last window, and the knots
cpi_amd.stream.assemble_windows cuts from the same stream."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cpi_amd import stream as st

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim", "hostsim_query_stream.cpp")
_LIB = os.path.join(_HERE, "hostsim", "libhostsim_query_stream.so")
_HDRS = [os.path.join(os.path.dirname(_HERE), "cpi_amd", "csrc", h) for h in ("cpi_math.hpp", "cpi_query_stream_kernels.hpp")]


@pytest.fixture(scope="module")
def lib():
    if (not os.path.exists(_LIB)) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in [_SRC] + _HDRS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB, _SRC])
    return C.CDLL(_LIB)


def _p(a, t=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def trips_of(n):
    t = 0
    while (1 << t) < n + 1:
        t += 1
    return t


def window(lib, ut, uo, qrun, qt, trips=None):
    ut, qt = np.ascontiguousarray(ut, dtype=np.float64), np.ascontiguousarray(qt, dtype=np.float64)
    uo = None if uo is None else np.ascontiguousarray(uo, dtype=np.int64)
    qrun = None if qrun is None else np.ascontiguousarray(qrun, dtype=np.int32)
    out = np.full(len(qt), -7, dtype=np.int64)
    R = 1 if uo is None else len(uo) - 1
    assert lib.hqs_window(_p(ut), C.c_longlong(len(ut)), _p(uo, C.c_longlong), R, C.c_longlong(len(qt)), _p(qrun, C.c_int), _p(qt),
                          trips_of(len(ut)) if trips is None else trips, _p(out, C.c_longlong)) == 0
    return out


def window_np(ut, uo, qrun, qt):
    uo = [0, len(ut)] if uo is None else [min(max(int(v), 0), len(ut)) for v in uo]
    R = len(uo) - 1
    out = []
    for k, t in enumerate(qt):
        r = 0 if qrun is None else min(max(int(qrun[k]), 0), R - 1)
        u0, u1 = uo[r], max(uo[r + 1], uo[r])
        if u1 <= u0:
            out.append(-1)
        elif t != t:
            out.append(u0)
        else:
            out.append(u0 + min(int(np.searchsorted(ut[u0:u1], t, side="left")), u1 - u0 - 1))
    return np.array(out, dtype=np.int64)


def _times(ut):
    """On every update time, one ulp above and below, between them, before the first, past the last, NaN."""
    ut = np.asarray(ut, dtype=np.float64)
    mids = 0.5 * (ut[:-1] + ut[1:]) if len(ut) > 1 else np.zeros(0)
    return np.concatenate([ut, np.nextafter(ut, np.inf), np.nextafter(ut, -np.inf), mids, [ut.min() - 1.0 if len(ut) else -1.0,
                           ut.max() + 1.0 if len(ut) else 1.0, np.nan]])


@pytest.mark.parametrize("U", [1, 2, 63, 64, 65])
def test_window_lookup_one_run(lib, U):
    """U on either side of a power of two: the trip count ceil(log2(U + 1)) changes between 63 and 64."""
    rng = np.random.default_rng(U)
    ut = np.cumsum(rng.uniform(0.01, 0.3, U)) + 5.0
    if U > 4:
        ut[3] = ut[2]                                       # equal update times: the first wins
    qt = _times(ut)
    got = window(lib, ut, None, None, qt)
    assert np.array_equal(got, window_np(ut, None, None, qt))
    assert (trips_of(63), trips_of(64)) == (6, 7)
    # the exact cases, spelled out: on an update time and one ulp below it that window (of equal ones the first), one ulp above it the
    # first window with a later update time, before the first 0, past the last U - 1, NaN 0
    assert got[-3] == 0 and got[-2] == U - 1 and got[-1] == 0
    for u in range(U):
        head = u if (u == 0 or ut[u] > ut[u - 1]) else u - 1
        assert got[u] == head and got[2 * U + u] == head and got[U + u] == min(int((ut <= ut[u]).sum()), U - 1), u


def test_window_lookup_many_runs(lib):
    """An empty run, a run of one window, equal update times, qrun at -3 and R + 5, every run's clock starting at 0."""
    runs = [np.array([0.5, 1.0, 1.0, 2.0]), np.zeros(0), np.array([0.7]), np.array([0.1, 0.2, 0.3, 0.4, 0.5]), np.zeros(0)]
    ut = np.concatenate(runs)
    uo = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    R = len(runs)
    qrun, qt = [], []
    for r in list(range(R)) + [-3, R + 5]:
        ts = _times(runs[min(max(r, 0), R - 1)])
        qrun += [r] * len(ts)
        qt += list(ts)
    qrun, qt = np.array(qrun), np.array(qt)
    got = window(lib, ut, uo, qrun, qt)
    ref = window_np(ut, uo, qrun, qt)
    assert np.array_equal(got, ref)
    assert (got[qrun == 1] == -1).all() and (got[qrun == R + 5] == -1).all() and (got[qrun == 2] == 4).all()
    assert np.array_equal(got[qrun == -3], got[qrun == 0])
    # offsets that lie: clamped into [0, U], never a read outside update_times (the reference clamps the same way)
    for bad in ([-5, 2, 1, 40, 9, 9], [3, 3, 3, 3, 3, 3], [0, 100, 100, 100, 100, 100]):
        assert np.array_equal(window(lib, ut, bad, qrun, qt), window_np(ut, bad, qrun, qt)), bad


def _cut(stream, ut):
    """first / count / tstart / tend as the cut kernel leaves them (cpi_cut_windows_kernel's closed form of the reference's deque
    loop), checked against the host assembler's windows."""
    knots, first, count = st.assemble_windows(stream, ut)
    t = stream[:, 0]
    f, ts, te = [], [], []
    for u, T in enumerate(ut):
        cT = int((t <= T).sum())
        fp = 0 if u == 0 else max(int((t <= ut[u - 1]).sum()) - 1, 0)
        start = t[0] if u == 0 else max(ut[u - 1], t[0])
        fu = max(cT - 1, 0, fp)
        front_t = t[fu] if fu > fp else start
        tail = T - front_t > 0
        assert count[u] == fu - fp + int(tail) and knots[first[u], 0] == start and np.array_equal(knots[first[u], 1:], stream[fp, 1:])
        f.append(fp); ts.append(start); te.append(T if tail else np.nan)
    return knots, first, count, np.array(f, dtype=np.int64), np.array(ts), np.array(te)


@pytest.mark.parametrize("trunc", [0, 3])
def test_stamps_and_interval_match_the_assembled_windows(lib, trunc):
    """Windows with and without a tail, of 0 intervals, and truncated to N: the stamps the accessor returns are the assembled
    knots' stamps, and the interval search is searchsorted(side="right") - 1 over them."""
    rng = np.random.default_rng(4)
    K = 60
    stream = np.concatenate([np.cumsum(rng.uniform(0.004, 0.006, K))[:, None] + 10.0, rng.standard_normal((K, 6))], axis=1)
    t = stream[:, 0]
    ut = np.array([t[0] - 0.1, t[7] + 0.001, t[7] + 0.001, t[15], t[30] + 0.002, t[31] + 0.001, t[-1] + 0.3])
    knots, first, count, f, ts, te = _cut(stream, ut)
    assert list(count) == [0, 8, 0, 8, 16, 2, 29] and np.isnan(te[[0, 2, 3]]).all() and not np.isnan(te[[1, 4, 5, 6]]).any()
    N = int(count.max()) - trunc
    trips = trips_of(N)
    stamps = np.zeros(N + 1)
    n, i, rd = C.c_int(), C.c_int(), C.c_longlong()
    cnt = count.astype(np.int32)
    for u in range(len(ut)):
        nn = min(int(count[u]), N)
        want = knots[first[u]:first[u] + nn + 1, 0]
        qs = np.concatenate([want, np.nextafter(want, np.inf), np.nextafter(want, -np.inf), 0.5 * (want[:-1] + want[1:]),
                             [want[0] - 1, want[-1] + 1, np.nan]])
        for tq in qs:
            assert lib.hqs_stamps(_p(stream), C.c_longlong(K), _p(f, C.c_longlong), _p(cnt, C.c_int), _p(ts), _p(te), C.c_longlong(u), N,
                                  C.c_double(tq), trips, _p(stamps), C.byref(n), C.byref(i), C.byref(rd)) == 0
            assert n.value == nn and np.array_equal(stamps[:nn + 1], want) and np.isnan(stamps[nn + 1:]).all(), u
            ref_i = 0 if tq != tq else max(int(np.searchsorted(want, tq, side="right")) - 1, 0)
            assert i.value == ref_i, (u, tq)
            # the reading of knot i is the assembled knot's (the tail knot repeats the reading before it), inside the stream
            assert 0 <= rd.value < K and np.array_equal(stream[rd.value, 1:], knots[first[u] + ref_i, 1:]), (u, tq)
