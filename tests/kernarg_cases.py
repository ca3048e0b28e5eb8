"""The mean kernels take what their prologue reads first as leading plain kernel parameters (preloaded into SGPRs on gfx950;
cpi_mean_kernels.hpp: CPI_MEAN_LEAD_PARAMS / CPI_TILED_LEAD_PARAMS).  The arithmetic did not change with that, so every output is
BIT-EQUAL to what the library computed before the change.  This module states the cases -- the smallest shapes at which a
mis-ordered argument, or one truncated to 32 bits, shows -- runs them through a library, and digests the raw bytes of every output.

tests/golden/kernarg_parent_sha256.json holds the digests of the library built from the commit BEFORE the signature change
(recorded on an MI355X):
    CPI_AMD_LIB=<that commit's libcpi_amd.so> python -m tests.kernarg_cases --record
tests/test_gpu_kernarg_preload.py compares the product library's digests with them: sha256 over the bytes, no tolerance.

The inputs are integer hashes scaled by powers of two and a few elementwise IEEE operations -- the same bits with every numpy --
and their own digest is part of the record, so that a drifting generator is not mistaken for a drifting kernel."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernarg_parent_sha256.json")
WS = (1, 9, 10, 11, 63, 64, 65, 641)
NS = (1, 2, 3, 50)
LANES = (0, 1, 5, 6, 8, 64)            # 0: the library's own choice
LAYOUTS = ("dense", "csr", "cut1", "cut2", "cut3", "carry")
MODES = tuple((m, a) for m in (1, 2) for a in (0, 1))


def _u(n, seed):
    """n doubles in [0, 1): a 32-bit integer hash of (index, seed) over 2^32 -- exact in float64"""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed * 40503 + 12345)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 4294967296.0


def readings(K, seed, t0=1000.0):
    """[K, 7] IMU readings at 256 Hz: stamps exact, |w| <= 1 rad/s, a = gravity +- 3 m/s^2"""
    v = _u(K * 6, seed).reshape(K, 6)
    k = np.empty((K, 7))
    k[:, 0] = t0 + np.arange(K) / 256.0
    k[:, 1:4] = (v[:, :3] - 0.5) * 2.0
    k[:, 4:7] = (v[:, 3:] - 0.5) * 6.0
    k[:, 6] += 9.8
    return k


def lin_q(W, seed):
    lin = (_u(W * 6, seed + 1).reshape(W, 6) - 0.5) * 0.03125
    q = _u(W * 4, seed + 2).reshape(W, 4) - 0.5
    q[:, 3] += 1.0
    q = q / np.sqrt(q[:, 0:1] * q[:, 0:1] + q[:, 1:2] * q[:, 1:2] + q[:, 2:3] * q[:, 2:3] + q[:, 3:4] * q[:, 3:4])
    return np.ascontiguousarray(lin), np.ascontiguousarray(q)


def windows(W, N, seed):
    """dense knots [W, N + 1, 7]: window w starts w seconds after window 0"""
    k = readings(W * (N + 1), seed).reshape(W, N + 1, 7)
    k[:, :, 0] = 1000.0 + np.arange(W)[:, None] + np.arange(N + 1)[None, :] / 256.0
    return np.ascontiguousarray(k)


def digest(arrays):
    """sha256[:16] over the raw bytes of host arrays (a dict is taken in the order of its sorted keys)"""
    if isinstance(arrays, dict):
        arrays = [arrays[k] for k in sorted(arrays) if not k.startswith("_")]
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def _host(torch, out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _call(fn):
    """the digest of what fn returns, or the library's refusal (both libraries must then refuse alike)"""
    from cpi_amd._lib import CpiError
    try:
        return fn()
    except CpiError as e:
        return "refused:%d" % e.code


def run_layout(eng, layout, W):
    """{case id: digest} of one layout at W windows: every N, model, imu_avg and lane count"""
    import torch
    dev = eng.device
    res = {}
    for N in NS:
        seed = 1000 * W + N
        lin_h, q_h = lin_q(W, seed)
        lin, q = torch.from_numpy(lin_h).to(dev), torch.from_numpy(q_h).to(dev)
        extra = {}
        if layout in ("dense", "carry"):
            kn_h = windows(W, N, seed)
            kn = torch.from_numpy(kn_h).to(dev)
            res["N%d/inputs" % N] = digest([kn_h, lin_h, q_h])
        elif layout == "csr":
            # a shared stream: window w owns count[w] + 1 knots from first[w]; the windows overlap and are not in address order
            K = W * N + N + 1
            kn_h = readings(K, seed)
            first_h = ((np.arange(W, dtype=np.int64) * 7919) % W) * N
            count_h = (N - (np.arange(W) % 3 == 1) * min(1, N)).astype(np.int32)
            count_h[0] = N
            kn = torch.from_numpy(kn_h).to(dev)
            extra = dict(first=torch.from_numpy(first_h).to(dev), count=torch.from_numpy(count_h).to(dev), N=N)
            res["N%d/inputs" % N] = digest([kn_h, lin_h, q_h, first_h, count_h])
        else:
            # one stream (cut3: two runs) cut every N samples, 3/8 of a sample period behind a reading: N whole intervals and a tail
            R = 2 if (layout == "cut3" and W >= 2) else 1
            uo = [0, W] if R == 1 else [0, W // 2, W]
            runs, upds = [], []
            for r in range(R):
                Ur = uo[r + 1] - uo[r]
                runs.append(readings(Ur * N + 2, seed + 17 * r, t0=1000.0 + 50.0 * r))
                upds.append(runs[-1][0, 0] + (np.arange(1, Ur + 1) * N + 0.375) / 256.0)
            st_h, up_h = np.concatenate(runs), np.concatenate(upds)
            so = np.concatenate([[0], np.cumsum([len(x) for x in runs])]).astype(np.int64)
            st, up = torch.from_numpy(st_h).to(dev), torch.from_numpy(up_h).to(dev)
            res["N%d/inputs" % N] = digest([st_h, up_h, lin_h, q_h])
        for model, avg in MODES:
            for L in LANES:
                prm = eng.make_params(model, imu_avg=bool(avg), lanes_per_window=L)
                key = "N%d/m%d/a%d/L%d" % (N, model, avg, L)
                if layout in ("dense", "csr"):
                    res[key] = _call(lambda: digest(_host(torch, eng.preintegrate(kn, lin, q, prm, want=("mean",), **extra))))
                elif layout == "carry":
                    def carry():
                        # the records start zeroed: a call writes only the blocks of the record that it owns, and the rest is digested too
                        d, cd = [], eng.carry_doubles(prm.model)
                        for want in (("mean",), ("mean", "jac")):
                            z1, z2 = (torch.zeros((W, cd), dtype=torch.float64, device=dev) for _ in range(2))
                            o1, c1 = eng.preintegrate_resume(kn, lin, q, prm, want=want, carry_out=z1)
                            o2, c2 = eng.preintegrate_resume(kn, lin, q, prm, want=want, carry_in=c1, carry_out=z2)
                            d += [digest(_host(torch, o1)), digest(_host(torch, o2)), digest([c1.cpu().numpy(), c2.cpu().numpy()])]
                        return digest([np.frombuffer("".join(d).encode(), dtype=np.uint8)])
                    res[key] = _call(carry)
                elif layout == "cut3":
                    res[key] = _call(lambda: digest(_host(torch, eng.preintegrate_streams(
                        st, torch.from_numpy(so).to(dev), up, torch.tensor(uo, dtype=torch.int64, device=dev), lin, q, prm,
                        want=("mean",), N=N + 1))))
                else:
                    want = ("mean", "jac") if layout == "cut1" else ("mean",)     # Jacobians asked for: the windows are cut by a kernel of their own
                    res[key] = _call(lambda: digest(_host(torch, eng.preintegrate_stream(st, up, lin, q, prm, want=want, N=N + 1))))
    return res


def run_tiled(eng, W):
    """the tiled layout: plain (one wavefront per tile), SPLIT (4 and 8 wavefronts per tile) and the library's choice"""
    import torch
    dev = eng.device
    res = {}
    for N in (3, 50):
        seed = 1000 * W + N + 5
        kn_h = windows(W, N, seed)
        lin_h, q_h = lin_q(W, seed)
        count_h = (N - (np.arange(W) % 4)).clip(0, N).astype(np.int32)
        kn, lin, q = (torch.from_numpy(x).to(dev) for x in (kn_h, lin_h, q_h))
        cnt = torch.from_numpy(count_h).to(dev)
        tiles = eng.tile_knots(kn)
        res["N%d/inputs" % N] = digest([kn_h, lin_h, q_h, count_h])
        res["N%d/tiles" % N] = digest([tiles.cpu().numpy()])
        for model, avg in MODES:
            for S in (0, 1, 4, 8):
                for counted in (0, 1):
                    prm = eng.make_params(model, imu_avg=bool(avg), lanes_per_window=S)
                    res["N%d/m%d/a%d/S%d/c%d" % (N, model, avg, S, counted)] = _call(lambda: digest(_host(torch, eng.preintegrate_tiled(
                        tiles, W, lin, q, prm, count=cnt if counted else None))))
    return res


def run_offset_2mib(eng):
    """dense, the knots 8 bytes behind a 2 MiB boundary (the headline's lane count and the library's choice)"""
    import torch
    W, N, two_mib = 641, 50, 1 << 21
    kn_h = windows(W, N, 77)
    lin_h, q_h = lin_q(W, 77)
    n = kn_h.size
    buf = torch.zeros(n + two_mib // 8 + 2, dtype=torch.float64, device=eng.device)
    off = ((-buf.data_ptr()) % two_mib + 8) // 8
    kn = buf[off:off + n].view(W, N + 1, 7)
    assert kn.data_ptr() % two_mib == 8 and kn.is_contiguous()
    kn.copy_(torch.from_numpy(kn_h))
    lin, q = torch.from_numpy(lin_h).to(eng.device), torch.from_numpy(q_h).to(eng.device)
    res = {"inputs": digest([kn_h, lin_h, q_h])}
    for model in (1, 2):
        for L in (0, 6):
            res["m%d/L%d" % (model, L)] = _call(lambda: digest(_host(torch, eng.preintegrate(
                kn, lin, q, eng.make_params(model, lanes_per_window=L), want=("mean",)))))
    return res


def run_beyond_4gib(eng):
    """W (N + 1) 56 bytes > 2^32, addressed through `first`: the knot array holds just the 4 W knots the windows read, and the
    knots pointer handed to the library lies SHIFT knots in front of it, so that first[w] = SHIFT + 4 w (SHIFT * 56 bytes > 2^32)
    reaches them -- an index or a product that lost its upper half would read (or fault) elsewhere."""
    import torch
    W, N, SHIFT = 1201, 65535, 80000000
    assert W * (N + 1) * 56 > 2 ** 32 and SHIFT * 56 > 2 ** 32
    kn_h = readings(4 * W, 91)
    lin_h, q_h = lin_q(W, 91)
    first_h = SHIFT + 4 * ((np.arange(W, dtype=np.int64) * 7919) % W)
    count_h = (1 + np.arange(W) % 3).astype(np.int32)
    dev = eng.device
    kn, lin, q, first, count = (torch.from_numpy(x).to(dev) for x in (kn_h, lin_h, q_h, first_h, count_h))
    res = {"inputs": digest([kn_h, lin_h, q_h, first_h, count_h])}
    for model in (1, 2):
        for L in (0, 1, 6):
            prm = eng.make_params(model, lanes_per_window=L)
            out = eng.alloc_outputs(W, ("mean",), model)
            o = eng._outputs_struct(out)
            eng._sync_stream()
            rc = eng.lib.cpi_preintegrate_batch(eng.ctx, C.byref(prm), W, N, C.c_void_p(kn.data_ptr() - SHIFT * 56), C.c_void_p(first.data_ptr()),
                                                C.c_void_p(count.data_ptr()), C.c_void_p(lin.data_ptr()), C.c_void_p(q.data_ptr()), C.byref(o))
            res["m%d/L%d" % (model, L)] = digest(_host(torch, out)) if rc == 0 else "refused:%d" % rc
    return res


def groups():
    """(group id, runner) of every golden group"""
    g = [("%s/W%d" % (layout, W), (lambda eng, layout=layout, W=W: run_layout(eng, layout, W))) for layout in LAYOUTS for W in WS]
    g += [("tiled/W%d" % W, (lambda eng, W=W: run_tiled(eng, W))) for W in (65, 641)]
    g += [("offset_2mib", run_offset_2mib), ("beyond_4gib", run_beyond_4gib)]
    return g


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    assert "--record" in sys.argv, "usage: CPI_AMD_LIB=<library of the commit before the change> python -m tests.kernarg_cases --record [FILE]"
    import cpi_amd
    path = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    eng = cpi_amd.Engine()
    rec = {"build_id": (eng.lib.cpi_build_id() or b"").decode(), "groups": {}}
    for gid, fn in groups():
        rec["groups"][gid] = fn(eng)
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d digests in %d groups -> %s" % (sum(len(v) for v in rec["groups"].values()), len(rec["groups"]), path))
