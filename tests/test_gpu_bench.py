"""GPU: the DRIVER's bench command, verbatim (`python bench.py --gpus 1 --steps 20 --warmup 5`, no shortening flags) and the
same command with `--full`: the LAST stdout line is one JSON object small enough for the driver to keep whole (< 6 KB; round
3's line had grown to 33 KB and `BENCH_r03.parsed` came back null) and carries the contract's keys and the roofline of the
dominant kernel; the plain run measures nothing else, the --full run adds the CPU baseline, a compact BASELINE configs[2]
object, and names the file that holds the full extra rows.  `--dump-outputs` writes the last step's outputs, the same ones
from run to run."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5"]


def _bench(args, timeout):
    extra_path = os.path.join(ROOT, "bench_extra.json")
    if os.path.exists(extra_path):
        os.remove(extra_path)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout, wall, extra_path


@pytest.fixture(scope="module")
def driver_run():
    out = _bench(DRIVER_ARGS, 600)
    assert not os.path.exists(out[2]), "a plain run measures the headline only"
    return out


@pytest.fixture(scope="module")
def full_run():
    return _bench(DRIVER_ARGS + ["--full"], 1500)


def _contract_line(stdout, wall):
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    line = lines[-1]
    assert len(line) < 6000, len(line)
    # what the driver keeps is a tail of stdout: everything it needs must be inside the last 8 000 characters
    assert stdout.rstrip("\n")[-8000:].endswith(line)
    r = json.loads(line)
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert r["metric"].startswith(base["metric"].split(" at ")[0]) and r["unit"] == "windows/s"
    assert r["n_gpus"] == 1 and r["steps"] == 20 and r["warmup"] == 5
    assert r["higher_is_better"] is True and r["scaling"] == "weak" and r["vs_baseline"] is None
    assert r["dtype"] == "f64" and r["data"] == "synthetic" and "model" not in r["config"]
    for k in ("workload", "library_build", "launch_mode"):
        assert r["config"][k], k
    assert "configs[1]" in r["config"]["workload"]
    assert r["value"] > 1e8 and abs(r["value"] * r["ms_per_step"] * 1e-3 / 10000 - 1.0) < 1e-6      # 10 k windows per step
    assert r["ms_per_step"] * 1e-3 * r["steps"] <= wall                                              # fits in the run that produced it
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and rf["kernel"]
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0.05 < rf["frac"] < 1.0
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (rf["launch_us"] * 1e-6) / 1e9) < 1e-6 * rf["achieved"]
    assert rf["launch_us"] * 1e-3 <= r["ms_per_step"] * 1.001                                      # kernel time <= step time
    assert rf["traffic"] is None or rf["traffic"] > 0.9 * rf["algorithmic_bytes_per_launch"]
    return r


def test_the_last_stdout_line_of_the_drivers_command_parses_and_is_small(driver_run, full_run):
    plain = _contract_line(*driver_run[:2])
    # the plain run: the headline and nothing that takes runs of its own
    for k in ("cpu_baseline", "overlapped", "configs2", "routes_1M_x_50", "extra_rows", "extra_file"):
        assert k not in plain, k
    assert plain["value_full_integrator"] is None and plain["value_overlapped"] is None
    assert plain["goal_40pct_hbm"] == (plain["roofline"]["frac"] >= 0.40)
    r = _contract_line(*full_run[:2])
    rf = r["roofline"]
    cb = r["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "windows/s"
    assert cb["single_core_value"] > 0 and 0 < len(cb["sample"]) <= 200 and cb["sparse_port"]["value"] > 0
    # the north-star's 40 % criterion is answered in the line itself
    assert r["goal_40pct_hbm"] == (rf["frac"] >= 0.40) and "17 k" in r["goal_note"]
    # ... and so is the one route to it at this batch size: several batches in flight, MEASURED in the same run (round 5)
    ov = r["overlapped"]
    assert ov["contexts"] == 3 and ov["unit"] == "windows/s" and ov["value"] > r["value"] * 0.8 and ov["batches"] >= 1000
    assert abs(ov["value"] * ov["ms_per_batch"] * 1e-3 / 10000 - 1.0) < 1e-9
    assert abs(ov["frac"] - ov["value"] * rf["algorithmic_bytes_per_unit"] / 8e12) < 1e-9 and 0.1 < ov["frac"] < 1.0
    assert set(ov["frac_by_contexts"]) == {"2", "3", "4"} and r["goal_40pct_hbm_overlapped"] == (ov["frac"] >= 0.40)
    # BASELINE configs[2] (V2 + covariance + Jacobians: the row the >= 10 M windows/s goal sits on) travels in the parsed part
    c2 = r["configs2"]
    assert "configs[2]" in c2["workload"] and c2["value"] > 1e7 and c2["goal_10M_windows_per_s"] is True and c2["launch_ms"] > 0
    assert c2["cpu_baseline"]["value"] > 0 and c2["cpu_baseline"]["cores"] >= 1 and c2["cpu_baseline"]["kind"] in ("reference", "port")
    assert set(c2["fp64"]) >= {"frac", "useful_frac"}
    # `value` is the lightest configuration: the full integrator's rate and the overlapped rate stand beside it at the top level
    assert r["value_full_integrator"] == c2["value"] and r["value_overlapped"] == ov["value"]
    rt = r["routes_1M_x_50"]
    assert rt["stream_in_place"] > 0 and rt["assemble_tiles"] > 0 and rt["tiled_kernel"] > 0 and rt["dense_kernel_preassembled"] > 0
    assert "bench_extra.json" in r["extra_file"]


def test_the_full_extra_rows_land_in_bench_extra_json(full_run):
    stdout, _, extra_path = full_run
    r = json.loads([ln for ln in stdout.splitlines() if ln.strip()][-1])
    doc = json.load(open(extra_path))
    rows = doc["rows"]
    assert len(rows) >= 45
    assert not [x for x in rows if "error" in x], [x for x in rows if "error" in x]
    with_roof = [x for x in rows if "roofline" in x]
    assert len(with_roof) >= 44
    for x in with_roof:
        rf = x["roofline"]
        assert rf["achieved"] > 0 and rf["kernel"] and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert doc["headline"]["value"] == r["value"] and doc["headline"]["config"]["library_build"] == r["config"]["library_build"]
    # every measured row is pre-ramped like the headline (late round 6: a row that starts on an idle GPU timed the power controller's transient)
    import bench
    assert all(x.get("clock_preramp_ms") == bench.EXTRA_PRERAMP_MS for x in with_roof) and r["config"]["clock_preramp_ms"] > 0
    # the compact per-row summary of the line agrees with the file
    key = bench.row_key
    assert set(r["extra_rows"]) == {key(x) for x in rows}
    by = {key(x): x for x in rows}
    # round 6: the reference's own window lengths (10 / 20 samples) with roofline AND the reference's CPU leg at that length
    for k in ("v1_mean@1Mx10", "v1_mean@1Mx20", "v1_full@1Mx10", "v2_full@1Mx20"):
        assert by[k]["roofline"]["frac"] > 0 and by[k]["cpu_baseline"]["value"] > 0 and "%d-sample" % by[k]["samples"] in by[k]["cpu_baseline"]["sample"], k
    assert by["v1_mean@1Mx20"]["roofline"]["frac"] >= 0.50
    # ... and the packed-triangle rows of ABI 3 beside their dense twins
    assert by["sqrt_info_packed@1M"]["launch_ms"] < 0.70 * by["sqrt_info@1M"]["launch_ms"]
    # (rows of one run are measured minutes apart at whatever clock the box holds then: the same-box alternating A/B of the two
    #  forms is profiles/r06_packed.md; here only "not slower beyond the noise")
    assert by["factor_v1_whitened_tri@1M"]["launch_ms"] < 1.05 * by["factor_v1_whitened@1M"]["launch_ms"]


def test_no_extra_no_cpu_still_prints_one_contract_line():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "10", "--full", "--no-extra", "--no-cpu"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    r = json.loads(lines[0])
    assert r["steps"] == 50 and "configs2" not in r and "cpu_baseline" not in r and "overlapped" not in r and r["roofline"]["frac"] > 0.05


def test_dump_outputs_writes_the_last_steps_outputs_the_same_from_run_to_run(tmp_path):
    """`--dump-outputs DIR`: the arrays the timed path returns in its last step (mean-only: DT, alpha, beta, q of the 10 k windows), float64,
    bitwise the same in two runs with the same arguments (seeded inputs, one pass of the same kernels), and equal to an independent
    recompute of the batch that LAST step reads.  K = 22, W = 5: the last step is step 26 of the walk, whose batch is neither the first
    warm-up step's nor the first timed step's, so a dump of any step other than the last one of the walk's period fails."""
    import numpy as np
    import torch

    import cpi_amd
    from cpi_amd import synth
    steps, warmup = 22, 5
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    got = []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / d)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        r = json.loads(p.stdout.strip().splitlines()[-1])
        assert r["steps"] == steps and r["warmup"] == warmup
        got.append({f[:-4]: np.load(str(tmp_path / d / f)) for f in sorted(os.listdir(str(tmp_path / d)))})
    a, b = got
    assert set(a) == {"DT", "alpha", "beta", "q"}, sorted(a)
    for k, v in a.items():
        assert v.dtype == np.float64 and v.shape[0] == 10000 and np.isfinite(v).all(), k
        assert np.array_equal(v, b[k]), k
    assert (a["DT"] > 0).all() and np.allclose(np.linalg.norm(a["q"].reshape(10000, 4), axis=1), 1.0, atol=1e-12)
    # the independent recompute: the pool's batch b is synth.make_windows(seed = 20190101 + 101 b) (bench.main: base_seed(rank 0) and
    # Workload), the walk starts at step 0 after the clock pre-ramp, so step `warmup + steps - 1` reads batch (warmup + steps - 1) % pool
    nb = r["config"]["pool_batches"]
    last = warmup + steps - 1
    assert last % nb not in (0, warmup % nb), nb
    eng = cpi_amd.Engine(device=0)

    def recompute(batch):
        kn, lin, q = synth.make_windows(10000, 50, seed=20190101 + 101 * batch, device=eng.device)
        out = eng.preintegrate(kn, lin, q, eng.make_params(1), want=("mean",))
        torch.cuda.synchronize()
        return {k: out[k].cpu().numpy().reshape(a[k].shape) for k in a}

    want = recompute(last % nb)
    for k, v in a.items():
        assert np.abs(v - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
    before = recompute((last - 1) % nb)
    assert not np.array_equal(before["alpha"], a["alpha"])      # the check tells the steps apart
