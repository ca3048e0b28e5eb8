"""CPU: bench.py's output contract without a GPU -- emit() turns a headline + the full extra rows into ONE last stdout line
of < 6 KB that the driver can parse (round 3's 33 KB line came back as `parsed: null`) and writes the full rows to
bench_extra.json."""
import json

import bench


def _row(name, W, with_cpu=True, N=None):
    N = N or bench.WORKLOADS[name]["N"]
    r = {"workload": name, "units_per_step": W, "samples": N, "value": 1.234567891234e8, "unit": "windows/s", "launch_ms": 1.23456789,
         "launch_mode": "graph", "roofline": bench.roofline_of(name, W, N, 1.2e-3, {}, "no profiles/r04_pmc.json")}
    if with_cpu:
        r["cpu_baseline"] = {"value": 4.0e4, "unit": "windows/s", "cores": 16, "kind": "reference", "single_core_value": 2.6e3, "sample": "x" * 300}
    return r


def test_emit_keeps_the_last_line_under_6k_and_writes_the_rows(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    res = {"metric": "preintegration windows/sec (50-sample windows)", "value": 7.1e8, "unit": "windows/s", "n_gpus": 1, "steps": 20, "warmup": 5,
           "ms_per_step": 0.014, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "v1_mean: 10000 windows x 50 samples per GPU per step, CPI model 1, mean-only (BASELINE.json configs[1])",
                      "pool_batches": 12, "clock_preramp_ms": 60.0, "library_build": "0123456789abcdef", "launch_mode": "g" * 80, "parallelism": "1 GPU"},
           "roofline": bench.roofline_of("v1_mean", 10000, 50, 12.4e-6, {}, "no pmc"), "goal_40pct_hbm": False, "goal_note": "n" * 250,
           "overlapped": {"contexts": 3, "value": 1.2e9, "unit": "windows/s", "ms_per_batch": 0.0084, "frac": 0.437, "batches": 3000,
                          "frac_by_contexts": {"2": 0.4012, "3": 0.4371, "4": 0.4402}, "how": "h" * 170}, "goal_40pct_hbm_overlapped": True,
           "cpu_baseline": dict(_row("v1_mean", 10000)["cpu_baseline"], sample="s" * 200,
                                sparse_port={"value": 3.2e6, "unit": "windows/s", "cores": 16, "kind": "port", "single_core_value": 2.1e5, "what": "w" * 60, "sample": "p" * 90})}
    extra = [_row(name, W, N=(rest[0] if rest else None)) for name, W, _, *rest in bench.EXTRA_ROWS]
    extra[4]["roofline"]["fp64"] = {"TFLOPs": 31.6, "peak": 78.6, "frac": 0.40, "source": "counters", "useful_frac": 0.34}
    extra.append({"workload": "v1_mean_3ctx", "units_per_step": 10000, "value": 1.2e9, "unit": "windows/s", "contexts": 3, "us_per_batch": 8.4,
                  "hbm_GBs": 3500.0, "hbm_frac": 0.437, "note": "n" * 120})
    extra.append({"workload": "broken", "units_per_step": 5, "error": "RuntimeError('x')"})
    bench.emit(res, extra)
    out = capsys.readouterr().out
    line = out.strip().splitlines()[-1]
    assert len(line) < 5700, len(line)       # head-room under the driver's 6 KB
    r = json.loads(line)
    assert r["value"] == 7.1e8 and r["roofline"]["frac"] > 0 and r["cpu_baseline"]["cores"] == 16
    assert r["configs2"]["value"] > 0 and r["configs2"]["fp64"]["useful_frac"] == 0.34 and r["configs2"]["cpu_baseline"]["kind"] == "reference"
    assert len(r["extra_rows"]) == len(extra) and r["extra_rows"]["broken@5"] == "error"
    # the short-window rows (the reference's own window lengths) are keyed apart from the 50-sample rows of the same workload
    assert "v1_mean@1M" in r["extra_rows"] and "v1_mean@1Mx10" in r["extra_rows"] and "v1_mean@1Mx20" in r["extra_rows"] and "v1_mean@30k" in r["extra_rows"]
    assert r["value_full_integrator"] == r["configs2"]["value"]
    assert r["routes_1M_x_50"]["dense_kernel_preassembled"] > 0
    assert r["overlapped"]["frac"] == 0.437 and r["goal_40pct_hbm_overlapped"] is True
    doc = json.load(open(tmp_path / "bench_extra.json"))
    assert len(doc["rows"]) == len(extra) and doc["headline"]["value"] == 7.1e8 and "extra_rows" not in doc["headline"]


def test_emit_without_extra_rows_is_the_plain_headline(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit({"metric": "m", "value": 1.0}, None)
    assert json.loads(capsys.readouterr().out.strip()) == {"metric": "m", "value": 1.0}
    assert not (tmp_path / "bench_extra.json").exists()


def test_link_types_are_parsed_from_rocm_smi_text():
    one = """============================ ROCm System Management Interface ============================
=============================== Link Type between two GPUs ===============================
       GPU0         
GPU0   0            
================================== End of ROCm SMI Log ==================================="""
    assert bench.parse_link_types(one) == {"GPU0": {}}
    four = """=============================== Link Type between two GPUs ===============================
       GPU0         GPU1         GPU2         GPU3         
GPU0   0            XGMI         XGMI         PCIE         
GPU1   XGMI         0            XGMI         XGMI         
GPU2   XGMI         XGMI         0            XGMI         
GPU3   PCIE         XGMI         XGMI         0            
"""
    lt = bench.parse_link_types(four)
    assert lt["GPU0"] == {"GPU1": "XGMI", "GPU2": "XGMI", "GPU3": "PCIE"} and lt["GPU3"]["GPU0"] == "PCIE" and len(lt) == 4
    assert bench.parse_link_types("WARNING: No JSON data to report") == {}


def test_every_global_name_bench_py_uses_is_defined():
    """A refactoring slip once deleted a helper that only the N > 1 path calls (found by the GPU rehearsals, not here): every global
    name loaded anywhere in bench.py must be a builtin, an import or a module-level definition."""
    import ast
    import builtins
    src = open(bench.__file__).read()
    tree = ast.parse(src)
    defined = set(dir(builtins)) | set(vars(bench))
    local_scopes = set()
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.Lambda)):
            a = node.args
            local_scopes.update(x.arg for x in a.args + a.kwonlyargs + ([a.vararg] if a.vararg else []) + ([a.kwarg] if a.kwarg else []))
        if isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
            local_scopes.add(node.id)
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            local_scopes.update((al.asname or al.name).split(".")[0] for al in node.names)
        if isinstance(node, ast.ExceptHandler) and node.name:
            local_scopes.add(node.name)
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            local_scopes.add(node.name)
    missing = sorted({n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)} - defined - local_scopes)
    assert not missing, missing


def test_parse_keeps_a_plain_run_plain():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    a = bench.parse(["--steps", "7", "--full", "--no-cpu", "--dump-outputs", "d"])
    assert a.full and a.no_cpu and not a.no_extra and a.dump_outputs == "d"


def test_dump_outputs_whole_or_a_fixed_sample_of_rows(tmp_path):
    """--dump-outputs: float64 .npy files named after the outputs; beyond the size limit the SAME seeded rows of every array, in
    ascending order, and the same rows on every call."""
    import os

    import numpy as np
    import torch
    W = 1000
    arrays = {"DT": torch.arange(W, dtype=torch.float64), "alpha": torch.arange(3 * W, dtype=torch.float64).view(W, 3) * 0.5,
              "q": torch.arange(4 * W, dtype=torch.float32).view(W, 4)}
    assert bench.dump_outputs(arrays, str(tmp_path / "whole")) == W
    got = {f[:-4]: np.load(str(tmp_path / "whole" / f)) for f in os.listdir(str(tmp_path / "whole"))}
    assert set(got) == set(arrays)
    for k, v in arrays.items():
        assert got[k].dtype == np.float64 and np.array_equal(got[k], v.double().numpy()), k
    limit = 20000
    for d in ("s1", "s2"):
        keep = bench.dump_outputs(arrays, str(tmp_path / d), limit=limit)
        assert 0 < keep < W
        assert sum(os.path.getsize(str(tmp_path / d / f)) for f in os.listdir(str(tmp_path / d))) <= limit
    s1 = {f[:-4]: np.load(str(tmp_path / "s1" / f)) for f in os.listdir(str(tmp_path / "s1"))}
    s2 = {f[:-4]: np.load(str(tmp_path / "s2" / f)) for f in os.listdir(str(tmp_path / "s2"))}
    rows = s1["DT"].astype(np.int64)
    assert len(rows) == keep and (np.diff(rows) > 0).all()
    assert np.array_equal(s1["alpha"], arrays["alpha"].numpy()[rows]) and np.array_equal(s1["q"], arrays["q"].double().numpy()[rows])
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
