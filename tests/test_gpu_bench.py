"""bench.py end to end on an MI355X: the JSON result line must come out for a plain run (headline fields only, and
the same --dump-outputs arrays from run to run), and under --full for the default configuration (C3, with the exact-fp32
parity leg) and for the chain configuration (C2), with the objects the contract names.

Schema and internal consistency only.  Throughput is what bench.py REPORTS, never what a correctness suite asserts: a
3-step run on a box that has just been leased measures the cold start, not the kernels (round 2's driver run: 317 858
samples/s here against 5.93 M in the driver's own bench), and these tests are collected LAST (conftest.py) so that
nothing end-to-end can stand in front of the parity tests under `pytest -x`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", *flags],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    print("bench line:", d["ms_per_step"], "ms/step; enqueue", d["host_enqueue_ms_per_step"], d.get("host_enqueue_done_ms_first_steps"),
          "ramp", d.get("ramp_up_step_ms"))
    return d, lines[0]


def test_default_bench_line_c3_with_fp32_parity_leg():
    d, line = _run("--full")                       # the full line, fewer steps; cpu_baseline on a bounded sample
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "bf16" and d["higher_is_better"] is True, line
    assert d["unit"] == "samples/s" and d["value"] > 0 and d["vs_baseline"] is None and d["full"] is True, line
    assert abs(d["value"] - 8192 * 3 / (d["ms_per_step"] * 3e-3)) <= 1e-6 * d["value"], line
    assert d["warmup"] >= 1 and d["warmup_effective"] >= d["warmup"], line
    assert d["step_path"] == "layers" and d["config"]["global_batch"] == 8192, line
    assert "workload" in d["config"] and "model" not in d["config"], line
    r = d["roofline"]
    assert r["bound"] == "mfma" and 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9, line
    by = r["by_kernel"]
    assert {"gemm_fwd", "gemm_dgrad", "gemm_wgrad", "loss", "adam"} <= set(by), line
    # the kernel the roofline is quoted on is the class with the largest share of the step among the GEMM classes
    gemm = [k for k in by if k.startswith("gemm_")]
    assert r["kernel"] == max(gemm, key=lambda k: by[k]["ms_per_step"]), line
    assert by[r["kernel"]]["sampled_steps"] >= 3, line
    rs = d["roofline_step"]
    assert rs["bound"] == "mfma" and abs(rs["frac"] - rs["achieved"] / rs["peak"]) < 1e-9 and 0.0 < rs["frac"] < 1.0, line
    f = d["f32_parity"]
    assert f["ms_per_step"] > 0 and f["steps"] == 10 and abs(f["samples_per_s"] - 8192 / (f["ms_per_step"] * 1e-3)) <= 1e-6 * f["samples_per_s"], line
    assert abs(f["frac"] - f["tflops"] / f["roofline_tflops"]) < 1e-9 and f["roofline_tflops"] in (157.3, 2500.0 / 6.0), line
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1, line
    # thread pools capped at the container's CPU quota before the timed region (codae/hostcpu.py): the baseline ran on that many
    assert d["host_cpu_share"] >= 1 and d["host_threads"] <= d["host_cpu_share"] and c["cores"] <= d["host_cpu_share"], line


def test_bench_line_c2_takes_the_chain():
    d, line = _run("--full", "--config", "c2", "--no-f32-parity", "--no-cpu-baseline")
    assert d["step_path"] == "chain" and d["config"]["global_batch"] == 1024, line
    assert "chain" in d["roofline"]["by_kernel"] and d["value"] > 0, line
    assert d["roofline"]["bound"] == "hbm", line


def test_plain_bench_line_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    import numpy as np
    runs = []
    for name in ("a", "b"):
        d, line = _run("--dump-outputs", str(tmp_path / name))
        assert d["metric"] == "training samples/sec at 3x512-dim input, batch 8192" and d["unit"] == "samples/s", line
        assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "bf16" and d["higher_is_better"] is True, line
        assert d["value"] > 0 and abs(d["value"] - 8192 * 3 / (d["ms_per_step"] * 3e-3)) <= 1e-6 * d["value"], line
        # what only --full measures is not measured
        assert d["full"] is False and d["f32_parity"] is None and d["roofline"] is None and d["cpu_baseline"] is None, line
        arrays = {}
        for f in sorted(os.listdir(tmp_path / name)):
            a = np.load(tmp_path / name / f)
            assert f.endswith(".npy") and a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
            arrays[f[:-4]] = a
        assert sorted(arrays) == sorted(d["dumped_outputs"]["arrays"]), line
        assert {"loss", "grad_norm", "metric_sums", "weights_sample", "biases"} <= set(arrays), sorted(arrays)
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays["loss"][0] == d["final_loss"] and arrays["grad_norm"][0] == d["final_grad_norm"], line
        assert arrays["biases"].shape == (10, 1536) and arrays["weights_sample"].shape[0] == 10
        runs.append(arrays)
    # same arguments, same inputs, same bits: the untimed extra warm-up is rolled back, and the step's only atomics are
    # fp64 additions of fp32 partial sums into the scalars block (loss, metric sums, sum g^2), which come out the same in
    # any order in practice (53-bit sums of 24-bit terms) - the same ground DESIGN.md's determinism rests on
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
