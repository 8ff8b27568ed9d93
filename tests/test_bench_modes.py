"""bench.py's two modes: a plain run prints the headline line only; `--full` adds the per-kernel rooflines, the CPU oracle
baseline, parity against it and the fp16 legs.  The GPU tests run the benchmark at a small shape."""
import json
import math
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "2", "--height", "256", "--width", "256", "--frames", "5"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "rooflines", "step_mfma_frac", "kernel_ms_per_step", "cpu_baseline", "parity", "fp16_build",
             "fp16_split_trunk_build", "at_tolerance")


def test_full_is_off_by_default():
    assert bench.parse([]).full is False
    assert bench.parse(["--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse(["--full", "--no-fp16-leg"]).full is True


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _check_headline(out):
    assert all(k in out for k in HEADLINE), out
    assert out["unit"] == "steps/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 2 and out["finite"]
    assert out["value"] > 0 and math.isclose(out["value"], 1e3 / out["ms_per_step"], rel_tol=1e-2)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(hip_lib):
    out = _run()
    _check_headline(out)
    assert not [k for k in FULL_ONLY if k in out], out


@pytest.mark.gpu
def test_full_run_adds_kernel_figures_and_oracle_legs(hip_lib):
    out = _run("--full", "--cpu-threads", "16")
    _check_headline(out)
    assert out["rooflines"] and out["roofline"]["kernel"] in out["rooflines"] and out["kernel_ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["cores"] == 16
    for leg in (out, out["fp16_build"], out["fp16_split_trunk_build"]):
        assert math.isfinite(leg["parity"]["rel_l2"]) and leg["parity"]["tolerance"] > 0
    assert out["fp16_build"]["value"] > 0 and out["fp16_split_trunk_build"]["value"] > 0
    assert "at_tolerance" in out
