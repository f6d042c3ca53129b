"""CPU-side smoke of the bench.py contract: the driver runs
`python bench.py ...` at round end — a broken import/flag surface there is
a silent zero, so exercise the CPU-reachable legs here."""

import json
import os
import subprocess
import sys

import pytest


def test_cpu_baseline_only_runs(repo_root):
    """`--cpu-baseline-only` runs the full configs[0]-shaped loop (at the 2m
    shape for speed) and prints one JSON object with the contract keys."""
    r = subprocess.run(
        [sys.executable, "bench.py", "--cpu-baseline-only", "--model", "llama-2m",
         "--seq", "128"],
        cwd=repo_root, capture_output=True, text=True, timeout=600,
        env={**os.environ, "OMP_NUM_THREADS": "4"})
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "tokens/s"
    assert line["kind"] == "port"
    assert line["cores"] > 0
    assert line["value"] > 0
    assert "outer" in line["sample"]  # the timed region includes the outer block


def test_bench_requires_gpu_for_training_leg(repo_root):
    """Without a GPU the training leg must fail loudly (no CPU fallback on
    the product path), not silently measure something else."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "1", "--warmup", "0",
         "--no-cpu-baseline"],
        cwd=repo_root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "needs a GPU" in (r.stdout + r.stderr)


def test_bench_rejects_zero_steps(repo_root):
    """`--steps` is the exact timed-step count; zero timed steps has no
    last step to report and no rate, so it is refused up front."""
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "0", "--no-cpu-baseline"],
        cwd=repo_root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--steps must be >= 1" in r.stderr


def test_dump_outputs_sample_is_fixed_and_capped(repo_root, tmp_path):
    """`--dump-outputs` writes float32 arrays within the 64 MB cap; a
    parameter buffer larger than the sample size is sampled at the same
    indices on every call, so two runs compare element for element."""
    import numpy as np
    import torch

    import bench

    n = bench.DUMP_PARAM_SAMPLES + 12345
    flat = torch.arange(n, dtype=torch.float32)
    losses = [torch.tensor(2.5), torch.tensor(3.5)]
    norm = torch.tensor(0.75)
    bench._dump_outputs(str(tmp_path / "a"), losses, norm, flat)
    bench._dump_outputs(str(tmp_path / "b"), losses, norm, flat)

    total = 0
    for name in ("loss", "grad_norm", "params"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        b = np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [2.5, 3.5]
    assert np.load(tmp_path / "a" / "grad_norm.npy").tolist() == [0.75]
    params = np.load(tmp_path / "a" / "params.npy")
    assert params.shape == (bench.DUMP_PARAM_SAMPLES,)
    # values are the sampled indices here: sorted, in range
    assert np.all(np.diff(params) >= 0) and params[-1] < n

    small = torch.arange(10, dtype=torch.float32)
    bench._dump_outputs(str(tmp_path / "c"), losses, norm, small)
    assert np.array_equal(np.load(tmp_path / "c" / "params.npy"), small.numpy())
