"""GPU leg of the bench.py contract: `--dump-outputs` writes what the timed
step computed, and identical arguments give identical seeded inputs (so the
outputs of two runs agree)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


def _bench(repo_root, out_dir):
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
         "--model", "llama-2m", "--batch", "16", "--per-device", "8", "--seq", "128",
         "--no-cpu-baseline", "--no-roofline", "--dump-outputs", str(out_dir)],
        cwd=repo_root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return {name: np.load(os.path.join(out_dir, f"{name}.npy"))
            for name in ("loss", "grad_norm", "params")}


@requires_gpu
def test_bench_dump_outputs_reproducible(repo_root, tmp_path):
    a = _bench(repo_root, tmp_path / "a")
    b = _bench(repo_root, tmp_path / "b")
    assert a["loss"].shape == (2,)  # one per micro-batch (16 / 8)
    assert a["grad_norm"].shape == (1,)
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.all(np.isfinite(a["loss"])) and np.all(a["loss"] > 0)
    # loss of a near-uniform 1024-way prediction after three small steps
    assert np.all(np.abs(a["loss"] - np.log(1024)) < 0.5), a["loss"]
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-5, atol=1e-7, err_msg=name)
