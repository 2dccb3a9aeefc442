"""bench.py's options that need no GPU: the step-count check and the --dump-outputs writer -- CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=60)


def test_help_lists_full_and_dump_outputs():
    r = run_bench("--help")
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked_before_any_work(args):
    r = run_bench("--gpus", "1", *args)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_fixed_sample_under_64_mb(tmp_path):
    import torch

    import bench

    g = torch.Generator().manual_seed(5)
    o = torch.rand(1, bench.B_PER_GPU * bench.H, bench.N, bench.D, generator=g).to(torch.bfloat16)
    lse = torch.rand(1, bench.B_PER_GPU * bench.H, bench.N, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), torch, o, lse)
    bench.dump_outputs(str(tmp_path / "b"), torch, o, lse)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["lse.npy", "o_rows_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 2 ** 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)  # the same rows in every run
    assert np.array_equal(np.load(tmp_path / "a" / "lse.npy"), lse.numpy())
    sample = np.load(tmp_path / "a" / "o_rows_sample.npy")
    rows = o.reshape(-1, bench.D).float().numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(rows.shape[0], size=bench.DUMP_ROWS, replace=False))
    assert sample.shape == (bench.DUMP_ROWS, bench.D) and np.array_equal(sample, rows[idx])
