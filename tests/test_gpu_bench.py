"""A plain bench.py run on the GPU: its result line, and its --dump-outputs files against the operator on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import torch

    import bench
    import flash_attention_metal_amd as fa

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 7 and res["warmup"] == 2 and res["unit"] == "TFLOP/s" and res["dtype"] == "bf16"
    assert res["higher_is_better"] is True and res["value"] > 0 and res["ms_per_step"] > 0
    # what moved behind --full stays out of a plain run
    assert not {"value_public_api", "c4_slice", "c5_fp8", "sweep", "cpu_baseline"} & set(res)

    # the dump is what the operator returns for the benchmark's inputs
    dev = torch.device("cuda", 0)
    q, k, v = bench.workload_qkv(torch, dev, bench.B_PER_GPU * bench.H, 0)
    o, lse = fa.flash_attention_forward(q, k, v, is_causal=bench.CAUSAL)
    torch.cuda.synchronize()
    lse_d = np.load(tmp_path / "lse.npy")
    o_d = np.load(tmp_path / "o_rows_sample.npy")
    assert lse_d.dtype == np.float32 and o_d.dtype == np.float32
    assert np.array_equal(lse_d, lse.cpu().numpy())
    rows = o.reshape(-1, bench.D).float().cpu().numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(rows.shape[0], size=bench.DUMP_ROWS, replace=False))
    assert np.array_equal(o_d, rows[idx])
