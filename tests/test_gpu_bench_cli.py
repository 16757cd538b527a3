"""bench.py on one GPU, the plain run: `--steps` sets the number of timed steps, the line carries the headline
figure and `ms_per_step` and none of the measurements that `--full` adds, and `--dump-outputs` writes what the last
timed step computed (tiny model: the run is about the script, not the number)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("sustained", "roofline", "ttft_ms_p50", "batch_sweep_tokens_per_s", "other_configs", "cpu_baseline",
             "process_group_path")


def test_plain_run_is_lean_and_dumps_its_last_step(gpu_device, tmp_path):
    steps, warmup, batch = 5, 2, 4
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup), "--model", "tiny", "--batch", str(batch), "--context", "40",
                          "--dump-outputs", str(tmp_path / "dump")], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["value"] > 0 and out["unit"] == "tokens/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and abs(out["value"] - batch / out["ms_per_step"] * 1e3) <= 0.01 * out["value"]
    # every timed step appends one token: the context the last one attended to is steps - 1 beyond the first one's
    first, last = out["config"]["context_len_timed_steps"]
    assert last - first == steps - 1
    assert not [k for k in FULL_ONLY if k in out]
    tok = np.load(tmp_path / "dump" / "next_tokens.npy")
    kv = np.load(tmp_path / "dump" / "kv_last_step.npy")
    assert tok.dtype == np.float32 and tok.shape == (batch, )
    assert np.all(tok == np.floor(tok)) and tok.min() >= 0 and tok.max() < 2048      # TINY's vocabulary
    # TINY: 2 layers, K and V, every sequence of this small batch, one block of 16 slots x 2 KV heads x 64
    assert kv.dtype == np.float32 and kv.shape == (2, 2, batch, 16 * 2 * 64)
    assert np.isfinite(kv).all() and np.abs(kv).max() > 0
    assert tok.nbytes + kv.nbytes <= 64 << 20
