"""bench.py as it is run for every change: a plain run (the headline only) and --dump-outputs, on the tiny configuration."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--config", "tiny",
           "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """the plain run prints the headline fields and nothing that --full measures; two runs with the same arguments dump the same outputs"""
    d = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 2 and len(d["turn_ms"]) == 3
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "action-steps/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]          # 4 actions per timed step
    for k in ("roofline", "roofline_prefill_gemm", "with_feature_cache", "fp8_decode_weights", "memory_prune_32", "batched_envs",
              "metric_allreduce_check"):
        assert d[k] is None, k
    assert "cpu_baseline" not in d
    _bench(tmp_path / "b")
    for name, dtype in (("sequences", np.float64), ("hidden", np.float32)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == dtype and a.size > 0 and np.isfinite(a).all(), name
        assert np.array_equal(a, b), name
    seq, hid = np.load(tmp_path / "a" / "sequences.npy"), np.load(tmp_path / "a" / "hidden.npy")
    assert seq.shape == (1, 5) and hid.shape[0] == seq.shape[1]     # 5 decode tokens per turn (no EOS in the bench), one hidden row each
