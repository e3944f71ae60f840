"""bench.py on the GPU: a plain run times exactly --steps steps once and prints the headline keys only; --dump-outputs
writes the last timed step's outputs, the same in a plain and a --full run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["action", "done", "log_prob", "next_obs", "obs", "reward", "value"]


def _bench(extra, out_dir):
    env = dict(os.environ); env.pop("WORLD_SIZE", None)
    # 70 steps: one full 64-step rollout chunk and a partial one, so the last step sits in a shorter chunk
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "70", "--warmup", "10", "--envs", "256",
           "--dump-outputs", str(out_dir)] + extra
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench([], tmp_path / "plain")
    full = _bench(["--full", "--no-cpu-baseline", "--no-sb3-path", "--no-large-batch"], tmp_path / "full")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain and k in full
    assert plain["steps"] == 70 and plain["repeats"] == 1 and "roofline" not in plain
    assert plain["value"] == pytest.approx(256 * 1e3 / plain["ms_per_step"], rel=1e-9)
    assert full["repeats"] >= 3 and full["roofline"]["kernel_ms"] > 0
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "full")) == [n + ".npy" for n in NAMES]
    for n in NAMES:
        a = np.load(tmp_path / "plain" / (n + ".npy")); b = np.load(tmp_path / "full" / (n + ".npy"))
        assert a.dtype == np.float32 and a.shape[0] == 256 and np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6, err_msg=n)
    obs = np.load(tmp_path / "plain" / "obs.npy"); nxt = np.load(tmp_path / "plain" / "next_obs.npy")
    assert obs.shape == nxt.shape and not np.array_equal(obs, nxt)
