"""GPU: bench.py's plain run and --dump-outputs on a small shape — the headline fields are there and nothing else runs (no roofline, no
legs, no CPU baseline: those are --full), --steps is the number of timed steps, and two runs with the same arguments write the same
arrays, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--games", "32", "--budget", "16", "--L", "2",
           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    pr = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in pr.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    la, lb = _run(a, 3), _run(b, 3)
    for d in (la, lb):
        assert d["metric"] == "mcts_sims_per_sec" and d["unit"] == "sims/s" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        # every game simulated once per timed step: value x the region's time = 32 games x 3 steps (null simulations aside)
        assert 0 < d["value"] * d["ms_per_step"] * d["steps"] * 1e-3 <= 32 * 3 + 0.5
        assert "roofline" not in d and "cpu_baseline" not in d and "other_compute_modes" not in d["extra"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "root_visits.npy" in names and "board.npy" in names
    total, differ = 0, []
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and y.dtype == np.float32, n
        if not np.array_equal(x, y):
            differ.append(n)
        total += os.path.getsize(a / n)
    assert not differ, "differ between two runs: %s" % differ
    assert total < 64 << 20
    visits = np.load(a / "root_visits.npy")
    assert visits.shape[:2] == (32, 2) and visits.sum() > 0
