"""What a training step sampled from a replay window costs on the G19 trainer shape (19x19, K = 256, 20 blocks, BatchSize 256,
AGZ_COMPUTE_WINO_H2), against a batch of agz_train_dev over the same number of rows resident in HBM.

One process times ONE arm, so that an A/B alternates whole processes (and, for the parent commit's arm, whole trees):
  --arm dev      agz_examples_prepare + agz_train_dev(batches, iterations = 1): ms per batch — the arm that also runs on a tree without
                 the replay window
  --arm replay   a window of batches * 256 rows filled with agz_replay_append_examples, agz_train_replay(steps = batches, symmetric on):
                 ms per step
Two warm-up batches / steps, then the timed call between two context synchronisations.  Prints one line: <arm> <ms>.  The sampler's own
kernel time comes from running the replay arm under `rocprofv3 --kernel-trace --stats`.  Figures: profiles/replay.md."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import agogo_amd as A
from agogo_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--arm", choices=["dev", "replay"], required=True)
ap.add_argument("--batches", type=int, default=16, help="batches / steps timed; the window holds batches * 256 rows")
ap.add_argument("--symmetric", type=int, default=1)
args = ap.parse_args()

S, K, L, B, N = 19, 256, 20, 256, args.batches
ctx = A.Ctx(0)
t = A.Trainer(ctx, K, L, 2 * K, S, S, 18, S * S + 1, B)
t.init_random(1337)
t.set_compute_mode(capi.COMPUTE_WINO_H2)
rng = np.random.default_rng(0)
x = rng.choice(np.array([-1, 0, 1], np.float32), size=(B, 18, S, S)).astype(np.float32)
pi = np.zeros((B, S * S + 1), np.float32)
pi[np.arange(B), rng.integers(0, S * S + 1, B)] = 1
v = rng.choice(np.array([-1, 0, 1], np.float32), size=B).astype(np.float32)
ex = A.Examples(ctx, 18, S, S, S * S + 1)
for _ in range(N):
    ex.append_host(x, pi, v)
if args.arm == "dev":
    nb = ex.prepare(B, 0, seed=1)
    xd, pd, vd, rows_d, bd = ex.tensors_dev()
    assert bd == N
    t.train_dev(xd, pd, vd, 2, 1, seed=3)
    ctx.sync()
    t0 = time.perf_counter()
    t.train_dev(xd, pd, vd, bd, 1, seed=3)
    ctx.sync()
else:
    rp = A.Replay(ctx, 18, S, S, S * S + 1, N * B)
    rp.append_examples(ex)
    assert len(rp) == N * B
    t.train_replay(rp, 2, 3, bool(args.symmetric))
    ctx.sync()
    t0 = time.perf_counter()
    t.train_replay(rp, N, 3, bool(args.symmetric))
    ctx.sync()
print("%s %.4f" % (args.arm, (time.perf_counter() - t0) / N * 1e3), flush=True)
