"""The sharded trainer's step (agz_trainer_create_sharded) against the plain agz_trainer_batch step at G19 (K=256, 20 blocks, 19x19, F=18,
A=362), AGZ_COMPUTE_WINO_H2, `--rows` rows per rank, in the same process, alternated A/B over --reps repeats of --steps steps each.
With one rank (the default; a real RCCL communicator over this GPU) the two compute the same step: the difference is what the sharded
form adds — 2 (L + 3) or so small all-gathers on the compute stream, the rank-order finalize kernels, one grouped all-reduce of the
shared gradients and the status word.  n > 1 over xGMI is not measured here.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import agogo_amd as A
from agogo_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--L", type=int, default=20)
ap.add_argument("--size", type=int, default=19)
ap.add_argument("--rows", type=int, default=256, help="rows per rank (the global batch is rows x ranks)")
ap.add_argument("--steps", type=int, default=5, help="steps per timed block")
ap.add_argument("--reps", type=int, default=6, help="alternated A/B blocks")
args = ap.parse_args()
S, K, L, B = args.size, args.K, args.L, args.rows
Aspace = S * S + 1
ctx = A.Ctx(0)
comm = A.Comm.init_all([ctx])[0]
plain = A.Trainer(ctx, K, L, 2 * K, S, S, 18, Aspace, B)
sharded = A.Trainer.sharded(ctx, comm, K, L, 2 * K, S, S, 18, Aspace, B * comm.size())
for t in (plain, sharded):
    t.init_random(1337)
    t.set_compute_mode(capi.COMPUTE_WINO_H2)
rng = np.random.default_rng(0)
x = rng.choice(np.array([-1, 0, 1], np.float32), size=(B, 18, S, S)).astype(np.float32)
pi = np.zeros((B, Aspace), np.float32)
pi[np.arange(B), rng.integers(0, Aspace, B)] = 1
v = rng.choice(np.array([-1, 0, 1], np.float32), size=B).astype(np.float32)
# the first steps: the same parameters, the same data -> the same cost (one rank: the same arithmetic)
c_plain, c_sharded = plain.batch(x, pi, v), sharded.batch(x, pi, v)


def block(t):
    t0 = time.perf_counter()
    for _ in range(args.steps):
        c = t.batch(x, pi, v)
    return (time.perf_counter() - t0) / args.steps * 1e3, c


ms_p, ms_s, over = [], [], []
for rep in range(args.reps):
    order = (plain, sharded) if rep % 2 == 0 else (sharded, plain)
    got = {}
    for t in order:
        got[id(t)] = block(t)[0]
    ms_p.append(got[id(plain)])
    ms_s.append(got[id(sharded)])
    over.append(100.0 * (got[id(sharded)] / got[id(plain)] - 1.0))
print(json.dumps({"bench": "train_sharded", "K": K, "L": L, "board": S, "rows_per_rank": B, "ranks": comm.size(), "steps": args.steps,
                  "reps": args.reps, "plain_step_ms": [round(m, 3) for m in ms_p], "sharded_step_ms": [round(m, 3) for m in ms_s],
                  "plain_median_ms": round(statistics.median(ms_p), 3), "sharded_median_ms": round(statistics.median(ms_s), 3),
                  "overhead_pct": [round(o, 2) for o in over], "overhead_median_pct": round(statistics.median(over), 2),
                  "overhead_min_pct": round(min(over), 2), "overhead_max_pct": round(max(over), 2),
                  "first_cost_plain": c_plain, "first_cost_sharded": c_sharded, "first_costs_equal": c_plain == c_sharded}))
for h in (sharded, plain, comm):
    h.close()
ctx.close()
