"""What the visit-count policy target costs at the headline shape (19x19, K = 256, 20 blocks, 512 games, Winograd fp16x2, Budget 800).

ONE arena plays whole moves; agz_arena_set_policy_target is switched between moves, AGZ_TARGET_REFERENCE (off: the parent's code path,
the baseline) and AGZ_TARGET_VISITS (on; temperature 1 by default) in the order A B B A A B B A ... so that the slow growth of the trees
from move to move weighs on both arms alike.  Reported per arm:
  * whole-move sims/s (begin_move + Budget simulation steps + end_move, wall clock between two fences; timing only AGZ_PROF_MOVE keeps
    the step on the path it takes without a profiler: the split step at this shape),
  * the AGZ_PROF_MOVE class time per move from the kernel-class timers, recorded on the same moves: k_begin_move + k_end_move — the
    kind adds no launch, k_end_move writes another row — and
  * the example rows the move recorded.
A first move (off) from the openings is played untimed: it evaluates every root and grows the pools.
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import agogo_amd as A
from agogo_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=512)
ap.add_argument("--size", type=int, default=19)
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--L", type=int, default=20)
ap.add_argument("--budget", type=int, default=800)
ap.add_argument("--moves", type=int, default=8, help="timed whole moves, half per arm (a multiple of 4 keeps A B B A balanced)")
ap.add_argument("--temperature", type=float, default=1.0)
args = ap.parse_args()
S, G, B = args.size, args.games, args.budget

ctx = A.Ctx(0)
net = A.Net(ctx, args.K, args.L, 2 * args.K, S, S, 18, S * S + 1, bn_mode=capi.BN_IDENTITY)
net.init_random(1337)
for i in range(net.num_params()):
    name, n = net.param_info(i)
    if name.endswith("_gamma"):
        net.set_param(i, np.ones(n, np.float32))
    elif name.endswith("_beta"):
        net.set_param(i, np.zeros(n, np.float32))
net.commit()
net.set_compute_mode(capi.COMPUTE_WINO_H2)
arena = A.Arena(ctx, capi.GAME_WQ, S, S, komi=7.5, encoder=capi.ENC_WQ, n_games=G, seed=1337, Budget=B)
arena.set_inferencer(0, capi.INF_NET, net)
arena.set_inferencer(1, capi.INF_NET, net)
arena.reset()
arena.random_moves(np.random.default_rng(1337).integers(0, int(0.6 * S * S) + 1, size=G).astype(np.int32), 1337)

ARMS = ("off", "on")


def whole_move(arm, prof=True):
    arena.set_policy_target(capi.TARGET_VISITS if arm == "on" else capi.TARGET_REFERENCE, args.temperature)
    if prof:
        ctx.prof_enable(True, classes=[capi.PROF_MOVE])
    ctx.sync()
    s0, t0 = arena.stats(), time.perf_counter()
    arena.begin_move()
    for _ in range(B):
        arena.simulate(1)
    arena.end_move(True)
    ctx.sync()
    dt = time.perf_counter() - t0
    s1 = arena.stats()
    out = {"arm": arm, "seconds": dt, "sims_per_s": (s1["sims_nonnull"] - s0["sims_nonnull"]) / dt, "split_steps": arena.split_steps()[0],
           "rows": s1["examples"] - s0["examples"]}
    if prof:
        ctx.prof_enable(False)
        launches, ms = ctx.prof_read(capi.PROF_MOVE)
        out.update(move_class_launches=launches, move_class_us=1e3 * ms)
    return out


def order(n):
    return [("off", "on", "on", "off")[i % 4] for i in range(n)]


whole_move("off", prof=False)                       # untimed: every root evaluated, pools grown
runs = [whole_move(arm) for arm in order(args.moves)]
out = {"shape": {"size": S, "games": G, "K": args.K, "L": args.L, "budget": B}, "temperature": args.temperature, "moves": runs}
for arm in ARMS:
    v = [r["sims_per_s"] for r in runs if r["arm"] == arm]
    u = [r["move_class_us"] for r in runs if r["arm"] == arm]
    out[arm] = {"sims_per_s_mean": float(np.mean(v)), "sims_per_s_min": float(np.min(v)), "sims_per_s_max": float(np.max(v)),
                "move_class_us_per_move": float(np.mean(u)), "move_class_launches_per_move": float(np.mean([r["move_class_launches"] for r in runs if r["arm"] == arm])),
                "rows_per_move": float(np.mean([r["rows"] for r in runs if r["arm"] == arm]))}
print(json.dumps(out))
arena.close()
net.close()
ctx.close()
