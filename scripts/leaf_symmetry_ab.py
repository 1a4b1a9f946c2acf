"""What AGZ_SYM_RANDOM costs at the headline shape (19x19, K = 256, 20 blocks, 512 games, Winograd fp16x2, Budget 800).

ONE arena plays whole moves; the leaf symmetry is switched between moves, OFF and AGZ_SYM_RANDOM in the order A B B A A B B A ...
so that the slow growth of the trees from move to move weighs on both arms alike.  Reported per arm:
  * whole-move sims/s (begin_move + Budget simulation steps + end_move, wall clock between two fences; the step takes whatever path it
    takes without a profiler: the split step at this shape), and
  * per-step k_select / k_expand time from the kernel-class timers (AGZ_PROF_SELECT / AGZ_PROF_EXPAND), on moves of their own: timing
    those classes puts the step on the joined path, so these moves are not part of the sims/s figure.
A first move (OFF) from the openings is played untimed: it evaluates every root and grows the pools.
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
ap.add_argument("--prof-moves", type=int, default=4, help="extra moves with the select / expand timers on, half per arm")
ap.add_argument("--seed", type=int, default=0x5EED5EED5EED)
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

ARMS = {"off": capi.SYM_OFF, "random": capi.SYM_RANDOM}


def whole_move(arm):
    arena.set_leaf_symmetry(ARMS[arm], args.seed)
    ctx.sync()
    s0, t0 = arena.stats(), time.perf_counter()
    arena.begin_move()
    for _ in range(B):
        arena.simulate(1)
    arena.end_move(True)
    ctx.sync()
    dt = time.perf_counter() - t0
    s1 = arena.stats()
    return {"arm": arm, "seconds": dt, "sims_per_s": (s1["sims_nonnull"] - s0["sims_nonnull"]) / dt, "split_steps": arena.split_steps()[0]}


def order(n):
    return [("off", "random", "random", "off")[i % 4] for i in range(n)]


whole_move("off")                                   # untimed: every root evaluated, pools grown
runs = [whole_move(arm) for arm in order(args.moves)]
prof = []
for arm in order(args.prof_moves):
    ctx.prof_enable(True, classes=[capi.PROF_SELECT, capi.PROF_EXPAND])
    whole_move(arm)
    ctx.prof_enable(False)
    (sn, sms), (en, ems) = ctx.prof_read(capi.PROF_SELECT), ctx.prof_read(capi.PROF_EXPAND)
    prof.append({"arm": arm, "select_launch_groups": sn, "select_us_per_step": 1e3 * sms / max(1, sn),
                 "expand_launch_groups": en, "expand_us_per_step": 1e3 * ems / max(1, en)})
out = {"shape": {"size": S, "games": G, "K": args.K, "L": args.L, "budget": B}, "moves": runs, "profiled_moves": prof}
for arm in ARMS:
    v = [r["sims_per_s"] for r in runs if r["arm"] == arm]
    out[arm] = {"sims_per_s_mean": float(np.mean(v)), "sims_per_s_min": float(np.min(v)), "sims_per_s_max": float(np.max(v)),
                "select_us_per_step": float(np.mean([p["select_us_per_step"] for p in prof if p["arm"] == arm])) if prof else None,
                "expand_us_per_step": float(np.mean([p["expand_us_per_step"] for p in prof if p["arm"] == arm])) if prof else None}
print(json.dumps(out))
arena.close()
net.close()
ctx.close()
