"""What playout cap randomization gives at the headline shape (19x19, K = 256, 20 blocks, 512 games, Winograd fp16x2, Budget 800).

ONE arena plays whole moves; agz_arena_set_playout_cap is switched between moves: off (the parent's code path, the baseline), on
(p_full 0.25, fast_budget 100 by default) and, for --whole moves at the end, on with the tail compaction off (agz_arena_set_cap_compact(0):
the tail steps on the whole 512-board batch with the fast games idle), in the order off, on, on, off, ... so that the slow growth of the
trees weighs on both arms alike.  Reported per move and per arm:
  * seconds per whole move (begin_move + Budget simulation steps + end_move, wall clock between two fences) and moves/s (games x moves),
  * the example rows the move recorded and rows/s,
  * the number of FULL games and the network batch nb of the tail steps (agz_arena_last_cap_batch),
  * the seconds of the head (the first fast_budget steps, every game searching) and of the tail (the remaining steps), each between
    fences of its own, and from them the time of one head step and of one tail step at that nb.
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
ap.add_argument("--fast", type=int, default=100)
ap.add_argument("--p-full", type=float, default=0.25)
ap.add_argument("--moves", type=int, default=8, help="timed whole moves, half per arm (a multiple of 4 keeps off on on off balanced)")
ap.add_argument("--whole", type=int, default=2, help="further on-moves with the tail compaction off")
args = ap.parse_args()
S, G, B, F = args.size, args.games, args.budget, args.fast

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


def whole_move(arm):
    on = arm != "off"
    arena.set_playout_cap(args.p_full, F, on=on, seed=1337)
    arena.set_cap_compact(arm != "on_whole")
    ctx.sync()
    s0, t0 = arena.stats(), time.perf_counter()
    arena.begin_move()
    for _ in range(F):
        arena.simulate(1)
    ctx.sync()
    t1 = time.perf_counter()
    for _ in range(B - F):
        arena.simulate(1)
    nb, n_full = arena.last_cap_batch()
    ctx.sync()
    t2 = time.perf_counter()
    arena.end_move(True)
    ctx.sync()
    t3 = time.perf_counter()
    s1 = arena.stats()
    dt = t3 - t0
    live = s1["moves_played"] - s0["moves_played"]
    return {"arm": arm, "seconds": dt, "moves_per_s": live / dt, "rows": s1["examples"] - s0["examples"], "rows_per_s": (s1["examples"] - s0["examples"]) / dt,
            "sims": s1["sims_total"] - s0["sims_total"], "full_games": n_full if on else live, "tail_batch": nb if on else G,
            "head_seconds": t1 - t0, "head_ms_per_step": 1e3 * (t1 - t0) / F, "tail_seconds": t2 - t1, "tail_ms_per_step": 1e3 * (t2 - t1) / (B - F)}


def order(n):
    return [("off", "on", "on", "off")[i % 4] for i in range(n)]


whole_move("off")                                   # untimed: every root evaluated, pools grown
runs = [whole_move(arm) for arm in order(args.moves)] + [whole_move("on_whole") for _ in range(args.whole)]
out = {"shape": {"size": S, "games": G, "K": args.K, "L": args.L, "budget": B}, "p_full": args.p_full, "fast_budget": F, "moves": runs}
for arm in ("off", "on", "on_whole"):
    rs = [r for r in runs if r["arm"] == arm]
    if not rs:
        continue
    out[arm] = {"moves": len(rs)}
    for key in ("seconds", "moves_per_s", "rows", "rows_per_s", "full_games", "tail_batch", "head_ms_per_step", "tail_ms_per_step"):
        v = [r[key] for r in rs]
        out[arm][key] = {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))}
print(json.dumps(out))
arena.close()
net.close()
ctx.close()
