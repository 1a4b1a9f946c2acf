"""What forced playouts and the pruned policy target cost at the headline shape (19x19, K = 256, 20 blocks, 512 games, Winograd fp16x2,
Budget 800).

ONE arena with AGZ_TARGET_VISITS plays whole moves; agz_arena_set_forced_playouts is switched between moves, off (the parent's code
path, the baseline) and on (k = 2, prune on by default) in the order A B B A A B B A ... so that the slow growth of the trees from move
to move weighs on both arms alike.  Reported per arm:
  * whole-move sims/s (begin_move + Budget simulation steps + end_move, wall clock between two fences; timing only AGZ_PROF_MOVE keeps
    the step on the path it takes without a profiler: the split step at this shape),
  * the AGZ_PROF_MOVE class time per move from the kernel-class timers, recorded on the same moves: k_begin_move + k_end_move — the
    setting adds no launch, k_end_move computes the pruned playouts before it writes the row —,
  * the nodes on a descent's path and the children Select read per simulation (agz_arena_stats): forcing widens the root, which changes
    the trees the step walks, and
  * from --prof-moves further moves per arm with AGZ_PROF_SELECT timed as well (the joined step: a profiled class keeps the step off the
    split path, so these moves are not in the sims/s figures): the time of one k_select launch.
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
ap.add_argument("--moves", type=int, default=4, help="timed whole moves, half per arm (a multiple of 4 keeps A B B A balanced)")
ap.add_argument("--prof-moves", type=int, default=2, help="further whole moves with k_select timed, half per arm")
ap.add_argument("--k", type=float, default=2.0)
ap.add_argument("--no-prune", action="store_true")
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
arena.set_policy_target(capi.TARGET_VISITS, 1.0)
arena.reset()
arena.random_moves(np.random.default_rng(1337).integers(0, int(0.6 * S * S) + 1, size=G).astype(np.int32), 1337)

ARMS = ("off", "on")


def whole_move(arm, classes=(capi.PROF_MOVE,)):
    arena.set_forced_playouts(args.k, on=(arm == "on"), prune=not args.no_prune)
    if classes:
        ctx.prof_enable(True, classes=list(classes))
    ctx.sync()
    s0, t0 = arena.stats(), time.perf_counter()
    arena.begin_move()
    for _ in range(B):
        arena.simulate(1)
    arena.end_move(True)
    ctx.sync()
    dt = time.perf_counter() - t0
    s1 = arena.stats()
    sims = s1["sims_nonnull"] - s0["sims_nonnull"]
    out = {"arm": arm, "seconds": dt, "sims_per_s": sims / dt, "split_steps": arena.split_steps()[0], "rows": s1["examples"] - s0["examples"],
           "path_nodes_per_sim": (s1["path_nodes"] - s0["path_nodes"]) / max(sims, 1), "children_read_per_sim": (s1["children_read"] - s0["children_read"]) / max(sims, 1)}
    if classes:
        ctx.prof_enable(False)
        for klass, name in ((capi.PROF_MOVE, "move"), (capi.PROF_SELECT, "select")):
            if klass in classes:
                launches, ms = ctx.prof_read(klass)
                out.update({name + "_class_launches": launches, name + "_class_us": 1e3 * ms})
    return out


def order(n):
    return [("off", "on", "on", "off")[i % 4] for i in range(n)]


def mean(rs, key):
    return float(np.mean([r[key] for r in rs]))


whole_move("off", classes=())                       # untimed: every root evaluated, pools grown
runs = [whole_move(arm) for arm in order(args.moves)]
prof = [whole_move(arm, classes=(capi.PROF_MOVE, capi.PROF_SELECT)) for arm in order(args.prof_moves)]
out = {"shape": {"size": S, "games": G, "K": args.K, "L": args.L, "budget": B}, "k": args.k, "prune": not args.no_prune, "moves": runs, "profiled_moves": prof}
for arm in ARMS:
    rs, ps = [r for r in runs if r["arm"] == arm], [r for r in prof if r["arm"] == arm]
    v = [r["sims_per_s"] for r in rs]
    out[arm] = {"sims_per_s_mean": float(np.mean(v)), "sims_per_s_min": float(np.min(v)), "sims_per_s_max": float(np.max(v)),
                "move_class_us_per_move": mean(rs, "move_class_us"), "move_class_launches_per_move": mean(rs, "move_class_launches"),
                "rows_per_move": mean(rs, "rows"), "path_nodes_per_sim": mean(rs, "path_nodes_per_sim"), "children_read_per_sim": mean(rs, "children_read_per_sim")}
    if ps:
        out[arm]["select_us_per_launch"] = float(np.sum([r["select_class_us"] for r in ps]) / np.sum([r["select_class_launches"] for r in ps]))
        out[arm]["profiled_sims_per_s"] = mean(ps, "sims_per_s")
out["on_over_off_sims_per_s"] = out["on"]["sims_per_s_mean"] / out["off"]["sims_per_s_mean"]
print(json.dumps(out))
arena.close()
net.close()
ctx.close()
