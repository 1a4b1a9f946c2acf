"""AGZ_COMPUTE_BF16 (one bf16 product per multiply, conv_bf16.hpp) against AGZ_COMPUTE_WINO_H2 at the headline shape (19x19, K = 256,
20 blocks, 512 boards), in ONE process, the two modes alternating.

Part 1, the network alone: ONE net, agz_net_set_compute_mode switched between runs in the order A B B A ..., ten runs per arm, one tower
queue (per-kernel durations inflate under the two-queue overlap).  Per run: `--reps` forwards with the AGZ_PROF_CONV class timer (device
events around every dual block: per-block ms = class time / launches), then `--reps` forwards without a profiler between two fences
(whole-forward ms).  Reported per arm: mean, min and max over the runs, and the bf16 block's rate as a fraction of the 1772 TFLOP/s a
bare bf16 MFMA loop sustains on random operands (conv_x3.hpp).
Part 2, self-play: one arena of `--games` games plays whole moves, the mode switched between moves (A B B A); whole-move sims/s per arm
(the Winograd arm takes the two-queue split step where it engages, the bf16 arm the joined step: what a user gets).
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import agogo_amd as A
from agogo_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=512)
ap.add_argument("--games", type=int, default=512)
ap.add_argument("--size", type=int, default=19)
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--L", type=int, default=20)
ap.add_argument("--runs", type=int, default=10, help="runs per arm of part 1")
ap.add_argument("--reps", type=int, default=10, help="forwards per timed window")
ap.add_argument("--budget", type=int, default=800)
ap.add_argument("--moves", type=int, default=4, help="timed whole moves of part 2, half per arm (0: skip part 2)")
args = ap.parse_args()
S, B, L, K = args.size, args.B, args.L, args.K
MODES = {"wino_h2": capi.COMPUTE_WINO_H2, "bf16": capi.COMPUTE_BF16}
SUSTAINED_TFLOPS = 1772.0


def order(n):
    return [("wino_h2", "bf16", "bf16", "wino_h2")[i % 4] for i in range(n)]


ctx = A.Ctx(0)
net = A.Net(ctx, K, L, 2 * K, S, S, 18, S * S + 1, bn_mode=capi.BN_IDENTITY)
net.init_random(1337)
for i in range(net.num_params()):
    name, n = net.param_info(i)
    if name.endswith("_gamma"):
        net.set_param(i, np.ones(n, np.float32))
    elif name.endswith("_beta"):
        net.set_param(i, np.zeros(n, np.float32))
net.commit()
net.set_tower_queues(1)
x = torch.randint(-1, 2, (B, 18, S, S), device="cuda").float()
pol = torch.empty((B, S * S + 1), device="cuda")
val = torch.empty((B,), device="cuda")
torch.cuda.synchronize()


def forwards(n):
    for _ in range(n):
        net.infer_dev(x.data_ptr(), B, pol.data_ptr(), val.data_ptr())


def net_run(arm):
    net.set_compute_mode(MODES[arm])
    forwards(2)                                             # warm: this mode's weights, scratch and code objects
    ctx.sync()
    ctx.prof_enable(True, classes=[capi.PROF_CONV])
    forwards(args.reps)
    ctx.sync()
    ctx.prof_enable(False)
    launches, ms = ctx.prof_read(capi.PROF_CONV)
    ctx.sync()
    t0 = time.perf_counter()
    forwards(args.reps)
    ctx.sync()
    dt = time.perf_counter() - t0
    return {"arm": arm, "block_ms": ms / launches, "block_launches": launches, "forward_ms": 1e3 * dt / args.reps, "block_path": net.last_paths()[1]}


runs = [net_run(arm) for arm in order(2 * args.runs)]
block_flop = 2.0 * B * S * S * (2 * K) * 9 * K
out = {"shape": {"size": S, "B": B, "K": K, "L": L}, "reps": args.reps, "block_gflop": block_flop / 1e9, "net_runs": runs}
for arm in MODES:
    bm = [r["block_ms"] for r in runs if r["arm"] == arm]
    fm = [r["forward_ms"] for r in runs if r["arm"] == arm]
    out[arm] = {"block_ms_mean": float(np.mean(bm)), "block_ms_min": float(np.min(bm)), "block_ms_max": float(np.max(bm)),
                "forward_ms_mean": float(np.mean(fm)), "forward_ms_min": float(np.min(fm)), "forward_ms_max": float(np.max(fm))}
out["bf16"]["block_tflops"] = block_flop / (out["bf16"]["block_ms_mean"] * 1e-3) / 1e12
out["bf16"]["fraction_of_sustained_1772"] = out["bf16"]["block_tflops"] / SUSTAINED_TFLOPS

if args.moves > 0:
    net.set_tower_queues(0)                                 # self-play as a user runs it
    G, Bu = args.games, args.budget
    arena = A.Arena(ctx, capi.GAME_WQ, S, S, komi=7.5, encoder=capi.ENC_WQ, n_games=G, seed=1337, Budget=Bu)
    arena.set_inferencer(0, capi.INF_NET, net)
    arena.set_inferencer(1, capi.INF_NET, net)
    arena.reset()
    arena.random_moves(np.random.default_rng(1337).integers(0, int(0.6 * S * S) + 1, size=G).astype(np.int32), 1337)

    def whole_move(arm):
        net.set_compute_mode(MODES[arm])
        ctx.sync()
        s0, t0 = arena.stats(), time.perf_counter()
        arena.begin_move()
        for _ in range(Bu):
            arena.simulate(1)
        arena.end_move(True)
        ctx.sync()
        dt = time.perf_counter() - t0
        s1 = arena.stats()
        return {"arm": arm, "seconds": dt, "sims_per_s": (s1["sims_nonnull"] - s0["sims_nonnull"]) / dt, "split_steps": arena.split_steps()[0]}

    whole_move("wino_h2")                                   # untimed: every root evaluated, pools grown
    moves = [whole_move(arm) for arm in order(args.moves)]
    out["arena"] = {"games": G, "budget": Bu, "moves": moves}
    for arm in MODES:
        v = [m["sims_per_s"] for m in moves if m["arm"] == arm]
        out["arena"][arm] = {"sims_per_s_mean": float(np.mean(v)), "sims_per_s_min": float(np.min(v)), "sims_per_s_max": float(np.max(v))}
    arena.close()
print(json.dumps(out))
net.close()
ctx.close()
