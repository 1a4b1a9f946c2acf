"""AGZ_COMPUTE_BF16_ACT (bf16 activations between blocks, operands DMA'd into LDS: conv_bf16a.hpp) against AGZ_COMPUTE_BF16, the kernel it
derives from, and against AGZ_COMPUTE_WINO_H2, at the headline shape (19x19, K = 256, 20 blocks, 512 boards), in ONE process.

ONE net, agz_net_set_compute_mode switched between runs in the order A B C C B A ... (A = bf16_act, B = bf16, C = wino_h2), `--runs` runs per
arm, one tower queue (per-kernel durations inflate under the two-queue overlap).  Per run: two warm-up forwards, `--reps` forwards with the
AGZ_PROF_CONV class timer (device events around every dual block: per-block ms = class time / launches), then `--reps` forwards without a
profiler between two fences (whole-forward ms).  Reported per arm: mean, min and max over the runs.  Before the timed runs the script
checks, at the timed shape, that bf16_act and bf16 give the same policy and value bit for bit.  Prints one JSON object."""
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
ap.add_argument("--size", type=int, default=19)
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--L", type=int, default=20)
ap.add_argument("--runs", type=int, default=10, help="runs per arm")
ap.add_argument("--reps", type=int, default=10, help="forwards per timed window")
args = ap.parse_args()
S, B, L, K = args.size, args.B, args.L, args.K
MODES = {"bf16_act": capi.COMPUTE_BF16_ACT, "bf16": capi.COMPUTE_BF16, "wino_h2": capi.COMPUTE_WINO_H2}
ORDER = ("bf16_act", "bf16", "wino_h2", "wino_h2", "bf16", "bf16_act")

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


def outputs(arm):
    net.set_compute_mode(MODES[arm])
    forwards(1)
    ctx.sync()
    return pol.cpu().numpy().copy(), val.cpu().numpy().copy()


same = all(np.array_equal(p, q) for p, q in zip(outputs("bf16_act"), outputs("bf16")))


def net_run(arm):
    net.set_compute_mode(MODES[arm])
    forwards(2)                                             # warm: this mode's weights, buffers and code objects
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


runs = [net_run(ORDER[i % 6]) for i in range(3 * args.runs)]
out = {"shape": {"size": S, "B": B, "K": K, "L": L}, "reps": args.reps, "bf16_act_equals_bf16": bool(same),
       "block_gflop": 2.0 * B * S * S * (2 * K) * 9 * K / 1e9, "net_runs": runs}
for arm in MODES:
    bm = [r["block_ms"] for r in runs if r["arm"] == arm]
    fm = [r["forward_ms"] for r in runs if r["arm"] == arm]
    out[arm] = {"block_ms_mean": float(np.mean(bm)), "block_ms_min": float(np.min(bm)), "block_ms_max": float(np.max(bm)),
                "forward_ms_mean": float(np.mean(fm)), "forward_ms_min": float(np.min(fm)), "forward_ms_max": float(np.max(fm))}
out["bf16_act_mean_below_bf16_min"] = out["bf16_act"]["block_ms_mean"] < out["bf16"]["block_ms_min"]
print(json.dumps(out))
net.close()
ctx.close()
