"""The few-boards form of the 16-bit block (AGZ_BF16_SMALL_FEW_ALWAYS, conv_bf16f.hpp) against the small-batch form (conv_bf16s.hpp) and the
whole-board kernel (conv_bf16a.hpp) of AGZ_COMPUTE_BF16_ACT, at 19x19, K = 256, 40 blocks and B = 1, 2, 4, 8, 16, 21, 32 boards, in ONE
process on ONE net; scripts/bf16_small_ab.py's net, class timer and fence-to-fence forward.

Arms per batch size, in the order A B C D D C B A ..., `--runs` runs per arm: A = FEW_ALWAYS (path 23), B = ALWAYS (small form, path 17),
C = OFF (whole-board kernel, path 16), D = AGZ_COMPUTE_AUTO with the latency regime on (fp32-grade, context only).  One tower queue.  Per
run: two warm-up forwards, `--reps` forwards with the AGZ_PROF_CONV class timer (per-block ms = class time / launches), then `--reps`
forwards without a profiler between two fences.  Reported per arm: mean, min and max over the runs.  Before the timed runs of a batch size
the script checks that the three 16-bit arms give the same policy and value bit for bit.  Needs a GPU; prints one JSON object."""
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
ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8, 16, 21, 32])
ap.add_argument("--size", type=int, default=19)
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--L", type=int, default=40)
ap.add_argument("--runs", type=int, default=6, help="runs per arm")
ap.add_argument("--reps", type=int, default=50, help="forwards per timed window")
ap.add_argument("--rb", type=int, default=0, help="row blocks per workgroup of the small and few-boards forms: 0 the launcher's rule, 1 / 2 / 4 forced")
args = ap.parse_args()
S, L, K, BMAX = args.size, args.L, args.K, max(args.batches)
ARMS = {"few": (capi.COMPUTE_BF16_ACT, capi.BF16_SMALL_FEW_ALWAYS), "small": (capi.COMPUTE_BF16_ACT, capi.BF16_SMALL_ALWAYS),
        "whole": (capi.COMPUTE_BF16_ACT, capi.BF16_SMALL_OFF),
        "auto_mode": (capi.COMPUTE_AUTO, capi.BF16_SMALL_OFF)}
ORDER = ("few", "small", "whole", "auto_mode", "auto_mode", "whole", "small", "few")

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
net.debug_set_bf16_small_rb(args.rb)
x = torch.randint(-1, 2, (BMAX, 18, S, S), device="cuda").float()
pol = torch.empty((BMAX, S * S + 1), device="cuda")
val = torch.empty((BMAX,), device="cuda")
torch.cuda.synchronize()


def forwards(n, B):
    for _ in range(n):
        net.infer_dev(x.data_ptr(), B, pol.data_ptr(), val.data_ptr())


def select(arm):
    net.set_compute_mode(ARMS[arm][0])
    net.set_bf16_small_batch(ARMS[arm][1])


def outputs(arm, B):
    select(arm)
    forwards(1, B)
    ctx.sync()
    return pol[:B].cpu().numpy().copy(), val[:B].cpu().numpy().copy()


def net_run(arm, B):
    select(arm)
    forwards(2, B)                                          # warm: this mode's weights, buffers and code objects
    ctx.sync()
    ctx.prof_enable(True, classes=[capi.PROF_CONV])
    forwards(args.reps, B)
    ctx.sync()
    ctx.prof_enable(False)
    launches, ms = ctx.prof_read(capi.PROF_CONV)
    ctx.sync()
    t0 = time.perf_counter()
    forwards(args.reps, B)
    ctx.sync()
    dt = time.perf_counter() - t0
    return {"arm": arm, "block_us": 1e3 * ms / launches, "forward_ms": 1e3 * dt / args.reps, "block_path": net.last_paths()[1]}


out = {"shape": {"size": S, "K": K, "L": L}, "reps": args.reps, "runs": args.runs, "rb": args.rb, "batches": {}}
for B in args.batches:
    ref = outputs("whole", B)
    same = all(np.array_equal(p, q) for arm in ("few", "small") for p, q in zip(outputs(arm, B), ref))
    runs = [net_run(ORDER[i % 8], B) for i in range(4 * args.runs)]
    res = {"few_and_small_equal_whole": bool(same), "block_gflop": 2.0 * B * S * S * (2 * K) * 9 * K / 1e9}
    for arm in ARMS:
        bu = [r["block_us"] for r in runs if r["arm"] == arm]
        fm = [r["forward_ms"] for r in runs if r["arm"] == arm]
        res[arm] = {"block_path": [r["block_path"] for r in runs if r["arm"] == arm][0],
                    "block_us_mean": float(np.mean(bu)), "block_us_min": float(np.min(bu)), "block_us_max": float(np.max(bu)),
                    "forward_ms_mean": float(np.mean(fm)), "forward_ms_min": float(np.min(fm)), "forward_ms_max": float(np.max(fm))}
    res["few_mean_below_small_min"] = res["few"]["block_us_mean"] < res["small"]["block_us_min"]
    out["batches"][str(B)] = res
print(json.dumps(out))
net.close()
ctx.close()
