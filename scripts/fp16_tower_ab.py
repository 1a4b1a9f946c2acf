"""AGZ_COMPUTE_FP16 (BF16_ACT's kernels on IEEE half) against AGZ_COMPUTE_BF16_ACT, in ONE process.

Time (`--part time`): ONE net per shape, agz_net_set_compute_mode switched between runs in the order A B B A ..., `--runs` runs per arm, one
tower queue.  Per run: two warm-up forwards, `--reps` forwards with the AGZ_PROF_CONV class timer (device events around every dual block:
per-block ms = class time / launches), then `--reps` forwards without a profiler between two fences (whole-forward ms).  Reported per arm:
mean, min and max over the runs.  Two shapes: the headline one (19x19, K = 256, 20 blocks, 512 boards) and a small board with the
packed-boards form on (9x9, K = 128, 20 blocks, 512 boards, AGZ_BF16_PACKED_ALWAYS).
Accuracy at depth (`--part accuracy`): 19x19, K = 256, 20 blocks, 2 boards, parameters tamed as the tests tame them (gamma in [0.5, 1.5],
beta N(0, 0.1)), planes N(0, 1).  Distance of the FP16, BF16_ACT and WINO_H2 (forced) tower outputs from the float64 tower of
tests/f64_tower.py on its two metrics, and max |policy - policy64|, |value - value64| against the float64 heads on the float64 tower.
Prints one JSON object per part."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import agogo_amd as A
from agogo_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("time", "accuracy", "all"), default="all")
ap.add_argument("--B", type=int, default=512)
ap.add_argument("--L", type=int, default=20)
ap.add_argument("--runs", type=int, default=6, help="runs per arm and shape")
ap.add_argument("--reps", type=int, default=10, help="forwards per timed window")
args = ap.parse_args()
MODES = {"fp16": capi.COMPUTE_FP16, "bf16_act": capi.COMPUTE_BF16_ACT}
ctx = A.Ctx(0)


def timed(S, K, L, B, packed):
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
    net.set_bf16_packed_boards(capi.BF16_PACKED_ALWAYS if packed else capi.BF16_PACKED_OFF)
    x = torch.randint(-1, 2, (B, 18, S, S), device="cuda").float()
    pol = torch.empty((B, S * S + 1), device="cuda")
    val = torch.empty((B,), device="cuda")
    torch.cuda.synchronize()

    def forwards(n):
        for _ in range(n):
            net.infer_dev(x.data_ptr(), B, pol.data_ptr(), val.data_ptr())

    def run(arm):
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
        return {"arm": arm, "block_ms": ms / launches, "forward_ms": 1e3 * dt / args.reps, "block_path": net.last_paths()[1]}

    runs = [run(("fp16", "bf16_act", "bf16_act", "fp16")[i % 4]) for i in range(2 * args.runs)]
    out = {"shape": {"size": S, "K": K, "L": L, "B": B, "packed": packed}, "reps": args.reps, "block_gflop": 2.0 * B * S * S * (2 * K) * 9 * K / 1e9,
           "finite": bool(torch.isfinite(pol).all() and torch.isfinite(val).all()), "runs": runs}
    for arm in MODES:
        bm = [r["block_ms"] for r in runs if r["arm"] == arm]
        fm = [r["forward_ms"] for r in runs if r["arm"] == arm]
        out[arm] = {"block_ms_mean": float(np.mean(bm)), "block_ms_min": float(np.min(bm)), "block_ms_max": float(np.max(bm)),
                    "forward_ms_mean": float(np.mean(fm)), "forward_ms_min": float(np.min(fm)), "forward_ms_max": float(np.max(fm))}
    net.close()
    return out


def accuracy(S, K, L, B):
    from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
    from test_tower_f64_gpu import C, build_net, draw_planes
    c = C("depth", capi.COMPUTE_FP16, 0, K, S, S, L, B, None, F=18)
    net, P, conf, _ = build_net(ctx, c, 1337)
    x = np.random.default_rng(1338).normal(0, 1, (B, 18, S, S)).astype(np.float32)
    t64 = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64 = t64.tower(x)
    p64, v64 = t64.heads(f64)
    f64 = f64.numpy()
    out = {"shape": {"size": S, "K": K, "L": L, "B": B}, "f64_tower_max": float(np.abs(f64).max()), "f64_tower_rms": float(np.sqrt((f64 ** 2).mean()))}
    for arm, mode in (("fp16", capi.COMPUTE_FP16), ("bf16_act", capi.COMPUTE_BF16_ACT), ("wino_h2", capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE)):
        net.set_compute_mode(mode)
        pol, val = net.infer(x)
        dev = net.tower_out(B)
        out[arm] = {"local": local_metric(dev, f64)[0], "diffuse": diffuse_metric(dev, f64), "max_abs_dpolicy": float(np.abs(pol - p64).max()),
                    "max_abs_dvalue": float(np.abs(val - v64).max()), "block_path": net.last_paths()[1]}
    net.close()
    return out


if args.part in ("time", "all"):
    print(json.dumps({"time_headline": timed(19, 256, args.L, args.B, False)}), flush=True)
    print(json.dumps({"time_small_board_packed": timed(9, 128, args.L, args.B, True)}), flush=True)
if args.part in ("accuracy", "all"):
    print(json.dumps({"accuracy_at_depth": accuracy(19, 256, args.L, 2)}), flush=True)
ctx.close()
