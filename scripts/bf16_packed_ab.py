"""The packed-boards form of the AGZ_COMPUTE_BF16_ACT block (agz_net_set_bf16_packed_boards, conv_bf16p.hpp) against that mode's whole-board
kernel (conv_bf16a.hpp) on small boards, in ONE process, one net per shape: G9 (9x9, K = 128, 10 blocks, 18 planes) and C4 (7x6, K = 64,
6 blocks, 2 planes), at B = 512, 256, 64 and the first B on either side of AGZ_BF16_PACKED_AUTO's boundary (boards x 128-filter tiles
against the CU count: 129 | 128 and 257 | 256 on 256 CUs).

Arms per batch size, in the order A B C C B A ..., `--runs` runs per arm: A = policy ALWAYS (packed form, the launcher's G), B = policy OFF
(whole-board kernel, path 16), C = AGZ_COMPUTE_WINO_H2 (as context).  One tower queue.  Per run: two warm-up forwards, `--reps` forwards
with the AGZ_PROF_CONV class timer (device events around every dual block: per-block us = class time / launches), then `--reps` forwards
without a profiler between two fences (whole-forward ms).  Reported per arm: mean, min and max over the runs.  Before the timed runs of a
batch size the script asserts that ALWAYS and OFF give the same policy and value bit for bit.  `--debug-g` adds, at the first shape and
its first batch size, one line per forced G (agz_net_debug_set_bf16_packed_g), three runs each.  Prints one JSON object."""
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

SHAPES = {"G9": dict(W=9, H=9, K=128, L=10, F=18), "C4": dict(W=7, H=6, K=64, L=6, F=2)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["G9", "C4"], choices=sorted(SHAPES))
ap.add_argument("--batches", type=int, nargs="+", default=[512, 256, 64])
ap.add_argument("--runs", type=int, default=6, help="runs per arm")
ap.add_argument("--reps", type=int, default=300, help="forwards per timed window")
ap.add_argument("--debug-g", type=int, nargs="*", default=[], help="forced boards per workgroup, measured at the first shape and batch")
args = ap.parse_args()
ARMS = {"packed": (capi.COMPUTE_BF16_ACT, capi.BF16_PACKED_ALWAYS), "whole": (capi.COMPUTE_BF16_ACT, capi.BF16_PACKED_OFF),
        "wino_h2": (capi.COMPUTE_WINO_H2, capi.BF16_PACKED_OFF)}
ORDER = ("packed", "whole", "wino_h2", "wino_h2", "whole", "packed")

ctx = A.Ctx(0)
cus = torch.cuda.get_device_properties(0).multi_processor_count
out = {"cus": cus, "reps": args.reps, "runs": args.runs, "shapes": {}}
for si, name in enumerate(args.shapes):
    s = SHAPES[name]
    W, H, K, L, F = s["W"], s["H"], s["K"], s["L"], s["F"]
    edge = cus // (2 * K // 128)                            # AUTO: packed from edge + 1 boards
    batches = sorted(set(args.batches) | {edge, edge + 1}, reverse=True)
    BMAX = max(batches)
    net = A.Net(ctx, K, L, 2 * K, W, H, F, W * H + 1, bn_mode=capi.BN_IDENTITY)
    net.init_random(1337)
    for i in range(net.num_params()):
        pname, n = net.param_info(i)
        if pname.endswith("_gamma"):
            net.set_param(i, np.ones(n, np.float32))
        elif pname.endswith("_beta"):
            net.set_param(i, np.zeros(n, np.float32))
    net.commit()
    net.set_tower_queues(1)
    x = torch.randint(-1, 2, (BMAX, F, H, W), device="cuda").float()
    pol = torch.empty((BMAX, W * H + 1), device="cuda")
    val = torch.empty((BMAX,), device="cuda")
    torch.cuda.synchronize()

    def forwards(n, B):
        for _ in range(n):
            net.infer_dev(x.data_ptr(), B, pol.data_ptr(), val.data_ptr())

    def select(arm, g=0):
        net.set_compute_mode(ARMS[arm][0])
        net.set_bf16_packed_boards(ARMS[arm][1])
        net.debug_set_bf16_packed_g(g)

    def outputs(arm, B):
        select(arm)
        forwards(1, B)
        ctx.sync()
        return pol[:B].cpu().numpy().copy(), val[:B].cpu().numpy().copy()

    def net_run(arm, B, g=0):
        select(arm, g)
        forwards(2, B)                                      # warm: this mode's weights, buffers and code objects
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

    def stats(runs):
        bu, fm = [r["block_us"] for r in runs], [r["forward_ms"] for r in runs]
        return {"block_path": runs[0]["block_path"],
                "block_us_mean": float(np.mean(bu)), "block_us_min": float(np.min(bu)), "block_us_max": float(np.max(bu)),
                "forward_ms_mean": float(np.mean(fm)), "forward_ms_min": float(np.min(fm)), "forward_ms_max": float(np.max(fm))}

    shp = {"shape": s, "G": capi.lib().agz_bf16_packed_boards_of(H, W), "auto_packed_from": edge + 1, "batches": {}}
    for B in batches:
        assert all(np.array_equal(p, q) for p, q in zip(outputs("packed", B), outputs("whole", B))), (name, B)
        runs = [net_run(ORDER[i % 6], B) for i in range(3 * args.runs)]
        res = {"packed_equals_whole": True, "block_gflop": 2.0 * B * W * H * (2 * K) * 9 * K / 1e9}
        for arm in ARMS:
            res[arm] = stats([r for r in runs if r["arm"] == arm])
        res["packed_mean_below_whole_min"] = res["packed"]["block_us_mean"] < res["whole"]["block_us_min"]
        shp["batches"][str(B)] = res
    if si == 0 and args.debug_g:
        shp["debug_g"] = {"B": batches[0], **{str(g): stats([net_run("packed", batches[0], g) for _ in range(3)]) for g in args.debug_g}}
    out["shapes"][name] = shp
    net.close()
print(json.dumps(out))
ctx.close()
