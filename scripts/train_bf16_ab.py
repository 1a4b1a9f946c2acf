"""A/B: the trainer's AGZ_COMPUTE_WINO_H2 against AGZ_COMPUTE_BF16 at the G19 shape (K = 256, 20 blocks, B = 256, 19x19), tied and untied,
the two arms alternated in one process.  Prints the per-step times of every run (forward_backward from host batches, the same copies in
both arms) and one JSON line per trainer kind.  bench.py does not call this; results: profiles/train_bf16.md.

    python scripts/train_bf16_ab.py [--runs 10] [--steps 5] [--blocks 20] [--batch 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import agogo_amd as A  # noqa: E402
from agogo_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    ctx = A.Ctx(0)
    rng = np.random.default_rng(0)
    B = a.batch
    x = rng.choice(np.array([-1, 0, 1], np.float32), size=(B, 18, 19, 19)).astype(np.float32)
    pi = np.zeros((B, 362), np.float32)
    pi[np.arange(B), rng.integers(0, 362, B)] = 1
    v = rng.choice(np.array([-1, 1], np.float32), size=B).astype(np.float32)
    for tied in (False, True):
        t = A.Trainer(ctx, 256, a.blocks, 256, 19, 19, 18, 362, B, tied=tied)
        arms = {"wino_h2": capi.COMPUTE_WINO_H2, "bf16": capi.COMPUTE_BF16}
        ms = {k: [] for k in arms}
        paths = {}
        for run in range(a.runs + 1):                      # run 0 warms both arms up (allocations, first launches)
            for name, mode in arms.items():
                t.set_compute_mode(mode)
                t.forward_backward(x, pi, v)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    t.forward_backward(x, pi, v)
                dt = (time.perf_counter() - t0) * 1e3 / a.steps
                paths[name] = t.last_paths(1)[:3]
                if run:
                    ms[name].append(dt)
                    print("tied %d run %2d %-8s %.3f ms / step" % (tied, run, name, dt), flush=True)
        t.close()
        print(json.dumps({"tied": tied, "blocks": a.blocks, "batch": B, "paths_layer1": paths,
                          **{k: {"median_ms": float(np.median(w)), "min_ms": float(min(w)), "max_ms": float(max(w))} for k, w in ms.items()}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
