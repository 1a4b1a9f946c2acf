"""What a packed replay window (agz_replay_create_packed) costs against an unpacked one, at the headline row shape (19x19, 18 planes,
policy 362) on one GPU.  Both windows hold the same rows (planes drawn over agz_encoder_palette(AGZ_ENC_WQ)) and the arms are
alternated inside one process.  Three parts, one JSON object each:

  --part sampler   k_replay_sample_packed against k_replay_sample: minibatches of 256 rows from a window of 4096 rows, symmetric on, through
                   agz_replay_sample_dev.  The launches of the arms alternate one by one, so that a run of this part under
                   `rocprofv3 --kernel-trace --stats` gives each kernel's own time on the same minutes of the same GPU; without a
                   profiler the part reports the wall clock per launch of blocks of launches between two context synchronisations
                   (enqueue included).  The arms' outputs are compared byte for byte first.
  --part step      agz_train_replay(steps = 16, symmetric on) on the G19 trainer shape (K = 256, 20 blocks, BatchSize 256,
                   AGZ_COMPUTE_WINO_H2), ms per step, ten runs per arm in the order U P P U U P P U ...
  --part pack      one agz_replay_append_examples of --pack-rows rows into an empty window of that capacity: validation + packing against
                   the three copies of the unpacked window, between two context synchronisations.
Figures: profiles/replay_packed.md."""
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
ap.add_argument("--part", choices=["sampler", "step", "pack"], required=True)
ap.add_argument("--window", type=int, default=4096, help="rows of the window (sampler, step)")
ap.add_argument("--launches", type=int, default=400, help="sampler: alternated launches per arm")
ap.add_argument("--blocks", type=int, default=6, help="sampler: wall-clock blocks per arm")
ap.add_argument("--block", type=int, default=500, help="sampler: launches of one wall-clock block")
ap.add_argument("--runs", type=int, default=10, help="step: timed runs per arm")
ap.add_argument("--steps", type=int, default=16, help="step: steps of one run")
ap.add_argument("--pack-rows", type=int, default=131072)
args = ap.parse_args()

S, F, B = 19, 18, 256
A1 = S * S + 1
MM = S * S
WPP = (MM + 15) // 16
PACKED_ROW, PLAIN_ROW = F * WPP * 4 + A1 * 4 + 4, (F * MM + A1 + 1) * 4
ctx = A.Ctx(0)
pal = capi.encoder_palette(capi.ENC_WQ)
rng = np.random.default_rng(0)


def block_of_rows(n):
    x = rng.choice(pal.view(np.uint32), size=(n, F * MM)).astype(np.uint32).view(np.float32)
    pi = np.zeros((n, A1), np.float32)
    pi[np.arange(n), rng.integers(0, A1, n)] = 1
    v = rng.choice(np.array([-1, 0, 1], np.float32), size=n).astype(np.float32)
    return x, pi, v


def filled_examples(rows, block=4096):
    ex = A.Examples(ctx, F, S, S, A1)
    blk = block_of_rows(min(block, rows))
    done = 0
    while done < rows:
        n = min(len(blk[2]), rows - done)
        ex.append_host(blk[0][:n], blk[1][:n], blk[2][:n])
        done += n
    return ex


def windows(rows, ex=None):
    ex = ex or filled_examples(rows)
    packed = A.Replay(ctx, F, S, S, A1, rows, palette=pal)
    plain = A.Replay(ctx, F, S, S, A1, rows)
    for rp in (packed, plain):
        rp.append_examples(ex)
        assert len(rp) == rows
    return packed, plain, ex


def stats(v):
    return {"mean": float(np.mean(v)), "median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
            "std": float(np.std(v, ddof=1)) if len(v) > 1 else 0.0, "runs": [float(x) for x in v]}


out = {"part": args.part, "row_bytes": {"packed": PACKED_ROW, "unpacked": PLAIN_ROW}}
if args.part == "sampler":
    packed, plain, ex = windows(args.window)
    buf = A.Examples(ctx, F, S, S, A1)
    buf.append_host(*block_of_rows(B))
    bx, bp, bv = buf.raw_dev()
    got = A.Examples(ctx, F, S, S, A1)
    arms = [("unpacked", plain), ("packed", packed)]

    def launch(arm, step):
        arm[1].sample_dev(B, 1337, step, True, bx, bp, bv)

    ref = None                                      # the arms give the same bytes at the timed shape
    for arm in arms:
        launch(arm, 3)
        got.clear()
        got.append_dev(bx, bp, bv, B)
        res = b"".join(a.tobytes() for a in got.get())
        assert ref is None or res == ref, arm[0]
        ref = res
    for i in range(args.launches):                  # one by one: the kernel trace's part (the first launches are the warm-up)
        for arm in arms[i % len(arms):] + arms[:i % len(arms)]:
            launch(arm, i)
    ctx.sync()
    wall = {a[0]: [] for a in arms}
    for b in range(args.blocks):
        for arm in arms[b % len(arms):] + arms[:b % len(arms)]:
            ctx.sync()
            t0 = time.perf_counter()
            for i in range(args.block):
                launch(arm, i)
            ctx.sync()
            wall[arm[0]].append((time.perf_counter() - t0) / args.block * 1e6)
    out["rows"], out["window"] = B, args.window
    out["algorithmic_bytes_per_launch"] = {"packed": B * (PACKED_ROW + PLAIN_ROW), "unpacked": B * 2 * PLAIN_ROW}
    out["wall_us_per_launch"] = {k: stats(v) for k, v in wall.items() if v}
elif args.part == "step":
    K, L = 256, 20
    t = A.Trainer(ctx, K, L, 2 * K, S, S, F, A1, B)
    t.init_random(1337)
    t.set_compute_mode(capi.COMPUTE_WINO_H2)
    packed, plain, ex = windows(args.window)
    arms = {"unpacked": plain, "packed": packed}
    for rp in arms.values():
        t.train_replay(rp, 2, 3, True)
    ctx.sync()
    ms = {k: [] for k in arms}
    for i in range(2 * args.runs):
        arm = ("unpacked", "packed", "packed", "unpacked")[i % 4]
        ctx.sync()
        t0 = time.perf_counter()
        t.train_replay(arms[arm], args.steps, 3 + i, True)
        ctx.sync()
        ms[arm].append((time.perf_counter() - t0) / args.steps * 1e3)
    out["ms_per_step"] = {k: stats(v) for k, v in ms.items()}
    u, p = out["ms_per_step"]["unpacked"], out["ms_per_step"]["packed"]
    out["packed_minus_unpacked_ms"] = p["mean"] - u["mean"]
    out["unpacked_spread_ms"] = u["max"] - u["min"]
else:
    rows = args.pack_rows
    ex = filled_examples(rows)
    packed = A.Replay(ctx, F, S, S, A1, rows, palette=pal)
    plain = A.Replay(ctx, F, S, S, A1, rows)
    ms = {"unpacked": [], "packed": []}
    for i in range(4):                               # the first pair is the warm-up
        for name, rp in (("unpacked", plain), ("packed", packed)) if i % 2 == 0 else (("packed", packed), ("unpacked", plain)):
            rp.clear()
            ctx.sync()
            t0 = time.perf_counter()
            rp.append_examples(ex)
            ctx.sync()
            if i:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            assert len(rp) == rows
    out["rows"] = rows
    out["source_bytes"] = rows * PLAIN_ROW
    out["append_ms"] = {k: stats(v) for k, v in ms.items()}
    out["device_bytes"] = {"packed": packed.storage()[2], "unpacked": plain.storage()[2]}
print(json.dumps(out), flush=True)
ctx.close()
