"""The cost of the sharded replay route (profiles/replay_sharded.md), on the GPU.  Two parts, one JSON line each:

  --part digest    agz_replay_digest at the 19x19 / 18 planes / 362 policy shape: windows of --rows rows (unpacked and packed) and a packed
                   window of --packed-rows rows, filled device to device from one block of rows; the whole call between two host clocks
                   (it ends in a synchronise), --runs runs per window after one warm-up, the windows taken in turn.  Bytes = what the window
                   holds on the device for its live rows (agz_replay_storage's row bytes): the digest reads each of them once.
  --part step      two ranks (processes on GPU 0 over tests/fake_rccl) at the shape of tests/test_replay_sharded_gpu.py: per-step wall time
                   of train_replay_sharded(steps) against sharded train_dev(batches = steps, iterations = 1) over the same minibatches
                   sampled beforehand, --runs runs per arm, alternated; rank 0 reports.  A sanity ratio, not a bar.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import agogo_amd as A  # noqa: E402
from agogo_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["digest", "step"], required=True)
ap.add_argument("--rows", type=int, default=800000, help="digest: rows of the unpacked and of the small packed window")
ap.add_argument("--packed-rows", type=int, default=7000000, help="digest: rows of the large packed window")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--steps", type=int, default=200, help="step: steps of one run")
ap.add_argument("--rank", type=int, default=-1, help="step: set by the parent process")
ap.add_argument("--uid", default="")
args = ap.parse_args()


def stats(v):
    return {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [float(x) for x in v]}


if args.part == "digest":
    S, F = 19, 18
    A1 = S * S + 1
    ctx = A.Ctx(0)
    pal = capi.encoder_palette(capi.ENC_WQ)
    rng = np.random.default_rng(0)
    block = 16384
    x = rng.choice(pal.view(np.uint32), size=(block, F * S * S)).astype(np.uint32).view(np.float32)
    pi = rng.random(size=(block, A1), dtype=np.float32)
    v = rng.choice(np.array([-1, 0, 1], np.float32), size=block).astype(np.float32)
    ex = A.Examples(ctx, F, S, S, A1)
    ex.append_host(x, pi, v)
    bx, bp, bv = ex.raw_dev()

    def filled(rows, palette):
        rp = A.Replay(ctx, F, S, S, A1, rows, palette=palette)
        done = 0
        while done < rows:
            n = min(block, rows - done)
            rp.append_dev(bx, bp, bv, n)
            done += n
        assert len(rp) == rows
        return rp

    arms = [("unpacked", filled(args.rows, None)), ("packed", filled(args.rows, pal)), ("packed-large", filled(args.packed_rows, pal))]
    # the small windows hold the same rows: the same digest; and the host definition over the first block
    small = A.Replay(ctx, F, S, S, A1, block)
    small.append_dev(bx, bp, bv, block)
    assert small.digest() == capi.replay_digest_host(x, pi, v, F, S * S, A1)
    ms = {name: [] for name, _ in arms}
    digests = {}
    for i in range(args.runs + 1):
        for name, rp in arms:
            ctx.sync()
            t0 = time.perf_counter()
            d = rp.digest()
            dt = (time.perf_counter() - t0) * 1e3
            assert digests.setdefault(name, d) == d
            if i:
                ms[name].append(dt)
    assert digests["unpacked"] == digests["packed"]
    out = {"part": "digest", "shape": [F, S, S, A1], "windows": {}}
    for name, rp in arms:
        row_bytes = rp.storage()[1]
        nbytes = row_bytes * len(rp)
        st = stats(ms[name])
        out["windows"][name] = {"rows": len(rp), "row_bytes": row_bytes, "bytes": nbytes, "elements": len(rp) * (F * S * S + A1 + 1), "ms": st,
                                "GB_per_s": nbytes / (st["mean"] * 1e-3) / 1e9,
                                "Gelements_per_s": len(rp) * (F * S * S + A1 + 1) / (st["mean"] * 1e-3) / 1e9}
    print(json.dumps(out))
elif args.rank < 0:
    fake = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")
    assert os.path.exists(fake), fake
    uid = os.path.join(tempfile.mkdtemp(), "uid")
    env = dict(os.environ, AGZ_RCCL_LIB=fake)
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--part", "step", "--rank", str(r), "--uid", uid,
                               "--runs", str(args.runs), "--steps", str(args.steps)], env=env) for r in range(2)]
    rcs = [p.wait() for p in procs]
    if os.path.exists(uid):
        os.remove(uid)
    assert rcs == [0, 0], rcs
else:
    K, L, FC, S, F, Aspace, Bg = 32, 1, 16, 3, 2, 10, 8
    rank, steps = args.rank, args.steps
    ctx = A.Ctx(0)
    if rank == 0:
        with open(args.uid + ".tmp", "wb") as f:
            f.write(A.Comm.unique_id())
        os.replace(args.uid + ".tmp", args.uid)
    else:
        t0 = time.time()
        while not os.path.exists(args.uid):
            assert time.time() - t0 < 60
            time.sleep(0.01)
    comm = A.Comm.init_rank(ctx, 2, rank, open(args.uid, "rb").read())
    rng = np.random.default_rng(3)
    n = 20
    x = rng.choice(np.array([0.0, 1.0], np.float32), size=(n, F * S * S)).astype(np.float32)
    pi = np.zeros((n, Aspace), np.float32)
    pi[np.arange(n), rng.integers(0, Aspace, n)] = 1
    v = rng.choice(np.array([-1, 0, 1], np.float32), n).astype(np.float32)
    rp = A.Replay(ctx, F, S, S, Aspace, 12)
    rp.append_host(x, pi, v)
    mb = [rp.sample(Bg, 1, s, True) for s in range(steps)]
    ex = A.Examples(ctx, F, S, S, Aspace)
    ex.append_host(np.concatenate([m[0] for m in mb]).reshape(steps * Bg, -1), np.concatenate([m[1] for m in mb]), np.concatenate([m[2] for m in mb]))
    xd, pd, vd = ex.raw_dev()
    out = {"part": "step", "conf": [K, L, FC, S, S, F, Aspace, Bg], "ranks": 2, "steps": steps, "ms_per_step": {}}
    for tied in (False, True):
        t = A.Trainer.sharded(ctx, comm, K, L, FC, S, S, F, Aspace, Bg, tied=tied)
        t.init_random(9)
        arms = {"train_dev": lambda: t.train_dev(xd, pd, vd, steps, 1, seed=5), "replay_sharded": lambda: t.train_replay_sharded(rp, steps, 1, True, True),
                "replay_sharded_noverify": lambda: t.train_replay_sharded(rp, steps, 1, True, False)}
        for fn in arms.values():
            fn()
        ms = {k: [] for k in arms}
        order = list(arms)
        for i in range(args.runs):
            for k in order[i % 3:] + order[:i % 3]:
                ctx.sync()
                t0 = time.perf_counter()
                arms[k]()
                ctx.sync()
                ms[k].append((time.perf_counter() - t0) / steps * 1e3)
        out["ms_per_step"]["tied" if tied else "plain"] = {k: stats(vv) for k, vv in ms.items()}
        t.close()
    if rank == 0:
        print(json.dumps(out))
    comm.close()
    ctx.close()
