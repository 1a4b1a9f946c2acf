"""One AZ.Learn epoch (agogo.go:100-172) across N ranks, one GPU each, with dual.Train on the SHARDED trainer (agz_trainer_create_sharded):
  1. self-play: the games are sharded over the ranks (no data-path collective),
  2. the recorded examples are all-gathered (agz_examples_allgather) into a device Examples set,
  3. prepareExamples with a shared seed and the GLOBAL batch (every rank holds the same tensors),
  4. dual.Train at BatchSize = world * batch: train_dev on the sharded trainer — rank r trains rows [r * batch, (r + 1) * batch) of every
     global batch, BatchNorm statistics over the global batch, only the shared tensors' gradients summed — the run IS dual.Train at the
     global batch; the shared tensors stay identical on every rank and so do the exported nets,
  5. SwitchToInference (row-0 export, broadcast from rank 0) and the A-vs-B arena games, sharded again; wins all-reduced.
Prints one JSON line (rank 0).
Launch: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 scripts/learn_epoch_sharded.py
        (add --shared-gpu on a 1-GPU box: all ranks use GPU 0 and gloo).
"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.distributed as dist

import agogo_amd as A
from agogo_amd import capi
from agogo_amd import dist as adist

ap = argparse.ArgumentParser()
ap.add_argument("--shared-gpu", action="store_true")
ap.add_argument("--size", type=int, default=3, help="board size (mnk size x size, k = size for 3, else 4)")
ap.add_argument("--K", type=int, default=32)
ap.add_argument("--L", type=int, default=2)
ap.add_argument("--games", type=int, default=64, help="self-play games in total (sharded)")
ap.add_argument("--arena-games", type=int, default=32)
ap.add_argument("--budget", type=int, default=30)
ap.add_argument("--batch", type=int, default=32, help="rows per rank: the global batch is world * batch")
ap.add_argument("--nniters", type=int, default=2)
args = ap.parse_args()

rank, local, world = adist.init_from_env(backend="gloo" if args.shared_gpu else None)
if args.shared_gpu:
    local = 0
torch.cuda.set_device(local)
ctx = A.Ctx(local)
S, K, L = args.size, args.K, args.L
kk = 3 if S == 3 else 4
Aspace = S * S + 1
Bg = world * args.batch
t0 = time.perf_counter()


def digest(arrays):
    """8 bytes of a hash of the arrays' bits, as an int64 tensor (gathered to compare ranks)"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return torch.tensor([int.from_bytes(h.digest()[:8], "little", signed=True)], dtype=torch.int64)


def same_everywhere(t):
    if world == 1:
        return True
    ts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(ts, t)
    return all(torch.equal(x, ts[0]) for x in ts)


# agent A (current best, inference), identical on every rank; the communicator comes first: the learner is sharded over it
netA = A.Net(ctx, K, L, 2 * K, S, S, 2, Aspace)
netA.init_random(11)
netA.commit()
comm = adist.make_comm(ctx) if world > 1 else A.Comm.init_all([ctx])[0]
trainB = A.Trainer.sharded(ctx, comm, K, L, 2 * K, S, S, 2, Aspace, Bg)
trainB.init_random(12)    # this rank's rows of the global initialisation

# 1. self-play, sharded
lo, hi = adist.shard_games(args.games, rank, world)
sp = A.Arena(ctx, capi.GAME_MNK, S, S, kk, encoder=capi.ENC_TWOPLANE, n_games=hi - lo, seed=1000 + lo, Budget=args.budget)
sp.set_inferencer(0, capi.INF_NET, netA)
sp.set_inferencer(1, capi.INF_NET, netA)
sp.reset()
sp.play(0, True)
t_play = time.perf_counter() - t0

# 2. + 3. gather, prepare at the global batch (same seed everywhere)
ex = A.Examples(ctx, 2, S, S, Aspace)
ex.append_arena(sp)
comm.allgather_examples(ex)
n_all = len(ex)
batches = ex.prepare(Bg, 0, seed=77)
xd, pd, vd, rows, _ = ex.tensors_dev()
if batches < 1:
    raise SystemExit("too few examples (%d) for a global batch of %d" % (n_all, Bg))

# 4. dual.Train at the global batch: every rank passes the same global tensors, trains its rows of each batch
t1 = time.perf_counter()
cost = trainB.train_dev(xd, pd, vd, batches, args.nniters, seed=1234)
ctx.sync()
t_train = time.perf_counter() - t1
names = [trainB.param_info(i)[0] for i in range(trainB.num_params())]
shared = [trainB.get_param(i) for i, nm in enumerate(names) if not nm.endswith(("_gamma", "_beta", "_b"))]
shared_same = same_everywhere(digest(shared))

# 5. SwitchToInference (collective export: rank 0's row 0 everywhere) + arena games A vs B, sharded
netB = A.Net(ctx, K, L, 2 * K, S, S, 2, Aspace)
trainB.export(netB)
nets_same = same_everywhere(digest([netB.get_param(i) for i in range(netB.num_params())]))
alo, ahi = adist.shard_games(args.arena_games, rank, world)
ev = A.Arena(ctx, capi.GAME_MNK, S, S, kk, encoder=capi.ENC_TWOPLANE, n_games=max(ahi - alo, 1), seed=5000 + alo, Budget=args.budget)
ev.set_inferencer(0, capi.INF_NET, netA)
ev.set_inferencer(1, capi.INF_NET, netB)
ev.reset()
ev.play(0, False)
r = ev.results()
wins = torch.tensor([r["a_wins"], r["b_wins"], r["draws"]], dtype=torch.float64)
if world > 1:
    dist.all_reduce(wins)
ok = shared_same and nets_same
if rank == 0:
    print(json.dumps({"LEARN_EPOCH_SHARDED": "OK" if ok else "REPLICAS DIVERGED", "world": world, "global_batch": Bg,
                      "selfplay_games": args.games, "examples_gathered": n_all, "batches": batches,
                      "train_steps": batches * args.nniters, "last_cost": cost, "shared_identical": shared_same, "nets_identical": nets_same,
                      "arena": {"a_wins": int(wins[0]), "b_wins": int(wins[1]), "draws": int(wins[2])},
                      "seconds": time.perf_counter() - t0, "selfplay_seconds": t_play, "train_seconds": t_train}))
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
for h in (ev, netB, ex, sp, trainB, comm, netA):
    h.close()
ctx.close()
sys.exit(0 if ok else 1)
