"""A/B timing of the tied sharded trainer (agz_trainer_create_sharded_tied) at ONE rank through the real RCCL, on one MI355X at the headline
trainer shape (19x19, K=256, 20 blocks, batch 256, AGZ_COMPUTE_WINO_H2): one process, every arm a trainer of its own on the same device, the
arms timed in turn round after round (alternating order, so drift of the box falls on every arm alike).  After scripts/train_tied_ab.py.

Arms (all agz_trainer_batch, the fused vanilla step):
  base             a tied trainer of a build of the commit to compare against (--baseline-tree: a built checkout; optional)
  tied             a tied trainer of this build (must run what base runs)
  tied_sharded_n1  the tied sharded trainer over a one-rank communicator: the same arithmetic (bit for bit: tests/test_tied_sharded_gpu.py),
                   plus what the form adds at any n — the double partials written and read back, the self-gather copy, the rank-order kernels
                   — and the sharded step's own exchanges.  n > 1 over xGMI is not measured here.

Writes a table (per arm: every round's ms per step, min / median / max), the model's expectation (written before the measurement)
and the two acceptance lines: tied - base within 1 % of base; tied_sharded_n1 - tied at most 1.25 x the modelled delta plus the tied arm's
own spread (max - min over its rounds), both at the median."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import agogo_amd as A

ap = argparse.ArgumentParser()
ap.add_argument("--K", type=int, default=256); ap.add_argument("--L", type=int, default=20)
ap.add_argument("--B", type=int, default=256); ap.add_argument("--size", type=int, default=19)
ap.add_argument("--steps", type=int, default=3, help="timed steps per arm and round (after one untimed step)")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--baseline-tree", default="", help="a built checkout of the commit to compare against (its agogo_amd/capi.py and lib/libagz.so)")
ap.add_argument("--rate", type=float, default=2.0e12, help="bytes/s k_bn_bwd1_tied reaches (DESIGN §9, profiles/tied/train_tied_kernel_stats.txt)")
ap.add_argument("--launch-us", type=float, default=7.0, help="a small dependent launch on the step's stream (k_bn_tied_sums: 6.8 us, same profile)")
ap.add_argument("--sharded-ms", type=float, default=0.06, help="the sharded step's own exchanges at one rank (profiles/r07/train_sharded.md: 41.26 - 41.20 ms)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tied_sharded", "train_tied_sharded_ab.txt"))
args = ap.parse_args()
S, K, L, B = args.size, args.K, args.L, args.B


def load_baseline(tree):
    spec = importlib.util.spec_from_file_location("agz_baseline_capi", os.path.join(tree, "agogo_amd", "capi.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.lib()
    return m


rng = np.random.default_rng(0)
x = rng.choice(np.array([-1, 0, 1], np.float32), size=(B, 18, S, S)).astype(np.float32)
pi = np.zeros((B, S * S + 1), np.float32); pi[np.arange(B), rng.integers(0, S * S + 1, B)] = 1
v = rng.choice(np.array([-1, 0, 1], np.float32), size=B).astype(np.float32)


def ready(mod, t):
    t.init_random(1337)
    t.set_compute_mode(mod.COMPUTE_WINO_H2)
    return t


arms = []   # (name, trainer)
ctx = A.Ctx(0)
if args.baseline_tree:
    base = load_baseline(args.baseline_tree)
    bctx = base.Ctx(0)
    arms.append(("base", ready(base, base.Trainer(bctx, K, L, 2 * K, S, S, 18, S * S + 1, B, tied=True))))
comm = A.Comm.init_all([ctx])[0]
arms.append(("tied", ready(A.capi, A.Trainer(ctx, K, L, 2 * K, S, S, 18, S * S + 1, B, tied=True))))
arms.append(("tied_sharded_n1", ready(A.capi, A.Trainer.sharded(ctx, comm, K, L, 2 * K, S, S, 18, S * S + 1, B, tied=True))))

first = {name: t.batch(x, pi, v) for name, t in arms}   # the same parameters, the same data
ms = {name: [] for name, _ in arms}
for rnd in range(args.rounds):
    order = arms if rnd % 2 == 0 else arms[::-1]
    for name, t in order:
        t.batch(x, pi, v)
        t_a = time.perf_counter()
        for _ in range(args.steps):
            t.batch(x, pi, v)
        ms[name].append((time.perf_counter() - t_a) / args.steps * 1e3)

# the model (written before the measurement), per tower layer with C channels, e = 2 * HW * C elements of [gamma | beta]:
#   k_bn_bwd1_tied<.., true> writes e doubles where the plain form wrote e floats (the stepped gamma / beta):      + 4 e bytes
#   the one-rank gather copies the send buffer into the gather buffer (2048 + e doubles read and written):         + 16 e bytes
#   k_tied_ranks reads e doubles and reads and writes gamma / beta (fused vanilla step):                           + 16 e bytes
# at the rate k_bn_bwd1_tied reaches; plus one k_tied_ranks launch per layer and k_rows_ranks for the heads (L + 2 small dependent
# launches; the gathers themselves exist on every sharded step) and the sharded step's own exchanges at one rank, as measured for the
# plain sharded trainer.
Kp = (K + 31) // 32 * 32
e_all = 2 * S * S * (Kp + L * 2 * Kp)
bytes_ms = 36 * e_all / args.rate * 1e3
launch_ms = (L + 2) * args.launch_us * 1e-3
model_ms = bytes_ms + launch_ms + args.sharded_ms
lines = ["train_tied_sharded_ab: %dx%d K=%d L=%d B=%d AGZ_COMPUTE_WINO_H2, %d rounds x %d steps per arm, ms per step" % (S, S, K, L, B, args.rounds, args.steps),
         "%-16s %9s %9s %9s   rounds" % ("arm", "min", "median", "max")]
for name, _ in arms:
    r = ms[name]
    lines.append("%-16s %9.3f %9.3f %9.3f   %s" % (name, min(r), statistics.median(r), max(r), " ".join("%.3f" % q for q in r)))
med = {k: statistics.median(r) for k, r in ms.items()}
spread = max(ms["tied"]) - min(ms["tied"])
lines.append("first cost: %s (one rank: the tied trainer's bits: %s)" % (" ".join("%s %.9g" % kv for kv in first.items()), first["tied"] == first["tied_sharded_n1"]))
lines.append("model: %.0f MB of extra traffic at %.1f TB/s = %.3f ms, %d launches at %.1f us = %.3f ms, the sharded step's exchanges %.3f ms: %.3f ms" %
             (36 * e_all / 1e6, args.rate / 1e12, bytes_ms, L + 2, args.launch_us, launch_ms, args.sharded_ms, model_ms))
if "base" in med:
    ref = med["base"]
    lines.append("tied - base = %+.3f ms (%.2f %% of base; accepted: within 1 %%): %s" %
                 (med["tied"] - ref, 100 * (med["tied"] - ref) / ref, "ok" if abs(med["tied"] - ref) <= 0.01 * ref else "NOT MET"))
else:
    lines.append("no baseline arm (--baseline-tree): the first acceptance line needs one")
delta, bound = med["tied_sharded_n1"] - med["tied"], 1.25 * model_ms + spread
lines.append("tied_sharded_n1 - tied = %+.3f ms (accepted: <= 1.25 x %.3f + the tied arm's spread %.3f = %.3f ms): %s" %
             (delta, model_ms, spread, bound, "ok" if delta <= bound else "NOT MET"))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
print(json.dumps({"ms": ms, "model_ms": model_ms, "first_cost": first}))
for _, t in arms[::-1]:
    t.close()
comm.close()
ctx.close()
