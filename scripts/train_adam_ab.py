"""A/B timing of the trainer's Adam solver on one MI355X at the headline trainer shape (19x19, K=256, 20 blocks, batch 256,
AGZ_COMPUTE_WINO_H2): one process, every arm a trainer of its own on the same device, the arms timed in turn round after round
(alternating order, so drift of the box falls on every arm alike).

Arms:
  base           agz_trainer_batch of a build of the commit to compare against (--baseline-tree: a built checkout; optional)
  off            agz_trainer_batch, default solver (Adam off, all options 0)
  adam_fused     agz_trainer_batch with Adam (0.9, 0.999, 1e-8), L2 1e-4 (both moments stepped inside k_bn_bwd1)
  adam_two_pass  agz_trainer_forward_backward + agz_trainer_apply with the same settings (gradients materialised, one flat sweep)

Writes a table (per arm: every round's ms per step, min / median / max), the byte model's expectation for the fused Adam step and the two
acceptance lines (off - base within 1 % of base; adam_fused - base at most 1.25 x the model), both against the baseline arm."""
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
ap.add_argument("--bn-rate", type=float, default=5.3e12, help="bytes/s k_bn_bwd1 reaches (profiles/r04/train_kernel_stats.txt)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam", "train_adam_ab.txt"))
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


def make(mod, ctx):
    t = mod.Trainer(ctx, K, L, 2 * K, S, S, 18, S * S + 1, B)
    t.init_random(1337)
    t.set_compute_mode(mod.COMPUTE_WINO_H2)
    return t


arms = []   # (name, trainer, step function)
ctx = A.Ctx(0)
if args.baseline_tree:
    base = load_baseline(args.baseline_tree)
    bctx = base.Ctx(0)
    tb = make(base, bctx)
    arms.append(("base", lambda t=tb: t.batch(x, pi, v)))


def two_pass(t):
    c = t.forward_backward(x, pi, v)
    t.apply(0.1)
    ctx.sync()
    return c


tv = make(A.capi, ctx)
arms.append(("off", lambda t=tv: t.batch(x, pi, v)))
tm = make(A.capi, ctx)
tm.set_adam(0.9, 0.999, 1e-8)
tm.set_solver(0.0, 1e-4, 0.0)
arms.append(("adam_fused", lambda t=tm: t.batch(x, pi, v)))
t2 = make(A.capi, ctx)
t2.set_adam(0.9, 0.999, 1e-8)
t2.set_solver(0.0, 1e-4, 0.0)
arms.append(("adam_two_pass", lambda t=t2: two_pass(t)))

ms = {name: [] for name, _ in arms}
for rnd in range(args.rounds):
    order = arms if rnd % 2 == 0 else arms[::-1]
    for name, step in order:
        step()
        t_a = time.perf_counter()
        for _ in range(args.steps):
            step()
        ms[name].append((time.perf_counter() - t_a) / args.steps * 1e3)

# byte model: the fused Adam step reads and writes both moments of every batch-shaped gamma / beta of the tower once
Kp = (K + 31) // 32 * 32
gb_floats = B * S * S * (Kp + L * 2 * Kp) * 2              # gamma + beta, init layer + L dual blocks of two branches
extra_ms = 4 * 4 * gb_floats / args.bn_rate * 1e3
lines = ["train_adam_ab: %dx%d K=%d L=%d B=%d AGZ_COMPUTE_WINO_H2, %d rounds x %d steps per arm, ms per step" % (S, S, K, L, B, args.rounds, args.steps),
         "%-14s %9s %9s %9s   rounds" % ("arm", "min", "median", "max")]
for name, _ in arms:
    r = ms[name]
    lines.append("%-14s %9.3f %9.3f %9.3f   %s" % (name, min(r), statistics.median(r), max(r), " ".join("%.3f" % q for q in r)))
med = {k: statistics.median(r) for k, r in ms.items()}
lines.append("byte model: m and v of gamma / beta read + written = %.2f GB per step; at %.1f TB/s: +%.2f ms expected, accepted margin 1.25x = +%.2f ms"
             % (4 * 4 * gb_floats / 1e9, args.bn_rate / 1e12, extra_ms, 1.25 * extra_ms))
if "base" in med:
    ref = med["base"]
    lines.append("off - base = %+.3f ms (%.2f %% of base; accepted: within 1 %%): %s" %
                 (med["off"] - ref, 100 * (med["off"] - ref) / ref, "ok" if abs(med["off"] - ref) <= 0.01 * ref else "NOT MET"))
    lines.append("adam_fused - base = %+.3f ms (accepted: at most %+.2f ms): %s" %
                 (med["adam_fused"] - ref, 1.25 * extra_ms, "ok" if med["adam_fused"] - ref <= 1.25 * extra_ms else "NOT MET"))
else:
    lines.append("no baseline arm (--baseline-tree): the acceptance lines need one; adam_fused - off = %+.3f ms" % (med["adam_fused"] - med["off"]))
lines.append("adam_two_pass - adam_fused = %+.3f ms" % (med["adam_two_pass"] - med["adam_fused"]))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
print(json.dumps({"ms": ms, "expected_extra_ms": extra_ms}))
