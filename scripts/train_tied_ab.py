"""A/B timing of the tied-affine trainer (agz_trainer_create_tied) on one MI355X at the headline trainer shape (19x19, K=256, 20 blocks,
batch 256, AGZ_COMPUTE_WINO_H2): one process, every arm a trainer of its own on the same device, the arms timed in turn round after round
(alternating order, so drift of the box falls on every arm alike).

Arms (all agz_trainer_batch, the fused step):
  base         a plain trainer of a build of the commit to compare against (--baseline-tree: a built checkout; optional)
  untied       a plain trainer of this build (must run what base runs)
  tied         a tied trainer, vanilla solver
  tied_adam    a tied trainer, Adam (0.9, 0.999, 1e-8), L2 1e-4
  untied_adam  a plain trainer with the same Adam settings (both moments of the batch-shaped gamma / beta stepped inside k_bn_bwd1)

Writes a table (per arm: every round's ms per step, min / median / max), the byte model's expectation (written before the
measurement) and the two acceptance lines: untied - base within 1 % of base, tied not slower than untied, both at the median."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tied", "train_tied_ab.txt"))
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


def make(mod, ctx, tied=False, adam=False):
    t = mod.Trainer(ctx, K, L, 2 * K, S, S, 18, S * S + 1, B, tied=True) if tied else mod.Trainer(ctx, K, L, 2 * K, S, S, 18, S * S + 1, B)
    t.init_random(1337)
    t.set_compute_mode(mod.COMPUTE_WINO_H2)
    if adam:
        t.set_adam(0.9, 0.999, 1e-8)
        t.set_solver(0.0, 1e-4, 0.0)
    return t


arms = []   # (name, step function)
ctx = A.Ctx(0)
if args.baseline_tree:
    base = load_baseline(args.baseline_tree)
    bctx = base.Ctx(0)
    tb = make(base, bctx)
    arms.append(("base", lambda t=tb: t.batch(x, pi, v)))
for name, tied, adam in (("untied", False, False), ("tied", True, False), ("tied_adam", True, True), ("untied_adam", False, True)):
    arms.append((name, lambda t=make(A.capi, ctx, tied, adam): t.batch(x, pi, v)))

ms = {name: [] for name, _ in arms}
for rnd in range(args.rounds):
    order = arms if rnd % 2 == 0 else arms[::-1]
    for name, step in order:
        step()
        t_a = time.perf_counter()
        for _ in range(args.steps):
            step()
        ms[name].append((time.perf_counter() - t_a) / args.steps * 1e3)

# byte model: per BatchNorm tensor (gamma or beta) and tower layer the untied step moves B * HW * C floats three times — the
# forward read, the backward read and the backward write; the tied step moves HW * C.  With Adam the untied step also reads and writes
# both moments of both tensors.
Kp = (K + 31) // 32 * 32
gb_floats = B * S * S * (Kp + L * 2 * Kp) * 2              # gamma + beta, init layer + L dual blocks of two branches
saved_ms = 3 * 4 * gb_floats * (1 - 1 / B) / args.bn_rate * 1e3
saved_adam_ms = saved_ms + 4 * 4 * gb_floats * (1 - 1 / B) / args.bn_rate * 1e3
lines = ["train_tied_ab: %dx%d K=%d L=%d B=%d AGZ_COMPUTE_WINO_H2, %d rounds x %d steps per arm, ms per step" % (S, S, K, L, B, args.rounds, args.steps),
         "%-14s %9s %9s %9s   rounds" % ("arm", "min", "median", "max")]
for name, _ in arms:
    r = ms[name]
    lines.append("%-14s %9.3f %9.3f %9.3f   %s" % (name, min(r), statistics.median(r), max(r), " ".join("%.3f" % q for q in r)))
med = {k: statistics.median(r) for k, r in ms.items()}
lines.append("byte model: gamma / beta streams = %.2f GB per vanilla step, at %.1f TB/s: tied expected %.2f ms faster than untied; with Adam "
             "%.2f GB: %.2f ms" % (3 * 4 * gb_floats / 1e9, args.bn_rate / 1e12, saved_ms, 7 * 4 * gb_floats / 1e9, saved_adam_ms))
if "base" in med:
    ref = med["base"]
    lines.append("untied - base = %+.3f ms (%.2f %% of base; accepted: within 1 %%): %s" %
                 (med["untied"] - ref, 100 * (med["untied"] - ref) / ref, "ok" if abs(med["untied"] - ref) <= 0.01 * ref else "NOT MET"))
else:
    lines.append("no baseline arm (--baseline-tree): the first acceptance line needs one")
lines.append("tied - untied = %+.3f ms (accepted: <= 0): %s; the model says %+.2f ms: %.0f %% of the modelled saving reached" %
             (med["tied"] - med["untied"], "ok" if med["tied"] <= med["untied"] else "NOT MET", -saved_ms, 100 * (med["untied"] - med["tied"]) / saved_ms))
lines.append("tied_adam - untied_adam = %+.3f ms; the model says %+.2f ms: %.0f %% reached" %
             (med["tied_adam"] - med["untied_adam"], -saved_adam_ms, 100 * (med["untied_adam"] - med["tied_adam"]) / saved_adam_ms))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
print(json.dumps({"ms": ms, "model_saved_ms": saved_ms, "model_saved_adam_ms": saved_adam_ms}))
