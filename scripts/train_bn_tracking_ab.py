"""A/B timing of the trainer's running BatchNorm statistics on one MI355X at the headline trainer shape (19x19, K=256, 20 blocks,
batch 256, AGZ_COMPUTE_WINO_H2): one process, every arm a trainer of its own on the same device, the arms timed in turn round after round
(alternating order, so drift of the box falls on every arm alike).

Arms:
  base   agz_trainer_batch of a build of the commit to compare against (--baseline-tree: a built checkout; optional)
  off    agz_trainer_batch, tracking never enabled
  on     agz_trainer_batch with agz_trainer_set_bn_tracking(1, 0.997): the accumulation runs inside the finalize kernels
  eval   agz_trainer_eval on the `on` arm's trainer (forward only, the statistics kernels replaced by k_bn_from_running)

Acceptance (on medians, against the base arm): off - base and on - base each <= 1 % of base.  eval is reported, not gated.
Writes a table (per arm: every round's ms per step, min / median / max)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_tracking", "train_bn_tracking_ab.txt"))
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


arms = []   # (name, step function)
ctx = A.Ctx(0)
if args.baseline_tree:
    base = load_baseline(args.baseline_tree)
    bctx = base.Ctx(0)
    tb = make(base, bctx)
    arms.append(("base", lambda t=tb: t.batch(x, pi, v)))
toff = make(A.capi, ctx)
arms.append(("off", lambda t=toff: t.batch(x, pi, v)))
ton = make(A.capi, ctx)
ton.set_bn_tracking(True, 0.997)
arms.append(("on", lambda t=ton: t.batch(x, pi, v)))
arms.append(("eval", lambda t=ton: t.eval(x, pi, v)))     # (after `on` in the first round: the estimates exist)

ms = {name: [] for name, _ in arms}
for rnd in range(args.rounds):
    order = arms if rnd % 2 == 0 else arms[::-1]
    for name, step in order:
        step()
        t_a = time.perf_counter()
        for _ in range(args.steps):
            step()
        ms[name].append((time.perf_counter() - t_a) / args.steps * 1e3)

lines = ["train_bn_tracking_ab: %dx%d K=%d L=%d B=%d AGZ_COMPUTE_WINO_H2, %d rounds x %d steps per arm, ms per step" % (S, S, K, L, B, args.rounds, args.steps),
         "%-6s %9s %9s %9s   rounds" % ("arm", "min", "median", "max")]
for name, _ in arms:
    r = ms[name]
    lines.append("%-6s %9.3f %9.3f %9.3f   %s" % (name, min(r), statistics.median(r), max(r), " ".join("%.3f" % q for q in r)))
med = {k: statistics.median(r) for k, r in ms.items()}
ref_name = "base" if "base" in med else "off"
ref = med[ref_name]
lines.append("off - %s = %+.3f ms (%+.2f %%);  on - %s = %+.3f ms (%+.2f %%);  accepted: each <= 1 %% of %s = %.3f ms"
             % (ref_name, med["off"] - ref, 100 * (med["off"] - ref) / ref, ref_name, med["on"] - ref, 100 * (med["on"] - ref) / ref, ref_name, 0.01 * ref))
lines.append("N after the run: %.6f" % ton.get_bn_tracking()["weight"])
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
print(json.dumps({"ms": ms}))
