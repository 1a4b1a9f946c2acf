"""A/B timing of the trainer's loss kind (agz_trainer_set_loss) on one MI355X at the headline trainer shape (19x19, K=256, 20 blocks, batch
256, AGZ_COMPUTE_WINO_H2), untied and tied.

Every measurement is a process of its own with ONE trainer in it, started in turn round after round (parent build, this build, parent
build, ...), so drift of the box falls on every build alike and nothing but the build differs between two processes.  (Several trainers
in one process do not measure the builds: where a trainer's two streams land depends on how many streams the process made before, and a
tied trainer whose side stream lost its overlap runs at 46 ms instead of 39 — the figure agz_trainer_set_dma_forward bit 4, no side
stream, gives on purpose.  profiles/az_loss.md keeps those runs.)  A process times its arms in turn, `--inner` times; every timed window is
`--steps` steps after two untimed ones and ends in the step's own synchronise (agz_trainer_batch reads the cost back).

Arms:
  base   agz_trainer_batch of a build of the commit to compare against (--baseline-tree: a built checkout); its processes' medians
         differ by the run-to-run spread of identical code
  off    agz_trainer_batch of this build, the loss kind AGZ_LOSS_REFERENCE
  on     the same trainer after agz_trainer_set_loss(AGZ_LOSS_ALPHAZERO): the two arms differ in the loss kernels alone

Done means: |off - base| (median of the processes' medians) lies within the spread of the base processes (largest minus smallest process
median); no default instantiation changed, so a larger gap is a bug.  `on` is reported without a bar.  Writes a markdown report."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--K", type=int, default=256); ap.add_argument("--L", type=int, default=20)
ap.add_argument("--B", type=int, default=256); ap.add_argument("--size", type=int, default=19)
ap.add_argument("--steps", type=int, default=10, help="timed steps per window (after two untimed steps)")
ap.add_argument("--inner", type=int, default=4, help="windows per arm and process")
ap.add_argument("--rounds", type=int, default=3, help="processes per build")
ap.add_argument("--baseline-tree", default="", help="a built checkout of the commit to compare against (its agogo_amd/capi.py and lib/libagz.so)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "az_loss.md"))
ap.add_argument("--child", default="", help="(internal) base / new: run one process's measurement and print one JSON line")
ap.add_argument("--tied", type=int, default=0, help="(internal)")
args = ap.parse_args()
S, K, L, B = args.size, args.K, args.L, args.B
LR = 1e-3   # (small: neither loss runs away over a process's few hundred steps)


def child():
    import numpy as np
    if args.child == "base":
        spec = importlib.util.spec_from_file_location("agz_baseline_capi", os.path.join(args.baseline_tree, "agogo_amd", "capi.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.lib()
    else:
        import agogo_amd as A
        mod = A.capi
    rng = np.random.default_rng(0)
    x = rng.choice(np.array([-1, 0, 1], np.float32), size=(B, 18, S, S)).astype(np.float32)
    z = rng.normal(0, 2.0, (B, S * S + 1))
    pi = np.exp(z - z.max(axis=1, keepdims=True)); pi = (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)
    v = rng.uniform(-1, 1, B).astype(np.float32)
    ctx = mod.Ctx(0)
    t = mod.Trainer(ctx, K, L, 2 * K, S, S, 18, S * S + 1, B, tied=bool(args.tied))
    t.init_random(1337)
    t.set_compute_mode(mod.COMPUTE_WINO_H2)
    arms = [("base", None)] if args.child == "base" else [("off", mod.LOSS_REFERENCE), ("on", mod.LOSS_ALPHAZERO)]
    ms, last = {name: [] for name, _ in arms}, {}
    for w in range(args.inner):
        for name, kind in (arms if w % 2 == 0 else arms[::-1]):
            if kind is not None:
                t.set_loss(kind)
            t.batch(x, pi, v, lr=LR); t.batch(x, pi, v, lr=LR)
            t_a = time.perf_counter()
            for _ in range(args.steps):
                last[name] = t.batch(x, pi, v, lr=LR)
            ms[name].append((time.perf_counter() - t_a) / args.steps * 1e3)
    t.close(); ctx.close()
    print(json.dumps({"ms": ms, "last": last}))


def driver():
    text = ["# Loss kind A/B (scripts/az_loss_ab.py)", "",
            "%dx%d, K=%d, %d blocks, batch %d, AGZ_COMPUTE_WINO_H2; one process per measurement, %d processes per build in turn, %d windows x %d "
            "timed steps per arm and process (two untimed steps first), ms per step." % (S, S, K, L, B, args.rounds, args.inner, args.steps), "",
            "Command: `python scripts/az_loss_ab.py --baseline-tree <a built checkout of the parent commit>`", ""]
    builds = (["base"] if args.baseline_tree else []) + ["new"]
    everything = {}
    for tied in (0, 1):
        runs = {}   # arm -> list over processes of that process's windows
        for rnd in range(args.rounds):
            for build in builds:
                cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", build, "--tied", str(tied), "--K", str(K),
                       "--L", str(L), "--B", str(B), "--size", str(S), "--steps", str(args.steps), "--inner", str(args.inner),
                       "--baseline-tree", args.baseline_tree]
                r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                if r.returncode != 0:       # nothing more is started on the device after a failure
                    sys.exit("%s process failed (%d):\n%s" % (build, r.returncode, r.stderr.decode(errors="replace")[-3000:]))
                res = json.loads(r.stdout.decode().strip().splitlines()[-1])
                for name, w in res["ms"].items():
                    runs.setdefault(name, []).append(w)
                print("%s round %d %s: %s" % ("tied" if tied else "untied", rnd, build,
                                              " ".join("%s %.3f" % (k, statistics.median(w)) for k, w in res["ms"].items())), file=sys.stderr, flush=True)
        tag = "tied" if tied else "untied"
        everything[tag] = runs
        lines = ["## %s" % tag, "", "| arm | median of the processes' medians | each process's median | every window |", "|---|---|---|---|"]
        med = {}
        for name, procs in runs.items():
            pm = [statistics.median(w) for w in procs]
            med[name] = statistics.median(pm)
            lines.append("| %s | %.3f | %s | %s |" % (name, med[name], " ".join("%.3f" % q for q in pm),
                                                      " / ".join(" ".join("%.3f" % q for q in w) for w in procs)))
        lines.append("")
        if "base" in runs:
            pm = [statistics.median(w) for w in runs["base"]]
            spread = max(pm) - min(pm)
            lines.append("spread of identical code (largest minus smallest median of the base processes) = %.3f ms" % spread)
            lines.append("")
            lines.append("off - base = %+.3f ms (%+.2f %%): %s the spread.  on - base = %+.3f ms (%+.2f %%), on - off = %+.3f ms, no bar."
                         % (med["off"] - med["base"], 100 * (med["off"] - med["base"]) / med["base"],
                            "within" if abs(med["off"] - med["base"]) <= spread else "OUTSIDE",
                            med["on"] - med["base"], 100 * (med["on"] - med["base"]) / med["base"], med["on"] - med["off"]))
        else:
            lines.append("on - off = %+.3f ms (%+.2f %%); no baseline tree given" % (med["on"] - med["off"], 100 * (med["on"] - med["off"]) / med["off"]))
        text += lines + [""]
    text = "\n".join(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    print(json.dumps({"ms": everything}))


if args.child:
    child()
else:
    driver()
