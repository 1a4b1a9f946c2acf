"""CPU: choose the learn rates of tests/test_train_history_gpu.py's resume tests, and grade the tied trainer's draws, with float64 alone.
usage: python scripts/debug/history_lr_scan.py [plain|tied] [sgd|adam] ...   (no argument: all four, then the tied draws)

The resume tests take three batch(lr) steps at shape P (16x17, B = 2, K = 256, two blocks) on draws 101, 102, 106 and need a block layer whose
input range (max of the tensor the layer reads) has ANOTHER binary exponent in step 3 than in step 2, so that the planes k_bn_apply_v wrote
under step 2's range are NOT the ones step 3 may keep.  Here: the same three steps in float64 (tests/f64_train.py for the gradients; the
update rules restated: w -= lr g, and Adam with beta 0.9 / 0.999, eps 1e-8, bias-corrected), per learn rate the ranges of layers 1 and 2 at
the parameters steps 2 and 3 run on.  A learn rate is usable when some layer's exponent differs and both ranges are at least 6 % away
from the power of two between them (the device steps in fp32: 1e-4 of a trajectory, far inside that margin), everything finite.
Tied draws: the fp32 oracle with tiled rows, row gradients summed (test_tied_cpu.oracle_tied) against float64 the same way; usable when
within half the gradient bar (1e-5 of the tensor maximum + 5e-8), the rule of scripts/debug/wide_seed_scan.py.
Test infrastructure (imports oracle/ through tests/oracle_lib.py); not part of the product."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np
from f64_train import f64_train
from oracle_train_vs_f64 import oracle_net
from test_train_gpu import batch_data
from test_tied_cpu import is_batch_shaped, oracle_tied

W, H, B, K, L, FC, F = 16, 17, 2, 256, 2, 32, 18
A = H * W + 1
SEEDS = (101, 102, 106)
LRS = {"sgd": (0.005, 0.01, 0.02, 0.03, 0.05, 0.07, 0.1, 0.5), "adam": (0.02, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6, 0.8, 1.0, 1.5, 2.0, 3.0)}


def start(tied):
    ot = oracle_net(K, L, FC, W, H, F, A, B)
    names = [ot.param_name(i) for i in range(ot.num_params())]
    P = [ot.get_param(i).astype(np.float64) for i in range(ot.num_params())]
    if tied:
        P = [p.reshape(B, -1)[0].copy() if is_batch_shaped(nm) else p for nm, p in zip(names, P)]
    return names, P


def grads_and_ranges(names, P, tied, data):
    full = [np.tile(p, B) if tied and is_batch_shaped(nm) else p for nm, p in zip(names, P)]
    cost, G, pre = f64_train(full, *data, K, L, FC, W, H, F, A, B, want_pre=True)
    if tied:
        G = [g.reshape(B, -1).sum(axis=0) if is_batch_shaped(nm) else g for nm, g in zip(names, G)]
    relu = lambda a: np.maximum(a, 0.0)
    rng = [float(relu(pre[0]).max())] + [float(relu(relu(pre[2 * b + 1]) + relu(pre[2 * b + 2])).max()) for b in range(L - 1)]
    return cost, G, rng      # rng[l - 1]: the range of layer l's input, l = 1 .. L


def run(tied, kind, lr):
    names, P = start(tied)
    M = [np.zeros_like(p) for p in P]
    V = [np.zeros_like(p) for p in P]
    out = []
    for t, seed in enumerate(SEEDS, 1):
        cost, G, rng = grads_and_ranges(names, P, tied, batch_data(B, F, H, W, A, seed=seed))
        out.append((cost, rng))
        for i, g in enumerate(G):
            if kind == "adam":
                M[i] = 0.9 * M[i] + 0.1 * g
                V[i] = 0.999 * V[i] + 0.001 * g * g
                P[i] = P[i] - lr * (M[i] / (1 - 0.9 ** t)) / (np.sqrt(V[i] / (1 - 0.999 ** t)) + 1e-8)
            else:
                P[i] = P[i] - lr * g
    return out


def scan(tied, kind):
    for lr in LRS[kind]:
        out = run(tied, kind, lr)
        (c2, r2), (c3, r3) = out[1], out[2]
        ok = []
        for l in range(L):
            if not (np.isfinite(r2[l]) and np.isfinite(r3[l]) and r2[l] > 0 and r3[l] > 0):
                continue
            e2, e3 = int(np.floor(np.log2(r2[l]))), int(np.floor(np.log2(r3[l])))
            edge = 2.0 ** max(e2, e3)
            if e2 != e3 and min(abs(r2[l] / edge - 1), abs(r3[l] / edge - 1)) >= 0.06:
                ok.append(l + 1)
        print("%s %s lr %g: costs %s; ranges step 2 %s step 3 %s -> %s" % ("tied" if tied else "plain", kind, lr, ["%.4g" % o[0] for o in out],
              ["%.4g" % r for r in r2], ["%.4g" % r for r in r3], "usable (layers %r)" % ok if ok and all(np.isfinite(o[0]) for o in out) else "-"), flush=True)


def tied_draws():
    names, P = start(True)
    P32 = [p.astype(np.float32) for p in P]
    for seed in range(100, 108):
        data = batch_data(B, F, H, W, A, seed=seed)
        _, GO = oracle_tied((K, L, FC, W, H, F, A, B), names, P32, *data)
        _, G64, _ = grads_and_ranges(names, P, True, data)
        worst = max((float(np.abs(go - g).max()) / (float(np.abs(g).max()) + 1e-30), nm) for nm, go, g in zip(names, GO, G64))
        ok = all(float(np.abs(go - g).max()) <= 1e-5 * float(np.abs(g).max()) + 5e-8 for go, g in zip(GO, G64))
        print("tied draw %d: worst tensor %s at %.2e of its maximum -> %s" % (seed, worst[1], worst[0], "ok" if ok else "SKIP"), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    for tied in (False, True):
        for kind in ("sgd", "adam"):
            if not args or (("tied" if tied else "plain") in args and kind in args):
                scan(tied, kind)
    if not args or "draws" in args:
        tied_draws()
