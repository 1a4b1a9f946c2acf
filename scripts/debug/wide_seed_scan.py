"""CPU: choose the data draws of tests/test_train_wide_gpu.py with the oracle alone.
usage: python scripts/debug/wide_seed_scan.py [CASE ...]   (no argument: every case, then the family)
Per case, seeds from 100 upwards: the worst |g_oracle - g_f64| / max|g_f64| over the gradient tensors; a seed is usable when the fp32 oracle
is within HALF the trainer's bar (1e-5 of the maximum + 5e-8) on every tensor.  Prints the first three usable seeds and the skipped ones.
       python scripts/debug/wide_seed_scan.py --unit CASE SEED BN BOARD CHANNEL ROW COLUMN
           the float64 pre-activation (argument of the ReLU) of one unit of the BN-th BatchNorm (0 = Init, 1 / 2 = L1 / L2 of block 0, ...) on
           that draw, and how many units of the tower lie within 1e-6 of zero: what a replaced seed has to show.
Test infrastructure (imports oracle/ through tests/oracle_lib.py); not part of the product."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np
from f64_train import f64_train
from oracle_train_vs_f64 import oracle_net
from test_train_gpu import batch_data
import test_train_wide_gpu as T


def scan(tag, conf, first, want):
    K, L, FC, W, H, F, A, B = (conf[k] for k in ("K", "L", "FC", "W", "H", "F", "A", "B"))
    ot = oracle_net(K, L, FC, W, H, F, A, B)
    params = [ot.get_param(i) for i in range(ot.num_params())]
    good, skipped, seed = [], [], first
    while len(good) < want and seed < first + 12:
        t0 = time.time()
        x, pi, v = batch_data(B, F, H, W, A, seed=seed)
        co = ot.batch(x, pi, v, lr=0.0)
        t1 = time.time()
        c64, g64 = f64_train(params, x, pi, v, K, L, FC, W, H, F, A, B)
        worst, ok = (0.0, ""), True
        for i in range(ot.num_params()):
            s = float(np.abs(g64[i]).max()); e = float(np.abs(ot.get_grad(i) - g64[i]).max())
            worst = max(worst, (e / (s + 1e-30), ot.param_name(i)))
            ok = ok and e <= 1e-5 * s + 5e-8
        print("%s seed %d: oracle %.1f s, float64 %.1f s, |cost_o - cost_f64| %.1e, worst tensor %s at %.2e of its maximum -> %s"
              % (tag, seed, t1 - t0, time.time() - t1, abs(co - c64), worst[1], worst[0], "ok" if ok else "SKIP"), flush=True)
        (good if ok else skipped).append(seed)
        seed += 1
    print("%s: seeds %r skipped %r" % (tag, tuple(good), skipped), flush=True)


def unit(name, seed, k, b, c, y, x):
    conf = T.conf_of(*T.CASES[name][0]) if name in T.CASES else T.conf_of(*T.family_draw(int(name[4:]))[:5])
    K, L, FC, W, H, F, A, B = (conf[q] for q in ("K", "L", "FC", "W", "H", "F", "A", "B"))
    ot = oracle_net(K, L, FC, W, H, F, A, B)
    xs, pi, v = batch_data(B, F, H, W, A, seed=seed)
    _, _, pre = f64_train([ot.get_param(i) for i in range(ot.num_params())], xs, pi, v, K, L, FC, W, H, F, A, B, want_pre=True)
    tower = pre[:2 * L + 1]
    print("%s draw %d, BatchNorm %d, board %d channel %d pixel (%d, %d): float64 pre-activation %.3e (rms of the layer's %.3f); %d of %d tower units within 1e-6 of zero"
          % (name, seed, k, b, c, y, x, pre[k][b, c, y, x], np.sqrt((pre[k] ** 2).mean()), sum(int((np.abs(p) < 1e-6).sum()) for p in tower), sum(p.size for p in tower)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--unit"]:
        unit(sys.argv[2], *[int(a) for a in sys.argv[3:9]])
        sys.exit(0)
    names = sys.argv[1:] or list(T.CASES) + ["fam_%d" % s for s in range(12)]
    for name in names:
        if name.startswith("fam_"):
            W, H, B, K, L, mode = T.family_draw(int(name[4:]))
            scan("%s %dx%d B=%d K=%d L=%d %s" % (name, W, H, B, K, L, mode), T.conf_of(W, H, B, K, L), 200 + int(name[4:]), 1)
        else:
            scan(name, T.conf_of(*T.CASES[name][0]), 100, 3)
