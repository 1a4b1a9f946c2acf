"""GPU: the running BatchNorm statistics on the sharded trainer (agz_trainer_create_sharded + agz_trainer_set_bn_tracking).  The finalize
kernel of a sharded step (k_bn_fin_ranks) holds the GLOBAL batch's mean / variance, summed in rank order: every rank accumulates the same
bits.  agz_trainer_eval is collective there and exchanges the cost words alone.  Ranks are processes on GPU 0 through tests/fake_rccl, as in
test_solver_sharded_gpu.py.  Bars: the statistics' of test_bn_tracking_gpu (2e-5 of the scale for the mean, 4e-5 of the largest variance)
against the plain single-process trainer at the global batch, and its eval bar (1e-4 * max(1, |cost|)) for the held-out cost.

The local rows of the first two cases are below the single-pass threshold (4096 rows), so they run modes 0 / 1 of k_bn_fin_ranks; the third
case doubles the batch of SINGLE_PASS so that each rank's 4332 rows take mode 2."""
import numpy as np
import pytest

import agogo_amd as A
from test_bn_tracking_gpu import DETERMINISTIC, SINGLE_PASS, bn_stats, check_stats_against
from test_solver_sharded_gpu import batch_data, run_ranks

pytestmark = pytest.mark.gpu

LAM, LR = 0.9, 0.1
SINGLE_PASS_PER_RANK = SINGLE_PASS[:7] + (2 * SINGLE_PASS[7],)

WORKER = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import agogo_amd as A
rank, n, spec = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
job = json.load(open(spec))
ctx = A.Ctx(0)
idf = spec + ".uid"
if rank == 0:
    with open(idf + ".tmp", "wb") as f:
        f.write(A.Comm.unique_id())
    os.replace(idf + ".tmp", idf)
else:
    t0 = time.time()
    while not os.path.exists(idf):
        assert time.time() - t0 < 60, "rank 0 never published the unique id"
        time.sleep(0.01)
comm = A.Comm.init_rank(ctx, n, rank, open(idf, "rb").read())
K, L, FC, W, H, F, Aspace, Bg = job["conf"]
inp = np.load(job["inp"])
t = A.Trainer.sharded(ctx, comm, K, L, FC, W, H, F, Aspace, Bg)
r0, B, nr = t.shard()
for i in range(t.num_params()):
    name, k = t.param_info(i)
    g = inp["p%d" % i]
    t.set_param(i, g[rank * k:(rank + 1) * k] if name.endswith(("_gamma", "_beta", "_b")) else g)
t.set_bn_tracking(True, job["lam"])
res = {"costs": np.array([t.batch(inp["x%d" % s][r0:r0 + B], inp["pi%d" % s][r0:r0 + B], inp["v%d" % s][r0:r0 + B], lr=job["lr"])
                          for s in range(3)], np.float32)}
for i in range(t.num_bn()):
    res["m%d" % i], res["s%d" % i] = t.get_bn_stats(i)
res["weight"] = np.array([t.get_bn_tracking()["weight"]])
res["eval"] = np.array([t.eval(inp["x3"][r0:r0 + B], inp["pi3"][r0:r0 + B], inp["v3"][r0:r0 + B])], np.float32)
for i in range(t.num_bn()):          # eval leaves the estimates alone
    m, s = t.get_bn_stats(i)
    assert m.tobytes() == res["m%d" % i].tobytes() and s.tobytes() == res["s%d" % i].tobytes()
t.save(job["save_to"])                # collective: rank 0 writes the global AGZTRN03 file
t.close()
np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


@pytest.mark.parametrize("name,case", [("DETERMINISTIC", DETERMINISTIC), ("SINGLE_PASS", SINGLE_PASS), ("SINGLE_PASS_PER_RANK", SINGLE_PASS_PER_RANK)])
def test_two_ranks_track_the_global_statistics(ctx, name, case, tmp_path, monkeypatch):
    import test_solver_sharded_gpu as base
    monkeypatch.setattr(base, "WORKER", WORKER)
    n = 2
    K, L, FC, W, H, F, Aspace, Bg = case
    plain = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    plain.init_random(9)
    rng = np.random.default_rng(9)
    for i in range(plain.num_params()):
        nm, k = plain.param_info(i)
        if nm.endswith("_gamma"):
            plain.set_param(i, rng.uniform(0.5, 1.5, k).astype(np.float32))
        elif nm.endswith("_beta") or nm.endswith("_b"):
            plain.set_param(i, rng.normal(0, 0.1, k).astype(np.float32))
    data = {"p%d" % i: plain.get_param(i) for i in range(plain.num_params())}
    steps = []
    for s in range(4):
        x, pi, v = batch_data(Bg, F, H, W, Aspace, seed=100 + s)
        data.update({"x%d" % s: x, "pi%d" % s: pi, "v%d" % s: v})
        steps.append((x, pi, v))
    inp = str(tmp_path / "bn.npz")
    np.savez(inp, **data)
    plain.set_bn_tracking(True, LAM)
    for x, pi, v in steps[:3]:
        plain.batch(x, pi, v, lr=LR)
    want, want_eval, want_n = bn_stats(plain), plain.eval(*steps[3]), plain.get_bn_tracking()["weight"]
    sharded_file = tmp_path / "sharded.agz"
    R = run_ranks(n, {"conf": list(case), "inp": inp, "lam": LAM, "lr": LR, "save_to": str(sharded_file)}, tmp_path)
    nbn = plain.num_bn()
    for key in ["m%d" % i for i in range(nbn)] + ["s%d" % i for i in range(nbn)] + ["weight", "eval", "costs"]:
        assert R[0][key].tobytes() == R[1][key].tobytes(), (key, "differs between the ranks")
    assert float(R[0]["weight"][0]) == want_n
    check_stats_against([(R[0]["m%d" % i], R[0]["s%d" % i]) for i in range(nbn)],
                        [(m.astype(np.float64), s.astype(np.float64)) for m, s in want], name + " sharded")
    ev = float(R[0]["eval"][0])
    print("%s: sharded eval %.7f plain %.7f" % (name, ev, want_eval))
    assert abs(ev - want_eval) <= 1e-4 * max(1.0, abs(want_eval)), (ev, want_eval)
    # rank 0's file is a plain AGZTRN03 checkpoint at the global batch
    assert open(sharded_file, "rb").read(8) == b"AGZTRN03"
    other = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    other.load(sharded_file)
    assert other.get_bn_tracking() == {"on": True, "momentum": np.float32(LAM), "weight": want_n}
    for i, (m, s) in enumerate(bn_stats(other)):
        assert m.tobytes() == R[0]["m%d" % i].tobytes() and s.tobytes() == R[0]["s%d" % i].tobytes(), i
