"""GPU: the AlphaZero loss on the sharded trainer (agz_trainer_create_sharded(_tied) + agz_trainer_set_loss(AGZ_LOSS_ALPHAZERO)).  The loss
is normalised by the GLOBAL batch; the rows' cost terms are summed per rank in a fixed order and travel in the cost words of the exchange
that always carried them, summed in rank order: every rank reports the same bits.  Two rank processes on GPU 0 through tests/fake_rccl, as
in test_train_sharded_gpu.py; the worker is this file's own.

Reference: tests/f64_train_az.py at the global batch 6 of DETERMINISTIC (the draws and seeds of test_az_loss_gpu, margins re-asserted
there).  Bars: test_az_loss_gpu's — cost 1e-4 * max(1, |float64|), every gradient tensor 2e-5 * max|float64| + 1e-7, a rank's tensor being
its rows of a batch-shaped tensor and the whole of a shared one.

(The fake communicator keeps its operation count to itself, so that a step issues as many collectives as under the reference loss is not
asserted here; forward_backward_dev issues the same exchange() calls under both kinds.)"""
import numpy as np
import pytest

import test_solver_sharded_gpu as base
from f64_train_az import param_shapes
from test_az_loss_gpu import check_costs, check_grads, reference

pytestmark = pytest.mark.gpu

WORKER = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import agogo_amd as A
from agogo_amd import capi
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
tied = bool(job["tied"])
inp = np.load(job["inp"])
t = A.Trainer.sharded(ctx, comm, K, L, FC, W, H, F, Aspace, Bg, tied=tied)
r0, B, nr = t.shard()
assert (r0, B, nr) == (rank * (Bg // n), Bg // n, n)
for i in range(t.num_params()):
    name, k = t.param_info(i)
    g = inp["p%d" % i]
    t.set_param(i, g[rank * k:(rank + 1) * k] if (not tied and name.endswith(("_gamma", "_beta", "_b"))) else g)
assert t.get_loss() == capi.LOSS_REFERENCE
t.set_loss(capi.LOSS_ALPHAZERO)
cost = t.forward_backward(inp["x"][r0:r0 + B], inp["pi"][r0:r0 + B], inp["v"][r0:r0 + B])
res = {"cost": np.array([cost], np.float32), "terms": np.array(t.costs(), np.float32)}
for i in range(t.num_params()):
    res["g%d" % i] = t.get_grad(i)
t.close()
np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_two_ranks_compute_the_global_batchs_loss(ctx, tied, tmp_path, monkeypatch):
    monkeypatch.setattr(base, "WORKER", WORKER)
    n = 2
    ref = reference("DETERMINISTIC", tied=tied)
    case = ref["case"]
    Bg = case[7]
    data = {"p%d" % i: p for i, p in enumerate(ref["P"])}
    data.update(x=ref["x"], pi=ref["pi"], v=ref["v"])
    inp = str(tmp_path / "az.npz")
    np.savez(inp, **data)
    R = base.run_ranks(n, {"conf": list(case), "inp": inp, "tied": int(tied)}, tmp_path)
    assert R[0]["cost"].tobytes() == R[1]["cost"].tobytes() and R[0]["terms"].tobytes() == R[1]["terms"].tobytes(), "the cost differs between the ranks"
    names = [nm for nm, _ in param_shapes(case, tied)]
    for r in range(n):
        tag = "DETERMINISTIC %s rank %d" % ("tied" if tied else "untied", r)
        check_costs(tag, (float(R[r]["cost"][0]), float(R[r]["terms"][0]), float(R[r]["terms"][1])), ref)
        want = []
        for nm, g64 in zip(names, ref["grads"]):
            if not tied and base.batch_shaped(nm):      # this rank's rows
                k = g64.size // n
                g64 = g64[r * k:(r + 1) * k]
            want.append(g64)
        check_grads(tag, names, [R[r]["g%d" % i] for i in range(len(names))], want)
