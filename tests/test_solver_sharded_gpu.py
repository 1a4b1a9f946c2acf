"""GPU: the solver options on the sharded trainer (agz_trainer_create_sharded + agz_trainer_set_solver).  Each rank owns the velocity rows of
the batch-shaped tensors it owns; the shared tensors' velocity is computed on every rank from the summed gradient (no further
collective).  Ranks are processes on GPU 0 through tests/fake_rccl, as in test_train_sharded_gpu.py; bars: that file's for its `sgd` job
(cost 2e-5, parameters 1e-4 * max + 1e-7 per tensor), here against the plain single-process trainer at the global batch with the same
options.  The velocity is held to the same ABSOLUTE bar as its parameter (w3 = w0 + v1 + v2 + v3: their errors are of one size)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import agogo_amd as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")
MU, L2, LR = 0.9, 1e-4, 0.1

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
res = {}
for i in range(t.num_params()):
    name, k = t.param_info(i)
    g = inp["p%d" % i]
    t.set_param(i, g[rank * k:(rank + 1) * k] if name.endswith(("_gamma", "_beta", "_b")) else g)
t.set_solver(job["mu"], job["l2"], 0.0)
costs = []
for s in range(3):
    costs.append(t.batch(inp["x%d" % s][r0:r0 + B], inp["pi%d" % s][r0:r0 + B], inp["v%d" % s][r0:r0 + B], lr=job["lr"]))
res["costs"] = np.array(costs, np.float32)
for i in range(t.num_params()):
    res["p%d" % i], res["v%d" % i] = t.get_param(i), t.get_velocity(i)
t.save(job["save_to"])                      # collective: rank 0 writes the global AGZTRN02 file
t.set_solver(0.0, 0.0, 0.0)                 # (drops the velocity: the load below has to bring options and velocity back)
t.load(job["load_from"])                    # the plain trainer's AGZTRN02 file at the global batch
s = t.get_solver()
res["solver"] = np.array([s["momentum"], s["l2reg"], s["clip"]], np.float32)
for i in range(t.num_params()):
    res["lp%d" % i], res["lv%d" % i] = t.get_param(i), t.get_velocity(i)
t.close()
np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


def run_ranks(n, job, tmp_path, timeout=170):
    """n rank processes on GPU 0, each under its own time limit; no further rank is started once one has failed"""
    assert os.path.exists(FAKE), "tests/fake_rccl/librccl_fake.so is built by `make`"
    job["out"] = str(tmp_path / "mom_r%d.npz")
    spec = str(tmp_path / "mom.json")
    with open(spec, "w") as f:
        json.dump(job, f)
    env = dict(os.environ, AGZ_RCCL_LIB=FAKE)
    procs = []
    for r in range(n):
        assert all(p.poll() in (None, 0) for p in procs), "a rank failed before rank %d was started" % r
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, "-c", WORKER, str(r), str(n), spec], cwd=ROOT,
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        time.sleep(0.05)
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=timeout + 30)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, "rank %d failed (%d):\n%s" % (r, pr.returncode, logs[r][-3000:])
    return [np.load(job["out"] % r) for r in range(n)]


def batch_shaped(name):
    return name.endswith(("_gamma", "_beta", "_b"))


def batch_data(B, F, H, W, Aspace, seed):
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, 0.0, 1.0, 0.001], np.float32), size=(B, F, H, W)).astype(np.float32)
    pi = np.zeros((B, Aspace), np.float32)
    pi[np.arange(B), rng.integers(0, Aspace, B)] = 1.0
    v = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=B).astype(np.float32)
    return x, pi, v


def rank_slice(a, r, n):
    a = a.ravel()
    k = a.size // n
    return a[r * k:(r + 1) * k]


@pytest.mark.parametrize("n", [2, 3])
def test_sharded_momentum_equals_the_plain_trainer_at_the_global_batch(ctx, n, tmp_path):
    K, L, FC, W, H, F, Aspace, B = 32, 2, 32, 5, 5, 2, 26, 2      # test_three_sgd_steps_and_export_match_the_oracle's
    Bg = n * B
    plain = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    plain.init_random(9)
    rng = np.random.default_rng(9)
    names = []
    for i in range(plain.num_params()):
        nm, k = plain.param_info(i)
        names.append(nm)
        if nm.endswith("_gamma"):
            plain.set_param(i, rng.uniform(0.5, 1.5, k).astype(np.float32))
        elif nm.endswith("_beta") or nm.endswith("_b"):
            plain.set_param(i, rng.normal(0, 0.1, k).astype(np.float32))
    data = {"p%d" % i: plain.get_param(i) for i in range(plain.num_params())}
    steps = []
    for s in range(3):
        x, pi, v = batch_data(Bg, F, H, W, Aspace, seed=100 + s)
        data.update({"x%d" % s: x, "pi%d" % s: pi, "v%d" % s: v})
        steps.append((x, pi, v))
    inp = str(tmp_path / "mom.npz")
    np.savez(inp, **data)
    plain.set_solver(MU, L2, 0.0)
    costs = [plain.batch(x, pi, v, lr=LR) for x, pi, v in steps]
    pp = [plain.get_param(i) for i in range(plain.num_params())]
    pv = [plain.get_velocity(i) for i in range(plain.num_params())]
    global_file, sharded_file = tmp_path / "global.agz", tmp_path / "sharded.agz"
    plain.save(global_file)
    assert open(global_file, "rb").read(8) == b"AGZTRN02"
    R = run_ranks(n, {"conf": [K, L, FC, W, H, F, Aspace, Bg], "inp": inp, "mu": MU, "l2": L2, "lr": LR, "save_to": str(sharded_file),
                      "load_from": str(global_file)}, tmp_path)
    for r in range(n):
        assert R[r]["costs"].tobytes() == R[0]["costs"].tobytes()
    for s in range(3):
        assert abs(float(R[0]["costs"][s]) - costs[s]) <= 2e-5 * max(1.0, abs(costs[s])), (s, R[0]["costs"][s], costs[s])
    worst = [0.0, 0.0]
    for i, nm in enumerate(names):
        scale = float(np.abs(pp[i]).max())
        bar = 1e-4 * scale + 1e-7
        assert pv[i].any(), nm
        for r in range(n):
            for k, (key, ref_full) in enumerate((("p%d" % i, pp[i]), ("v%d" % i, pv[i]))):
                ref = rank_slice(ref_full, r, n) if batch_shaped(nm) else ref_full
                err = float(np.abs(R[r][key] - ref).max())
                worst[k] = max(worst[k], err / bar)
                assert err <= bar, (nm, r, key, err, bar)
                if not batch_shaped(nm):   # replicas of a shared tensor — and of its velocity — are the same bits on every rank
                    assert R[r][key].tobytes() == R[0][key].tobytes(), (nm, key, "differs between ranks")
            # the plain trainer's 02 checkpoint, loaded by the sharded trainer: this rank's rows of parameters and velocity, and the options
            for key, ref_full in (("lp%d" % i, pp[i]), ("lv%d" % i, pv[i])):
                ref = rank_slice(ref_full, r, n) if batch_shaped(nm) else ref_full
                assert R[r][key].tobytes() == ref.tobytes(), (nm, r, key)
            np.testing.assert_array_equal(R[r]["solver"], np.array([MU, L2, 0.0], np.float32))
    print("sharded momentum over %d ranks: worst parameter %.3f, worst velocity %.3f of the bar" % (n, worst[0], worst[1]))
    # the sharded save is a plain AGZTRN02 checkpoint at the global batch: a plain trainer loads the ranks' rows, velocity included
    assert open(sharded_file, "rb").read(8) == b"AGZTRN02" and os.path.getsize(sharded_file) == os.path.getsize(global_file)
    other = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    other.load(sharded_file)
    assert other.get_solver()["momentum"] == np.float32(MU)
    for i, nm in enumerate(names):
        for get, key in ((other.get_param, "p%d" % i), (other.get_velocity, "v%d" % i)):
            want = np.concatenate([R[r][key] for r in range(n)]) if batch_shaped(nm) else R[0][key]
            assert get(i).tobytes() == want.tobytes(), (nm, key)
