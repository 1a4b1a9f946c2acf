"""GPU: Adam on the sharded trainer (agz_trainer_create_sharded + agz_trainer_set_adam).  Each rank owns the moment rows of the batch-shaped
tensors it owns; the shared tensors' moments follow on every rank from the summed gradient (no further collective).  Ranks are processes
on GPU 0 through tests/fake_rccl, as in test_solver_sharded_gpu.py, each under its own time limit, at most three processes on the GPU
(the test's and two ranks); bars: that file's (cost 2e-5, parameters 1e-4 * max + 1e-7 per tensor), here against the plain single-process
trainer at the global batch with the same settings, the two moments held to the same ABSOLUTE bar as their parameter.

eps is eps* = the median |g| of a first scratch forward_backward of the plain trainer and lr = 0.1 * eps* (test_adam_gpu.py says why: the
two trainers compute the same gradient in different orders, and Adam's map is not Lipschitz in g near |g| ~ eps)."""
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
B1, B2, L2, STEPS = 0.9, 0.999, 1e-4, 2

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
t.set_adam(job["b1"], job["b2"], job["eps"])
t.set_solver(0.0, job["l2"], 0.0)
costs = []
for s in range(job["steps"]):
    costs.append(t.batch(inp["x%d" % s][r0:r0 + B], inp["pi%d" % s][r0:r0 + B], inp["v%d" % s][r0:r0 + B], lr=job["lr"]))
res["costs"] = np.array(costs, np.float32)
for i in range(t.num_params()):
    res["p%d" % i] = t.get_param(i)
    res["m%d" % i], res["v%d" % i] = t.get_moments(i)
res["t"] = np.array([t.get_adam()["t"]])
t.save(job["save_to"])                      # collective: rank 0 writes the global AGZTRN04 file
t.set_adam(on=False)                        # (drops the moments: the load below has to bring settings, counter and moments back)
t.set_solver(0.0, 0.0, 0.0)
t.load(job["load_from"])                    # the plain trainer's AGZTRN04 file at the global batch
s, a = t.get_solver(), t.get_adam()
res["solver"] = np.array([s["momentum"], s["l2reg"], s["clip"], a["beta1"], a["beta2"], a["eps"], a["on"], a["t"]], np.float32)
for i in range(t.num_params()):
    res["lp%d" % i] = t.get_param(i)
    res["lm%d" % i], res["lv%d" % i] = t.get_moments(i)
t.close()
np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


def run_ranks(n, job, tmp_path, timeout=170):
    """n rank processes on GPU 0, each under its own time limit; no further rank is started once one has failed"""
    assert os.path.exists(FAKE), "tests/fake_rccl/librccl_fake.so is built by `make`"
    job["out"] = str(tmp_path / "adam_r%d.npz")
    spec = str(tmp_path / "adam.json")
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


def test_sharded_adam_equals_the_plain_trainer_at_the_global_batch(ctx, tmp_path):
    n = 2
    K, L, FC, W, H, F, Aspace, B = 32, 2, 32, 5, 5, 2, 26, 2      # test_solver_sharded_gpu's
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
    for s in range(STEPS):
        x, pi, v = batch_data(Bg, F, H, W, Aspace, seed=100 + s)
        data.update({"x%d" % s: x, "pi%d" % s: pi, "v%d" % s: v})
        steps.append((x, pi, v))
    inp = str(tmp_path / "adam.npz")
    np.savez(inp, **data)
    plain.forward_backward(*steps[0])          # the scratch pass: gradients only, the parameters stay
    eps = float(np.median(np.concatenate([np.abs(plain.get_grad(i)) for i in range(plain.num_params())])))
    assert eps > 0
    lr = 0.1 * eps
    plain.set_adam(B1, B2, eps)
    plain.set_solver(0.0, L2, 0.0)
    costs = [plain.batch(x, pi, v, lr=lr) for x, pi, v in steps]
    pp = [plain.get_param(i) for i in range(plain.num_params())]
    pm = [plain.get_moments(i) for i in range(plain.num_params())]
    global_file, sharded_file = tmp_path / "global.agz", tmp_path / "sharded.agz"
    plain.save(global_file)
    assert open(global_file, "rb").read(8) == b"AGZTRN04"
    R = run_ranks(n, {"conf": [K, L, FC, W, H, F, Aspace, Bg], "inp": inp, "b1": B1, "b2": B2, "eps": eps, "l2": L2, "lr": lr, "steps": STEPS,
                      "save_to": str(sharded_file), "load_from": str(global_file)}, tmp_path)
    for r in range(n):
        assert R[r]["costs"].tobytes() == R[0]["costs"].tobytes()
        assert int(R[r]["t"][0]) == STEPS
    for s in range(STEPS):
        assert abs(float(R[0]["costs"][s]) - costs[s]) <= 2e-5 * max(1.0, abs(costs[s])), (s, R[0]["costs"][s], costs[s])
    worst = [0.0, 0.0, 0.0]
    f = np.float32
    for i, nm in enumerate(names):
        scale = float(np.abs(pp[i]).max())
        bar = 1e-4 * scale + 1e-7
        assert pm[i][0].any() and pm[i][1].any(), nm
        for r in range(n):
            for k, (key, ref_full) in enumerate((("p%d" % i, pp[i]), ("m%d" % i, pm[i][0]), ("v%d" % i, pm[i][1]))):
                ref = rank_slice(ref_full, r, n) if batch_shaped(nm) else ref_full
                err = float(np.abs(R[r][key] - ref).max())
                worst[k] = max(worst[k], err / bar)
                assert err <= bar, (nm, r, key, err, bar)
                if not batch_shaped(nm):   # replicas of a shared tensor — and of its moments — are the same bits on every rank
                    assert R[r][key].tobytes() == R[0][key].tobytes(), (nm, key, "differs between ranks")
            # the plain trainer's 04 checkpoint, loaded by the sharded trainer: this rank's rows of parameters and moments, and the settings
            for key, ref_full in (("lp%d" % i, pp[i]), ("lm%d" % i, pm[i][0]), ("lv%d" % i, pm[i][1])):
                ref = rank_slice(ref_full, r, n) if batch_shaped(nm) else ref_full
                assert R[r][key].tobytes() == ref.tobytes(), (nm, r, key)
            np.testing.assert_array_equal(R[r]["solver"], np.array([0.0, f(L2), 0.0, f(B1), f(B2), f(eps), 1, STEPS], np.float32))
    print("sharded Adam over %d ranks: worst parameter %.3f, worst m %.3f, worst v %.3f of the bar" % (n, worst[0], worst[1], worst[2]))
    # the sharded save is a plain AGZTRN04 checkpoint at the global batch: a plain trainer loads the ranks' rows, moments included
    assert open(sharded_file, "rb").read(8) == b"AGZTRN04" and os.path.getsize(sharded_file) == os.path.getsize(global_file)
    other = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    other.load(sharded_file)
    st = other.get_adam()
    assert st["on"] and st["t"] == STEPS and st["eps"] == f(eps) and other.get_solver()["l2reg"] == f(L2)
    for i, nm in enumerate(names):
        m, v = other.get_moments(i)
        for got, key in ((other.get_param(i), "p%d" % i), (m, "m%d" % i), (v, "v%d" % i)):
            want = np.concatenate([R[r][key] for r in range(n)]) if batch_shaped(nm) else R[0][key]
            assert got.tobytes() == want.tobytes(), (nm, key)
