"""GPU: the sharded trainer (agz_trainer_create_sharded) — dual.Train at the GLOBAL batch split over n ranks, each rank owning its rows of
the batch-shaped gamma / beta and FC biases.  Ranks are processes on GPU 0 through tests/fake_rccl (AGZ_RCCL_LIB), as in
test_comm_fake_gpu.py; every rank process runs a list of jobs over one communicator and saves what it computed, this process compares:
against oracle_lib.Trainer at BatchSize = n * B (the bars of test_train_gpu.py), against a plain single-process trainer, and across ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")

WORKER = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import agogo_amd as A
from agogo_amd import capi
rank, n, spec = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
jobs = json.load(open(spec))
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
MODES = {"f32": capi.COMPUTE_F32_MFMA, "wino_h2": capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE}

def batch_shaped(name):
    return name.endswith(("_gamma", "_beta", "_b"))

def rows(a, r0, B):
    return np.ascontiguousarray(a[r0:r0 + B])

def set_params(t, inp):
    for i in range(t.num_params()):
        name, k = t.param_info(i)
        g = inp["p%d" % i]
        t.set_param(i, g[rank * k:(rank + 1) * k] if batch_shaped(name) else g)

def err(fn):
    try:
        fn()
    except A.AgzError as e:
        return str(e)
    return ""

for ji, job in enumerate(jobs):
    K, L, FC, W, H, F, Aspace, Bg = job["conf"]
    inp = np.load(job["inp"]) if job.get("inp") else None
    res = {}
    t = A.Trainer.sharded(ctx, comm, K, L, FC, W, H, F, Aspace, Bg)
    r0, B, nr = t.shard()
    res["shard"] = np.array([r0, B, nr])
    if job.get("mode"):
        t.set_compute_mode(MODES[job["mode"]])
    kind = job["kind"]
    if kind == "fb":
        set_params(t, inp)
        res["cost"] = np.float32(t.forward_backward(rows(inp["x"], r0, B), rows(inp["pi"], r0, B), rows(inp["v"], r0, B)))
        for i in range(t.num_params()):
            res["g%d" % i] = t.get_grad(i)
    elif kind == "sgd":
        set_params(t, inp)
        costs = []
        for s in range(3):
            costs.append(t.batch(rows(inp["x%d" % s], r0, B), rows(inp["pi%d" % s], r0, B), rows(inp["v%d" % s], r0, B), lr=0.1))
        res["costs"] = np.array(costs, np.float32)
        for i in range(t.num_params()):
            res["p%d" % i] = t.get_param(i)
        net = A.Net(ctx, K, L, FC, W, H, F, Aspace, bn_mode=capi.BN_IDENTITY)
        t.export(net)
        for i in range(net.num_params()):
            res["n%d" % i] = net.get_param(i)
        net.close()
    elif kind == "identity":   # n = 1: the sharded trainer against a plain one, bit for bit
        pt = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
        for tt in (t, pt):
            if job.get("mode"):
                tt.set_compute_mode(MODES[job["mode"]])
            tt.init_random(job["seed"])
        x, pi, v = inp["x"], inp["pi"], inp["v"]
        res["cost"] = np.array([t.forward_backward(x, pi, v), pt.forward_backward(x, pi, v)], np.float32)
        for i in range(t.num_params()):
            res["gs%d" % i], res["gp%d" % i] = t.get_grad(i), pt.get_grad(i)
        res["cost_b"] = np.array([t.batch(x, pi, v, lr=0.1), pt.batch(x, pi, v, lr=0.1)], np.float32)
        for i in range(t.num_params()):
            res["ps%d" % i], res["pp%d" % i] = t.get_param(i), pt.get_param(i)
        pt.close()
    elif kind == "misc":   # initialisation, checkpoints both ways, refusals
        t.init_random(job["seed"])
        for i in range(t.num_params()):
            res["i%d" % i] = t.get_param(i)
        t.save(job["save_to"])
        t.load(job["load_from"])
        for i in range(t.num_params()):
            res["l%d" % i] = t.get_param(i)
        res["e_div"] = np.array(err(lambda: A.Trainer.sharded(ctx, comm, K, L, FC, W, H, F, Aspace, Bg + 1)) if n > 1 else "")
        x = np.zeros((B, F, H, W), np.float32); pi = np.zeros((B, Aspace), np.float32); v = np.zeros(B, np.float32)
        res["e_ar"] = np.array(err(lambda: comm.allreduce_trainer(t)))
        res["e_fba"] = np.array(err(lambda: comm.forward_backward_allreduce(t, x, pi, v)))
        gp, _ = t.grads_dev()
        res["e_fbad"] = np.array(err(lambda: comm.forward_backward_allreduce_dev(t, gp, gp, gp)))
    elif kind == "train_dev":
        ex = A.Examples(ctx, F, H, W, Aspace)
        ex.append_host(inp["x"], inp["pi"], inp["v"])
        batches = ex.prepare(Bg, 0, seed=77)
        xd, pd, vd, _, _ = ex.tensors_dev()
        set_params(t, inp)
        res["cost"] = np.float32(t.train_dev(xd, pd, vd, batches, 2, seed=job["seed"]))
        for i in range(t.num_params()):
            res["p%d" % i] = t.get_param(i)
        ex.close()
    elif kind == "fail":   # inject a failure on one rank before layer l's first exchange; the next step is an ordinary one
        t.init_random(3)
        x, pi, v = rows(inp["x"], r0, B), rows(inp["pi"], r0, B), rows(inp["v"], r0, B)
        res["clean"] = np.float32(t.forward_backward(x, pi, v))
        for k, layer in enumerate(job["layers"]):
            if rank == job["bad_rank"]:
                comm.debug_fail_layer(layer)
            res["msg%d" % k] = np.array(err(lambda: t.forward_backward(x, pi, v)))
            res["next%d" % k] = np.float32(t.forward_backward(x, pi, v))
    t.close()
    np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


def run_ranks(n, jobs, tmp_path, tag, timeout=170):
    """n rank processes on GPU 0 run `jobs` (collectively, in order); returns [job][rank] -> npz"""
    assert os.path.exists(FAKE), "tests/fake_rccl/librccl_fake.so is built by `make` (__graft_entry__.build)"
    for j, job in enumerate(jobs):
        job["out"] = str(tmp_path / ("%s_j%d_r%%d.npz" % (tag, j)))
    spec = str(tmp_path / ("%s.json" % tag))
    with open(spec, "w") as f:
        json.dump(jobs, f)
    env = dict(os.environ, AGZ_RCCL_LIB=FAKE)
    procs = [subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, "-c", WORKER, str(r), str(n), spec], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
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
    return [[np.load(job["out"] % r) for r in range(n)] for job in jobs]


def batch_shaped(name):
    return name.endswith(("_gamma", "_beta", "_b"))


def oracle_pair(K, L, FC, W, H, F, Aspace, B, seed=5, wscale=3.0):
    """the oracle trainer of test_train_gpu.make_pair (non-trivial gamma / beta / biases) and its global parameter arrays"""
    ot = O.TrainNet(K, L, FC, W, H, F, Aspace, B)
    ot.init_random(seed)
    rng = np.random.default_rng(seed)
    for i in range(ot.num_params()):
        nm = ot.param_name(i)
        p = ot.get_param(i)
        if nm.endswith("_gamma"):
            p = rng.uniform(0.5, 1.5, p.size).astype(np.float32)
        elif nm.endswith("_beta") or nm.endswith("_b"):
            p = rng.normal(0, 0.1, p.size).astype(np.float32)
        else:
            p = (p * wscale).astype(np.float32)
        ot.set_param(i, p)
    return ot, {"p%d" % i: ot.get_param(i) for i in range(ot.num_params())}


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


def check_grads_against_oracle(ot, R, n, label):
    """every gradient within 2e-5 * max|g| + 1e-7 of the oracle's global tensor: batch-shaped rows per rank, shared tensors in full; cost
    and shared gradients bit-identical across ranks"""
    co = None
    for r in range(n):
        assert R[r]["cost"].tobytes() == R[0]["cost"].tobytes(), (label, "cost differs between ranks")
    for i in range(ot.num_params()):
        nm = ot.param_name(i)
        go = ot.get_grad(i)
        scale = float(np.abs(go).max())
        for r in range(n):
            gd = R[r]["g%d" % i]
            ref = rank_slice(go, r, n) if batch_shaped(nm) else go
            assert gd.size == ref.size, (label, nm)
            err = float(np.abs(gd - ref).max())
            assert err <= 2e-5 * scale + 1e-7, (label, nm, r, err, scale)
            if not batch_shaped(nm):
                assert gd.tobytes() == R[0]["g%d" % i].tobytes(), (label, nm, "shared gradient differs between ranks")
    return co


FB_CASES = [
    # K, L, FC, W, H, F, A, B per rank
    (32, 1, 16, 3, 3, 2, 10, 4),
    (3, 3, 8, 3, 3, 2, 10, 5),        # K padded 3 -> 32
    (20, 1, 8, 4, 4, 2, 17, 1),       # one row per rank: BatchNorm statistics only exist across the ranks
    (40, 2, 24, 5, 4, 3, 21, 7),
]
# 4332 rows per rank: the single-pass k_bn_stats path.  f32 only: at this shape (3x Glorot filters, 24 boards) AGZ_COMPUTE_WINO_H2 misses the
# 2e-5 bar on the PLAIN trainer as well (5.7e-3 of a beta gradient's maximum at the global batch: its fp16x2 forward flips ReLU units).
# The single-GPU answer to that is tests/test_train_rows_gpu.py: at thousands of rows some unit lies within fp32 rounding of zero on every
# draw, and the fp32 oracle flips units of its own; there the draws are conditioned (f64_train.condition) and float64 is the only judge, and
# AGZ_COMPUTE_WINO_H2 holds the bar from 2 048 to 65 910 rows.
BIG = (64, 2, 32, 19, 19, 18, 362, 12)


@pytest.mark.parametrize("n", [2, 3])
def test_forward_backward_matches_the_oracle_at_the_global_batch(n, tmp_path):
    cases = list(FB_CASES) + ([BIG] if n == 2 else [])
    jobs, refs = [], []
    for ci, (K, L, FC, W, H, F, Aspace, B) in enumerate(cases):
        Bg = n * B
        ot, params = oracle_pair(K, L, FC, W, H, F, Aspace, Bg)
        x, pi, v = batch_data(Bg, F, H, W, Aspace, seed=K + Bg)
        co = ot.batch(x, pi, v, lr=0.0)
        path = str(tmp_path / ("fb%d.npz" % ci))
        np.savez(path, x=x, pi=pi, v=v, **params)
        for mode in ("f32", "wino_h2") if B < 12 else ("f32",):
            jobs.append({"kind": "fb", "conf": [K, L, FC, W, H, F, Aspace, Bg], "inp": path, "mode": mode})
            refs.append((ot, co, (K, L, FC, W, H, F, Aspace, B), mode))
    out = run_ranks(n, jobs, tmp_path, "fb")
    for (ot, co, case, mode), R in zip(refs, out):
        label = (case, mode, n)
        for r in range(n):
            assert list(R[r]["shard"]) == [r * case[-1], case[-1], n], label
        cd = float(R[0]["cost"])
        assert abs(cd - co) <= 1e-5 * max(1.0, abs(co)), (label, cd, co)
        check_grads_against_oracle(ot, R, n, label)


@pytest.mark.parametrize("n", [2, 3])
def test_three_sgd_steps_and_export_match_the_oracle(n, tmp_path):
    K, L, FC, W, H, F, Aspace, B = 32, 2, 32, 5, 5, 2, 26, 2
    Bg = n * B
    ot, params = oracle_pair(K, L, FC, W, H, F, Aspace, Bg, seed=9)
    data = {}
    costs = []
    for s in range(3):
        x, pi, v = batch_data(Bg, F, H, W, Aspace, seed=100 + s)
        data.update({"x%d" % s: x, "pi%d" % s: pi, "v%d" % s: v})
        costs.append(ot.batch(x, pi, v, lr=0.1))
    path = str(tmp_path / "sgd.npz")
    np.savez(path, **data, **params)
    R = run_ranks(n, [{"kind": "sgd", "conf": [K, L, FC, W, H, F, Aspace, Bg], "inp": path}], tmp_path, "sgd")[0]
    for r in range(n):
        assert R[r]["costs"].tobytes() == R[0]["costs"].tobytes()
    for s in range(3):
        assert abs(float(R[0]["costs"][s]) - costs[s]) <= 2e-5 * max(1.0, abs(costs[s])), (s, R[0]["costs"][s], costs[s])
    for i in range(ot.num_params()):
        nm = ot.param_name(i)
        po = ot.get_param(i)
        scale = float(np.abs(po).max())
        for r in range(n):
            ref = rank_slice(po, r, n) if batch_shaped(nm) else po
            assert float(np.abs(R[r]["p%d" % i] - ref).max()) <= 1e-4 * scale + 1e-7, (nm, r)
            if not batch_shaped(nm):
                assert R[r]["p%d" % i].tobytes() == R[0]["p%d" % i].tobytes(), (nm, "replicas of a shared tensor differ")
    # export: every rank's net is rank 0's row 0, bit for bit, and that row is the oracle's row 0
    onet = O.Net(K, L, FC, W, H, F, Aspace, bn_mode=2)
    for i in range(onet.num_params()):
        ref = ot.get_param(i)[: onet.get_param(i).size]
        scale = float(np.abs(ref).max())
        for r in range(n):
            assert R[r]["n%d" % i].tobytes() == R[0]["n%d" % i].tobytes(), (i, r)
        assert float(np.abs(R[0]["n%d" % i] - ref).max()) <= 1e-4 * scale + 1e-7, i


def test_one_rank_is_the_plain_trainer_bit_for_bit(tmp_path):
    """(54 rows: every reduction of the step runs in one workgroup, so that the plain trainer itself is deterministic to the bit)"""
    jobs = []
    for ci, ((K, L, FC, W, H, F, Aspace, B), mode) in enumerate([((32, 2, 24, 3, 3, 2, 10, 6), "f32"), ((64, 2, 24, 3, 3, 2, 10, 6), "wino_h2")]):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=3 + ci)
        path = str(tmp_path / ("id%d.npz" % ci))
        np.savez(path, x=x, pi=pi, v=v)
        jobs.append({"kind": "identity", "conf": [K, L, FC, W, H, F, Aspace, B], "inp": path, "seed": 21 + ci, "mode": mode})
    for job, R in zip(jobs, run_ranks(1, jobs, tmp_path, "id")):
        R = R[0]
        assert list(R["shard"]) == [0, job["conf"][7], 1]
        assert R["cost"][0].tobytes() == R["cost"][1].tobytes() and R["cost_b"][0].tobytes() == R["cost_b"][1].tobytes(), job
        n_p = len([k for k in R.files if k.startswith("gs")])
        for i in range(n_p):
            assert R["gs%d" % i].tobytes() == R["gp%d" % i].tobytes(), (job["mode"], "gradient", i)
            assert R["ps%d" % i].tobytes() == R["pp%d" % i].tobytes(), (job["mode"], "parameter", i)


@pytest.mark.parametrize("n", [2, 3])
def test_initialisation_checkpoints_and_refusals(ctx, n, tmp_path):
    K, L, FC, W, H, F, Aspace, B = 32, 1, 16, 3, 3, 2, 10, 3      # odd slices: the Box-Muller pairs straddle the ranks' boundaries
    Bg = n * B
    plain = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    plain.init_random(77)
    init = [plain.get_param(i) for i in range(plain.num_params())]
    init_file = tmp_path / "init.agz"
    plain.save(init_file)
    plain.init_random(78)
    global_file = tmp_path / "global.agz"
    plain.save(global_file)
    second = [plain.get_param(i) for i in range(plain.num_params())]
    sharded_file = tmp_path / "sharded.agz"
    R = run_ranks(n, [{"kind": "misc", "conf": [K, L, FC, W, H, F, Aspace, Bg], "seed": 77, "save_to": str(sharded_file),
                       "load_from": str(global_file)}], tmp_path, "misc")[0]
    names = [plain.param_info(i)[0] for i in range(plain.num_params())]
    for r in range(n):
        for i, nm in enumerate(names):
            want = rank_slice(init[i], r, n) if batch_shaped(nm) else init[i]
            np.testing.assert_array_equal(R[r]["i%d" % i].view(np.uint32), want.view(np.uint32), err_msg="init %s rank %d" % (nm, r))
            want = rank_slice(second[i], r, n) if batch_shaped(nm) else second[i]
            np.testing.assert_array_equal(R[r]["l%d" % i].view(np.uint32), want.view(np.uint32), err_msg="load %s rank %d" % (nm, r))
        assert "(-1)" in str(R[r]["e_div"]) and "not a multiple" in str(R[r]["e_div"]), str(R[r]["e_div"])
        for k in ("e_ar", "e_fba", "e_fbad"):
            assert "(-4)" in str(R[r][k]), (k, str(R[r][k]))
    # the sharded save is a plain checkpoint at the global batch: the plain trainer's file byte for byte; it loads into a plain trainer
    # and holds the ranks' slices
    assert open(sharded_file, "rb").read() == open(init_file, "rb").read()
    plain.load(sharded_file)
    for i, nm in enumerate(names):
        np.testing.assert_array_equal(plain.get_param(i).view(np.uint32), init[i].view(np.uint32), err_msg=nm)


def test_train_dev_equals_the_plain_trainer_at_the_global_batch(ctx, tmp_path):
    n = 2
    K, L, FC, W, H, F, Aspace, B = 32, 1, 16, 3, 3, 2, 10, 4
    Bg = n * B
    ot, params = oracle_pair(K, L, FC, W, H, F, Aspace, Bg, seed=13, wscale=1.0)
    x, pi, v = batch_data(3 * Bg + 2, F, H, W, Aspace, seed=31)   # prepareExamples trims to 3 global batches
    path = str(tmp_path / "td.npz")
    np.savez(path, x=x, pi=pi, v=v, **params)
    R = run_ranks(n, [{"kind": "train_dev", "conf": [K, L, FC, W, H, F, Aspace, Bg], "inp": path, "seed": 5}], tmp_path, "td")[0]
    plain = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg)
    for i in range(plain.num_params()):
        plain.set_param(i, params["p%d" % i])
    ex = A.Examples(ctx, F, H, W, Aspace)
    ex.append_host(x, pi, v)
    batches = ex.prepare(Bg, 0, seed=77)
    assert batches == 3
    xd, pd, vd, _, _ = ex.tensors_dev()
    cp = plain.train_dev(xd, pd, vd, batches, 2, seed=5)
    assert R[0]["cost"].tobytes() == R[1]["cost"].tobytes()
    assert abs(float(R[0]["cost"]) - cp) <= 2e-5 * max(1.0, abs(cp)), (float(R[0]["cost"]), cp)
    for i in range(plain.num_params()):
        nm, _ = plain.param_info(i)
        pp = plain.get_param(i)
        scale = float(np.abs(pp).max())
        for r in range(n):
            ref = rank_slice(pp, r, n) if batch_shaped(nm) else pp
            assert float(np.abs(R[r]["p%d" % i] - ref).max()) <= 1e-4 * scale + 1e-7, (nm, r)


def test_a_failing_rank_does_not_hang_the_sharded_step(tmp_path):
    """one rank fails before the first, a middle and the last layer's exchange (and the heads'): every rank's call fails (AGZ_E_PEER = -7
    on the healthy one), nobody hangs, and the following step is an ordinary one with the same cost everywhere"""
    n, L = 2, 2
    K, FC, W, H, F, Aspace, B = 32, 16, 3, 3, 2, 10, 4
    x, pi, v = batch_data(n * B, F, H, W, Aspace, seed=8)
    path = str(tmp_path / "fail.npz")
    np.savez(path, x=x, pi=pi, v=v)
    layers = [0, 1, L, L + 1]
    R = run_ranks(n, [{"kind": "fail", "conf": [K, L, FC, W, H, F, Aspace, n * B], "inp": path, "layers": layers, "bad_rank": 1}],
                  tmp_path, "fail")[0]
    for k, layer in enumerate(layers):
        for r in range(n):
            msg = str(R[r]["msg%d" % k])
            if r == 1:
                assert "(-4)" in msg and "injected failure before the exchange of layer %d" % layer in msg, msg
            else:
                assert "(-7)" in msg and "another rank failed" in msg, msg
            assert R[r]["next%d" % k].tobytes() == R[0]["next%d" % k].tobytes() and np.isfinite(R[r]["next%d" % k])
        assert R[0]["next%d" % k].tobytes() == R[0]["clean"].tobytes(), k   # the same parameters and data as the step before any failure


def test_learn_epoch_sharded_two_ranks_end_to_end():
    """scripts/learn_epoch_sharded.py: sharded self-play -> example all-gather -> shared-seed prepareExamples -> train_dev on the
    sharded trainer -> SwitchToInference -> arena; two ranks on GPU 0 (tests/fake_rccl)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", AGZ_RCCL_LIB=FAKE)
    out = subprocess.run(["timeout", "-k", "10", "280", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29613", os.path.join(ROOT, "scripts", "learn_epoch_sharded.py"),
                          "--shared-gpu"], capture_output=True, text=True, timeout=300, env=env)
    line = [l for l in out.stdout.splitlines() if l.startswith("{") and "LEARN_EPOCH_SHARDED" in l]
    assert line, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(line[-1])
    assert r["LEARN_EPOCH_SHARDED"] == "OK" and r["world"] == 2
    assert r["shared_identical"] and r["nets_identical"] and r["train_steps"] >= 2
    assert r["arena"]["a_wins"] + r["arena"]["b_wins"] + r["arena"]["draws"] == 32
