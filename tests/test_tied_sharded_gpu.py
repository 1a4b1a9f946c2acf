"""GPU: the tied sharded trainer (agz_trainer_create_sharded_tied; include/agz.h, DESIGN §2 `tied-affine`, §7) — the tied trainer at the GLOBAL
batch over n ranks, every rank holding every tied tensor whole.  Ranks are processes on GPU 0 through tests/fake_rccl (AGZ_RCCL_LIB), as in
test_train_sharded_gpu.py: every rank process runs a list of jobs over one communicator and saves what it computed, this process compares.

References: test_tied_sharded_cpu.oracle_tied_ranks — the oracle's per-row gradients summed as the declared definition says (and, from the same
oracle run, test_tied_cpu.oracle_tied's plain row sum, which it equals to one float ulp) — with the bars of test_tied_gpu.py; the
single-process tied trainer at the global batch (trajectories, checkpoints, eval), with the bars of the sharded SGD test; and bytes wherever
the definition promises the same bits: across ranks, one rank against the tied trainer, the forward against the untied sharded trainer's,
the fused step against the two-pass step.  Shapes: test_tied_sharded_cpu.S1 .. S4."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from test_tied_cpu import batch_data, draw_tied, is_batch_shaped
from test_tied_sharded_cpu import GRADIENT_CASES, S1, S3, S3_WINO, oracle_tied_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")
MODES = {"f32": capi.COMPUTE_F32_MFMA, "wino_h2": capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE}
B1, B2 = 0.9, 0.999
KINDS = ["vanilla", "l2clip", "momentum", "adam"]

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

def err(fn):
    try:
        fn()
    except A.AgzError as e:
        return str(e)
    return ""

def make(job, inp=None):
    t = A.Trainer.sharded(ctx, comm, *job["conf"], tied=True)
    if job.get("mode"):
        t.set_compute_mode(MODES[job["mode"]])
    if inp is not None:
        for i in range(t.num_params()):
            t.set_param(i, inp["p%d" % i])          # whole tied tensors, the same on every rank
    return t

def configure(t, kind, eps):
    if kind == "l2clip":
        t.set_solver(0, 1e-4, 10 * eps)
    elif kind == "momentum":
        t.set_solver(0.9, 1e-4, 0)
    elif kind == "adam":
        t.set_adam(0.9, 0.999, eps)
        t.set_solver(0, 1e-4, 0)

def state(t, res, tag):
    for i in range(t.num_params()):
        res["%sp%d" % (tag, i)] = t.get_param(i)
        res["%sv%d" % (tag, i)] = t.get_velocity(i)
        m1, m2 = t.get_moments(i)
        res["%sm%d" % (tag, i)], res["%su%d" % (tag, i)] = m1, m2
    res["%st" % tag] = np.int64(t.get_adam()["t"])

for ji, job in enumerate(jobs):
    K, L, FC, W, H, F, Aspace, Bg = job["conf"]
    inp = np.load(job["inp"]) if job.get("inp") else None
    res = {}
    kind = job["kind"]
    if kind == "fb":
        t = make(job, inp)
        r0, B, nr = t.shard()
        res["shard"] = np.array([r0, B, nr, int(t.is_tied())])
        res["cost"] = np.float32(t.forward_backward(rows(inp["x"], r0, B), rows(inp["pi"], r0, B), rows(inp["v"], r0, B)))
        for i in range(t.num_params()):
            res["g%d" % i] = t.get_grad(i)
        t.close()
    elif kind == "identity":   # n = 1: the tied sharded trainer against the tied trainer, bit for bit
        t = make(job)
        pt = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg, tied=True)
        pt.set_compute_mode(MODES[job["mode"]])
        for tt in (t, pt):
            tt.init_random(job["seed"])
        x, pi, v = inp["x"], inp["pi"], inp["v"]
        res["shard"] = np.array(list(t.shard()) + [int(t.is_tied())])
        res["cost"] = np.array([t.forward_backward(x, pi, v), pt.forward_backward(x, pi, v)], np.float32)
        for i in range(t.num_params()):
            res["gs%d" % i], res["gp%d" % i] = t.get_grad(i), pt.get_grad(i)
        res["cost_b"] = np.array([t.batch(x, pi, v, lr=0.1), pt.batch(x, pi, v, lr=0.1)], np.float32)
        for i in range(t.num_params()):
            res["ps%d" % i], res["pp%d" % i] = t.get_param(i), pt.get_param(i)
        pt.close()
        t.close()
    elif kind == "forward":    # the tied handle and a plain sharded handle holding the tied tensor in every row, on one communicator
        t = make(job, inp)
        u = A.Trainer.sharded(ctx, comm, *job["conf"])
        r0, B, nr = t.shard()
        for i in range(u.num_params()):
            name, _ = u.param_info(i)
            u.set_param(i, np.tile(inp["p%d" % i], B) if batch_shaped(name) else inp["p%d" % i])
        x, pi, v = rows(inp["x"], r0, B), rows(inp["pi"], r0, B), rows(inp["v"], r0, B)
        res["cost"] = np.array([t.forward_backward(x, pi, v), u.forward_backward(x, pi, v)], np.float32)
        u.close()
        t.close()
    elif kind == "fused":      # batch(lr) against forward_backward + apply(lr, 1) from the same state, two steps of every solver
        for sk in job["solvers"]:
            f, p = make(job, inp), make(job, inp)
            r0, B, nr = f.shard()
            lr = 0.1 * job["eps"] if sk == "adam" else 0.1
            for tt in (f, p):
                configure(tt, sk, job["eps"])
            for s in range(2):
                x, pi, v = rows(inp["x%d" % s], r0, B), rows(inp["pi%d" % s], r0, B), rows(inp["v%d" % s], r0, B)
                f.batch(x, pi, v, lr=lr)
                p.forward_backward(x, pi, v)
                p.apply(lr, 1.0)
            state(f, res, sk + "_f_")
            state(p, res, sk + "_p_")
            f.close()
            p.close()
    elif kind == "traj":       # three steps of every solver
        for sk in job["solvers"]:
            t = make(job, inp)
            r0, B, nr = t.shard()
            configure(t, sk, job["eps"])
            costs = []
            for s in range(3):
                costs.append(t.batch(rows(inp["x%d" % s], r0, B), rows(inp["pi%d" % s], r0, B), rows(inp["v%d" % s], r0, B), lr=job["lr"][sk]))
            res[sk + "_costs"] = np.array(costs, np.float32)
            state(t, res, sk + "_")
            t.close()
    elif kind == "state":      # initialisation, checkpoints both ways, refusals, export, eval
        t = make(job)
        r0, B, nr = t.shard()
        t.init_random(job["seed"])
        for i in range(t.num_params()):
            res["i%d" % i] = t.get_param(i)
        t.save(job["save_to"])
        t.load(job["load_tied"])
        for i in range(t.num_params()):
            res["l%d" % i] = t.get_param(i)
        res["e_plain"] = np.array(err(lambda: t.load(job["load_plain"])))
        for i in range(t.num_params()):
            res["u%d" % i] = t.get_param(i)
        u = A.Trainer.sharded(ctx, comm, *job["conf"])
        u.init_random(5)
        before = [u.get_param(i).tobytes() for i in range(u.num_params())]
        res["e_tied"] = np.array(err(lambda: u.load(job["load_tied"])))
        res["plain_untouched"] = np.array(before == [u.get_param(i).tobytes() for i in range(u.num_params())])
        u.close()
        net = A.Net(ctx, K, L, FC, W, H, F, Aspace, bn_mode=capi.BN_IDENTITY)
        t.export(net)
        for i in range(net.num_params()):
            res["n%d" % i] = net.get_param(i)
        net.close()
        x, pi, v = rows(inp["x"], r0, B), rows(inp["pi"], r0, B), rows(inp["v"], r0, B)
        res["e_ar"] = np.array(err(lambda: comm.allreduce_trainer(t)))
        res["e_fba"] = np.array(err(lambda: comm.forward_backward_allreduce(t, x, pi, v)))
        gp, _ = t.grads_dev()
        res["e_fbad"] = np.array(err(lambda: comm.forward_backward_allreduce_dev(t, gp, gp, gp)))
        t.set_bn_tracking(True, 0.9)
        res["cost"] = np.float32(t.forward_backward(x, pi, v))
        res["eval"] = np.float32(t.eval(x, pi, v))
        t.close()
    elif kind == "fail":       # a failure on one rank before a site's first exchange; the next step is an ordinary one
        t = make(job)
        r0, B, nr = t.shard()
        t.init_random(3)
        x, pi, v = rows(inp["x"], r0, B), rows(inp["pi"], r0, B), rows(inp["v"], r0, B)
        res["clean"] = np.float32(t.forward_backward(x, pi, v))
        for k, layer in enumerate(job["layers"]):
            if rank == job["bad_rank"]:
                comm.debug_fail_layer(layer)
            res["msg%d" % k] = np.array(err(lambda: t.forward_backward(x, pi, v)))
            res["next%d" % k] = np.float32(t.forward_backward(x, pi, v))
        for i in range(t.num_params()):
            res["g%d" % i] = t.get_grad(i)
        t.close()
    np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


def run_ranks(n, jobs, tmp_path, tag, timeout=120):
    """n rank processes on GPU 0 run `jobs` (collectively, in order), each under its own time limit; returns [job][rank] -> npz"""
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


@functools.lru_cache(maxsize=None)
def reference(case):
    """the draw of test_tied_gpu.check_gradient at the global batch and ONE oracle run for every rank count: (names, P, x, pi, v, cost, G, R)"""
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B)
    cost, G, R = oracle_tied_ranks(case, names, P, x, pi, v, tuple(n for n in (1, 2, 3) if B % n == 0))
    return names, P, x, pi, v, cost, G, R


def save_inputs(path, P, **data):
    np.savez(path, **data, **{"p%d" % i: p for i, p in enumerate(P)})
    return str(path)


def same_on_every_rank(R, keys, label):
    for r in range(1, len(R)):
        for k in keys:
            assert R[r][k].tobytes() == R[0][k].tobytes(), (label, k, "rank %d differs from rank 0" % r)


def tied_single(ctx, case, P, mode="f32"):
    t = A.Trainer(ctx, *case, tied=True)
    t.set_compute_mode(MODES[mode])
    for i, p in enumerate(P):
        t.set_param(i, p)
    return t


def configure(t, kind, eps):
    if kind == "l2clip":
        t.set_solver(0, 1e-4, 10 * eps)
    elif kind == "momentum":
        t.set_solver(0.9, 1e-4, 0)
    elif kind == "adam":
        t.set_adam(B1, B2, eps)
        t.set_solver(0, 1e-4, 0)


# ---- 1. the gradient against the oracle at the global batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_gradient_is_the_rank_ordered_sum_of_the_oracles_rows_at_the_global_batch(ctx, n, tmp_path):
    cases = [(c, mode) for c, k, mode in GRADIENT_CASES if k == n]
    jobs = []
    for ci, (case, mode) in enumerate(cases):
        names, P, x, pi, v, _, _, _ = reference(case)
        jobs.append({"kind": "fb", "conf": list(case), "mode": mode, "inp": save_inputs(tmp_path / ("fb%d.npz" % ci), P, x=x, pi=pi, v=v)})
    for (case, mode), R in zip(cases, run_ranks(n, jobs, tmp_path, "fb")):
        names, P, x, pi, v, co, GO, RK = reference(case)
        label, Bl = (case, mode, n), case[-1] // n
        for r in range(n):
            assert list(R[r]["shard"]) == [r * Bl, Bl, n, 1], label
        same_on_every_rank(R, ["cost"] + ["g%d" % i for i in range(len(names))], label)   # tied gradients included
        cd = float(R[0]["cost"])
        print("case %s mode %s n %d: cost %.9g oracle %.9g" % (case, mode, n, cd, co))
        assert abs(cd - co) <= 1e-5 * max(1.0, abs(co)), (label, cd, co)
        missed, worst = [], 0.0
        for i, (nm, go, gk) in enumerate(zip(names, GO, RK[n])):
            gd = R[0]["g%d" % i]
            assert gd.shape == go.shape, (label, nm)
            scale = float(np.abs(go).max())
            err = max(float(np.abs(gd - go).max()), float(np.abs(gd - gk).max()))     # oracle_tied's row sum, and the declared order
            worst = max(worst, err / (2e-5 * scale + 1e-7))
            if err > 2e-5 * scale + 1e-7:
                missed.append((i, nm, err, scale))
        print("    worst tensor %.3f of the gradient bar" % worst)
        if missed:   # the rule of test_tied_gpu.check_gradient, against the single-process tied trainer at the global batch on the same draw
            st = tied_single(ctx, case, P, mode)
            st.forward_backward(x, pi, v)
            GS = [st.get_grad(i) for i in range(st.num_params())]
            st.close()
            for i, nm, err, scale in missed:
                es = float(np.abs(GS[i] - GO[i]).max())
                print("    %s: err_sharded %.3e err_tied %.3e scale %.3e" % (nm, err, es, scale))
                assert err <= 2 * es, (label, nm, err, es, scale)
        assert any(np.abs(g).max() > 1e-6 for nm, g in zip(names, GO) if is_batch_shaped(nm))


# ---- 2. one rank is the tied trainer -----------------------------------------------------------------------------------------------------------
def test_one_rank_is_the_tied_trainer_bit_for_bit(tmp_path):
    jobs = []
    for ci, (case, mode) in enumerate([(S3, "f32"), (S3_WINO, "wino_h2")]):
        K, L, FC, W, H, F, Aspace, B = case
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=3 + ci)
        path = str(tmp_path / ("id%d.npz" % ci))
        np.savez(path, x=x, pi=pi, v=v)
        jobs.append({"kind": "identity", "conf": list(case), "inp": path, "seed": 21 + ci, "mode": mode})
    for job, R in zip(jobs, run_ranks(1, jobs, tmp_path, "id")):
        R = R[0]
        assert list(R["shard"]) == [0, job["conf"][7], 1, 1]
        assert R["cost"][0].tobytes() == R["cost"][1].tobytes() and R["cost_b"][0].tobytes() == R["cost_b"][1].tobytes(), job
        n_p = len([k for k in R.files if k.startswith("gs")])
        assert any(R["gs%d" % i].any() for i in range(n_p))
        for i in range(n_p):
            assert R["gs%d" % i].tobytes() == R["gp%d" % i].tobytes(), (job["mode"], "gradient", i)
            assert R["ps%d" % i].tobytes() == R["pp%d" % i].tobytes(), (job["mode"], "parameter", i)


# ---- 3. the forward is the untied sharded forward; 4. fused = two-pass -----------------------------------------------------------------------
def test_forward_is_the_untied_sharded_forward_and_the_fused_step_is_the_two_pass_step_to_the_bit(tmp_path):
    n, case = 2, S3
    K, L, FC, W, H, F, Aspace, B = case
    names, P, x, pi, v, _, GO, _ = reference(case)
    eps = float(np.median(np.concatenate([np.abs(g) for g in GO])))      # (test_tied_gpu.tied_eps_star's scale, from the oracle)
    assert eps > 0
    data = {}
    for s in range(2):
        xs, ps, vs = batch_data(B, F, H, W, Aspace, seed=300 + s)
        data.update({"x%d" % s: xs, "pi%d" % s: ps, "v%d" % s: vs})
    inp = save_inputs(tmp_path / "s3.npz", P, x=x, pi=pi, v=v, **data)
    fwd, fused = run_ranks(n, [{"kind": "forward", "conf": list(case), "inp": inp},
                               {"kind": "fused", "conf": list(case), "inp": inp, "solvers": KINDS, "eps": eps}], tmp_path, "s3")
    for r in range(n):
        assert fwd[r]["cost"][0].tobytes() == fwd[r]["cost"][1].tobytes() == fwd[0]["cost"][0].tobytes(), (r, fwd[r]["cost"])
    for kind in KINDS:
        for r in range(n):
            R = fused[r]
            for i, nm in enumerate(names):
                for what in "pvmu":
                    a, b = R["%s_f_%s%d" % (kind, what, i)], R["%s_p_%s%d" % (kind, what, i)]
                    assert a.tobytes() == b.tobytes(), (kind, r, nm, what)
                    assert a.tobytes() == fused[0]["%s_f_%s%d" % (kind, what, i)].tobytes(), (kind, r, nm, what, "ranks differ")
                assert R["%s_f_p%d" % (kind, i)].tobytes() != P[i].tobytes(), (kind, nm, "did not move")
            assert int(R[kind + "_f_t"]) == int(R[kind + "_p_t"]) == (2 if kind == "adam" else 0)
        if kind == "momentum":
            assert all(fused[0]["momentum_f_v%d" % i].any() for i in range(len(names)))
        if kind == "adam":
            assert all(fused[0]["adam_f_u%d" % i].any() for i in range(len(names)))


# ---- 5. trajectories against the single-process tied trainer at the global batch ---------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_three_steps_of_every_solver_follow_the_tied_trainer_at_the_global_batch(ctx, n, tmp_path):
    case = S1
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case, seed=9, wscale=1.0)
    _, _, _, _, _, _, GO, _ = reference(case)
    eps = float(np.median(np.concatenate([np.abs(g) for g in GO])))
    lr = {"vanilla": 0.1, "momentum": 0.02, "adam": 1e-3}
    data, steps = {}, []
    for s in range(3):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=100 + s)
        steps.append((x, pi, v))
        data.update({"x%d" % s: x, "pi%d" % s: pi, "v%d" % s: v})
    inp = save_inputs(tmp_path / "traj.npz", P, **data)
    R = run_ranks(n, [{"kind": "traj", "conf": list(case), "inp": inp, "solvers": list(lr), "eps": eps, "lr": lr}], tmp_path, "traj")[0]
    for kind in lr:
        st = tied_single(ctx, case, P)
        configure(st, kind, eps)
        costs = [st.batch(x, pi, v, lr=lr[kind]) for x, pi, v in steps]
        same_on_every_rank(R, [kind + "_costs", kind + "_t"] + ["%s_%s%d" % (kind, w, i) for w in "pvmu" for i in range(len(names))], (kind, n))
        for s in range(3):
            assert abs(float(R[0][kind + "_costs"][s]) - costs[s]) <= 2e-5 * max(1.0, abs(costs[s])), (kind, s, R[0][kind + "_costs"][s], costs[s])
        worst = 0.0
        for i, nm in enumerate(names):
            ps = st.get_param(i)
            scale, err = float(np.abs(ps).max()), float(np.abs(R[0]["%s_p%d" % (kind, i)] - ps).max())
            worst = max(worst, err / (1e-4 * scale + 1e-7))
            assert err <= 1e-4 * scale + 1e-7, (kind, nm, err, scale)
            assert ps.tobytes() != P[i].tobytes(), (kind, nm, "did not move")
        assert int(R[0][kind + "_t"]) == st.get_adam()["t"] == (3 if kind == "adam" else 0)
        print("%s, n = %d: worst parameter error %.3f of the bar" % (kind, n, worst))
        st.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------------
def test_initialisation_checkpoints_export_refusals_and_eval(ctx, tmp_path):
    n, case = 2, (32, 1, 16, 3, 3, 2, 10, 6)
    K, L, FC, W, H, F, Aspace, B = case
    st = A.Trainer(ctx, *case, tied=True)
    st.init_random(77)
    init = [st.get_param(i) for i in range(st.num_params())]
    names = [st.param_info(i)[0] for i in range(st.num_params())]
    init_file, tied_file, plain_file, sharded_file = (str(tmp_path / f) for f in ("init.agz", "tied.agz", "plain.agz", "sharded.agz"))
    st.save(init_file)
    st.init_random(78)
    st.save(tied_file)
    second = [st.get_param(i) for i in range(st.num_params())]
    plain = A.Trainer(ctx, *case)
    plain.init_random(78)
    plain.save(plain_file)
    plain.close()
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=41)
    path = str(tmp_path / "state.npz")
    np.savez(path, x=x, pi=pi, v=v)
    R = run_ranks(n, [{"kind": "state", "conf": list(case), "inp": path, "seed": 77, "save_to": sharded_file, "load_tied": tied_file,
                       "load_plain": plain_file}], tmp_path, "state")[0]
    for r in range(n):
        for i, nm in enumerate(names):
            assert R[r]["i%d" % i].tobytes() == init[i].tobytes(), ("init_random", nm, r)
            assert R[r]["l%d" % i].tobytes() == second[i].tobytes(), ("load", nm, r)
            assert R[r]["u%d" % i].tobytes() == second[i].tobytes(), ("a refused load touched", nm, r)
            assert R[r]["n%d" % i].tobytes() == second[i].tobytes(), ("export", nm, r)
        for k in ("e_plain", "e_tied"):
            assert "(-1)" in str(R[r][k]) and "checkpoint of a" in str(R[r][k]), (k, str(R[r][k]))
        assert "sharded_tied" in str(R[r]["e_tied"]) and bool(R[r]["plain_untouched"])
        for k in ("e_ar", "e_fba", "e_fbad"):
            assert "(-4)" in str(R[r][k]), (k, str(R[r][k]))
    assert open(sharded_file, "rb").read() == open(init_file, "rb").read()
    # eval under the tracked estimates of one training forward: the same bits on every rank, the single-process tied trainer's value
    st.set_bn_tracking(True, 0.9)
    cost = st.forward_backward(x, pi, v)
    ev = st.eval(x, pi, v)
    st.close()
    same_on_every_rank(R, ["cost", "eval"], "eval")
    assert abs(float(R[0]["cost"]) - cost) <= 2e-5 * max(1.0, abs(cost)), (float(R[0]["cost"]), cost)
    assert abs(float(R[0]["eval"]) - ev) <= 2e-5 * max(1.0, abs(ev)), (float(R[0]["eval"]), ev)


# ---- 7. a failing rank ---------------------------------------------------------------------------------------------------------------------------
def test_a_failing_rank_does_not_hang_the_tied_sharded_step(tmp_path):
    """one rank fails before the first exchange of layer 0, of layer L and of the heads: every gather behind it — the grown backward gathers
    among them — is entered in place by the communicator's catch-up loop; every rank's call fails (AGZ_E_PEER = -7 on the healthy one),
    nobody hangs, and the following step is an ordinary one.
    Only the no-hang property of the two-pass step (forward_backward) is covered.  A FUSED step (batch, train_dev) that fails part-way is not
    driven here: the healthy rank then steps gamma / beta from a gather its peer entered in place with undefined contents, so the replicated
    state after it is undefined by contract (include/agz.h: every rank reloads a checkpoint) and there is nothing to compare."""
    n, L = 2, 2
    K, FC, W, H, F, Aspace, B = 32, 16, 3, 3, 2, 10, 4
    x, pi, v = batch_data(n * B, F, H, W, Aspace, seed=8)
    path = str(tmp_path / "fail.npz")
    np.savez(path, x=x, pi=pi, v=v)
    layers = [0, L, L + 1]
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
    n_p = len([k for k in R[0].files if k.startswith("g")])
    same_on_every_rank(R, ["g%d" % i for i in range(n_p)], "gradients after the failures")
    assert all(np.isfinite(R[0]["g%d" % i]).all() for i in range(n_p))
