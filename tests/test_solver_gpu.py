"""GPU: the trainer's solver options (agz_trainer_set_solver: momentum, L2, clip), fused into the BatchNorm backward kernel for the
batch-shaped gamma / beta and swept by k_solver_sweep for everything else.

The contract (include/agz.h), per learnable element in fp32:
    g1 = grad_scale * g;  g2 = g1 + l2 * w (l2 != 0);  g3 = clamp(g2, -c, c) (c > 0)
    mu == 0: w += (-lr) * g3          mu != 0: v = mu * v + (-lr) * g3, w += v      (v starts at 0)
Bars: the element-wise recurrence 8 * 2^-24 * (|w| + |v| + lr |g3|) (each operation rounds to half an ulp, at most five are chained, and
the device may contract multiply-adds where numpy does not); fused against two-pass 3 * max(e0, 2e-6) with e0 the vanilla pair's own
difference in the same run; against the oracle the bars of test_train_gpu.test_sgd_steps_and_export."""
import os

import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi

pytestmark = pytest.mark.gpu

CASES = [
    # K, L, FC, W, H, F, A, B  (the shapes of test_train_gpu.CASES)
    (32, 1, 16, 3, 3, 2, 10, 4),
    (32, 2, 64, 5, 5, 2, 26, 6),
    (64, 2, 64, 7, 6, 2, 8, 5),
    (128, 1, 64, 9, 9, 18, 82, 3),
    (3, 3, 8, 3, 3, 2, 10, 5),
    (20, 1, 8, 4, 4, 2, 17, 1),
    (40, 2, 24, 5, 4, 3, 21, 7),
    (64, 1, 16, 16, 17, 3, 273, 2),
]
HEADLINE = (256, 1, 32, 19, 19, 18, 362, 2)      # the width and board of the measured step, one dual block, AGZ_COMPUTE_WINO_H2
DETERMINISTIC = (32, 2, 24, 3, 3, 2, 10, 6)      # 54 rows: every reduction of a step runs in one workgroup, a step is reproducible to the bit
FUSED_CASE = (64, 2, 32, 7, 7, 2, 50, 6)         # test_fused_gamma_beta_step_equals_the_two_pass_step's
EPS = 8 * 2.0 ** -24


def make_pair(ctx, K, L, FC, W, H, F, Aspace, B, seed=5, wscale=3.0):
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
    dt = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, B)
    for i in range(ot.num_params()):
        dt.set_param(i, ot.get_param(i))
    return ot, dt


def make_dev(ctx, case, seed, mode=None, head_scale=1.0):
    """a device trainer alone: the library's initialiser for the filters and FC weights, make_pair's draws for gamma / beta / biases
    (head_scale: the gamma / beta of the two head BatchNorms times this)"""
    dt = A.Trainer(ctx, *case)
    if mode == "wino_h2":
        dt.set_compute_mode(capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE)
    dt.init_random(seed)
    rng = np.random.default_rng(seed)
    for i in range(dt.num_params()):
        nm, n = dt.param_info(i)
        hs = np.float32(head_scale if nm.startswith(("PolicyHead_", "ValueHead_")) else 1.0)
        if nm.endswith("_gamma"):
            dt.set_param(i, rng.uniform(0.5, 1.5, n).astype(np.float32) * hs)
        elif nm.endswith("_beta") or nm.endswith("_b"):
            dt.set_param(i, rng.normal(0, 0.1, n).astype(np.float32) * hs)
    return dt


def batch_data(B, F, H, W, Aspace, seed):
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, 0.0, 1.0, 0.001], np.float32), size=(B, F, H, W)).astype(np.float32)
    pi = np.zeros((B, Aspace), np.float32)
    pi[np.arange(B), rng.integers(0, Aspace, B)] = 1.0
    v = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=B).astype(np.float32)
    return x, pi, v


def params(t):
    return [t.get_param(i) for i in range(t.num_params())]


def velocities(t):
    return [t.get_velocity(i) for i in range(t.num_params())]


def solver_step(w, v, g, lr, gs, mu, l2, c):
    """the contract restated in float32 numpy; returns w', v', g3"""
    f = np.float32
    g = f(gs) * g
    if l2 != 0:
        g = g + f(l2) * w
    if c > 0:
        g = np.minimum(np.maximum(g, f(-c)), f(c))
    if mu != 0:
        v = f(mu) * v + f(-lr) * g
        w = w + v
    else:
        w = w + f(-lr) * g
    return w.astype(np.float32), v.astype(np.float32), g.astype(np.float32)


def rel_diff(a, b):
    """max |a - b| relative to the tensor's maximum (the form of test_fused_gamma_beta_step_equals_the_two_pass_step's bar)"""
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-3)


def v1_file_size(t):
    """AGZTRN01: magic, agz_net_conf (10 x 4 bytes), count, then {uint64 n, n floats} per tensor"""
    return 8 + 40 + 8 + sum(8 + 4 * t.param_info(i)[1] for i in range(t.num_params()))


# ---- 1. the default solver is the code that ran before the options existed ---------------------------------------------------------------
def _default_variants(ctx, case, seed):
    ts = [make_dev(ctx, case, seed) for _ in range(3)]
    ts[1].set_solver(0, 0, 0)
    ts[2].set_solver(0.9, 1e-4, 0.01)
    ts[2].set_solver(0, 0, 0)
    return ts


def test_default_solver_two_pass_path_is_bit_equal(ctx, tmp_path):
    """(on the shape whose step is reproducible to the bit: the gradients of the three trainers are then the same bits, and apply is
    deterministic given G)"""
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    ts = _default_variants(ctx, case, seed=21)
    for step in range(2):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        costs = []
        for t in ts:
            costs.append(t.forward_backward(x, pi, v))
            t.apply(0.1)
        assert costs[0] == costs[1] == costs[2], costs
    ref = params(ts[0])
    for k in (1, 2):
        for i, p in enumerate(params(ts[k])):
            assert p.tobytes() == ref[i].tobytes(), (k, ts[0].param_info(i)[0])
        for i, vel in enumerate(velocities(ts[k])):
            assert not vel.any(), (k, i)
        assert ts[k].get_solver() == {"momentum": 0.0, "l2reg": 0.0, "clip": 0.0}
        path = tmp_path / ("default%d.agz" % k)
        ts[k].save(path)
        assert open(path, "rb").read(8) == b"AGZTRN01" and os.path.getsize(path) == v1_file_size(ts[k])
    ts[0].save(tmp_path / "untouched.agz")
    assert open(tmp_path / "untouched.agz", "rb").read() == open(tmp_path / "default1.agz", "rb").read()


def test_default_solver_fused_path_is_the_vanilla_step(ctx):
    case = FUSED_CASE
    K, L, FC, W, H, F, Aspace, B = case
    ts = _default_variants(ctx, case, seed=21)
    for step in range(2):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        costs = [t.batch(x, pi, v, lr=0.1) for t in ts]
        assert abs(costs[1] - costs[0]) <= 1e-6 * max(1.0, abs(costs[0])) and abs(costs[2] - costs[0]) <= 1e-6 * max(1.0, abs(costs[0]))
    ref = params(ts[0])
    for k in (1, 2):
        for i, p in enumerate(params(ts[k])):
            d = rel_diff(p, ref[i])
            assert d <= 2e-6, (k, ts[0].param_info(i)[0], d)
        assert not any(vel.any() for vel in velocities(ts[k]))


# ---- 2. the recurrence, element by element ---------------------------------------------------------------------------------------------
OPTIONS = [(0.9, 0.0, 0.0), (0.0, 1e-4, 0.0), (0.0, 0.0, "c*"), (0.9, 1e-4, "c*")]


def check_recurrence(ctx, case, mu, l2, clip, gs, mode=None, steps=2, lr=0.1):
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5, mode=mode)
    n = dt.num_params()
    fractions = []
    for step in range(steps):            # (the second step starts from a non-zero velocity)
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B + step)
        dt.forward_backward(x, pi, v)
        g = [dt.get_grad(i) for i in range(n)]
        c = clip
        if clip == "c*":                 # the median |g1| of the case: the clamp bites on about half of the elements
            c = float(np.median(np.concatenate([np.abs(np.float32(gs) * a) for a in g])))
            assert c > 0
        dt.set_solver(mu, l2, c)
        w0, v0 = params(dt), velocities(dt)
        dt.apply(lr, gs)
        w1, v1 = params(dt), velocities(dt)
        clamped = total = 0
        for i in range(n):
            we, ve, g3 = solver_step(w0[i], v0[i], g[i], lr, gs, mu, l2, c)
            bar = EPS * (np.abs(we) + np.abs(ve) + np.float32(lr) * np.abs(g3))
            name = dt.param_info(i)[0]
            dw, dv = np.abs(w1[i] - we), np.abs(v1[i] - ve)
            assert np.all(dw <= bar), (name, step, float((dw - bar).max()), float(dw.max()))
            assert np.all(dv <= bar), (name, step, float((dv - bar).max()), float(dv.max()))
            if mu == 0:
                assert not v1[i].any(), name
            if c > 0:
                clamped += int((np.abs(g3) == np.float32(c)).sum())
                total += g3.size
        if c > 0:
            fractions.append(clamped / total)
            assert 0.2 <= clamped / total <= 0.8, (step, clamped / total)
    return fractions


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("mu,l2,clip", OPTIONS)
@pytest.mark.parametrize("case", CASES)
def test_two_pass_step_is_the_recurrence_element_by_element(ctx, case, mu, l2, clip, gs):
    fr = check_recurrence(ctx, case, mu, l2, clip, gs)
    if fr:
        print("case %s options (%g, %g, c*), grad_scale %g: clamped fractions %s" % (case, mu, l2, gs, ["%.2f" % f for f in fr]))


# ---- 3. the fused step equals the two-pass step under momentum ---------------------------------------------------------------------------
def check_fused_equals_two_pass(ctx, case, seed, mode=None, mu=0.9, l2=1e-4, head_scale=1.0):
    K, L, FC, W, H, F, Aspace, B = case
    van_f, van_t, mom_f, mom_t = [make_dev(ctx, case, seed, mode=mode, head_scale=head_scale) for _ in range(4)]
    mom_f.set_solver(mu, l2, 0)
    mom_t.set_solver(mu, l2, 0)
    for step in range(3):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        van_f.batch(x, pi, v, lr=0.1)
        van_t.forward_backward(x, pi, v)
        van_t.apply(0.1)
        mom_f.batch(x, pi, v, lr=0.1)
        mom_t.forward_backward(x, pi, v)
        mom_t.apply(0.1)
    worst = (0.0, 0.0, 0.0)
    pf, pt, qf, qt = params(van_f), params(van_t), params(mom_f), params(mom_t)
    vf, vt = velocities(mom_f), velocities(mom_t)
    assert any(a.any() for a in vf)
    for i in range(len(pf)):
        e0 = rel_diff(pf[i], pt[i])            # the vanilla pair: the behaviour before the options existed, in this very run
        e = rel_diff(qf[i], qt[i])
        ev = rel_diff(vf[i], vt[i])
        worst = max(worst, (e, e0, ev))
        assert e <= 3 * max(e0, 2e-6), (van_f.param_info(i)[0], e, e0)
    print("fused vs two-pass, case %s mode %s: worst momentum pair %.2e (vanilla pair of that tensor e0 %.2e; its velocity %.2e)" %
          ((case, mode) + worst))


def test_fused_momentum_step_equals_the_two_pass_step(ctx):
    check_fused_equals_two_pass(ctx, FUSED_CASE, seed=21)


# ---- 4. against the oracle: numpy carries w, v over the oracle's gradients ---------------------------------------------------------------
def test_momentum_trajectory_matches_numpy_over_the_oracle(ctx):
    """Three steps of batch(lr) with momentum 0.9, L2 1e-4 against a trajectory the code under test has no part in: the oracle supplies
    the gradients (batch with lr = 0), float32 numpy carries w and v through the recurrence and sets the oracle's parameters each step.
    Bars: test_sgd_steps_and_export's (cost 2e-5, parameters 1e-4 * max|o| + 1e-7 per tensor).

    The case — CASES[0], seed 9, wscale 1.0, lr 0.02 — was fixed on the CPU beforehand: the numpy-over-oracle trajectory run twice, the second
    time with every gradient element perturbed by the project's gradient bar (2e-5 * max|g|, random signs), differs by 0.14 of the
    parameter bar and 0.32 of the cost bar (both <= 1/3: the bar measures the kernels, not the case's sensitivity).  At lr 0.1 the same
    case gives 0.42 / 0.61, and test_sgd_steps_and_export's own shape 0.52, so lr 0.1 was not used."""
    case = CASES[0]
    K, L, FC, W, H, F, Aspace, B = case
    mu, l2, lr = 0.9, 1e-4, 0.02
    ot, dt = make_pair(ctx, *case, seed=9, wscale=1.0)
    dt.set_solver(mu, l2, 0)
    n = ot.num_params()
    w = [ot.get_param(i) for i in range(n)]
    vel = [np.zeros_like(a) for a in w]
    for step in range(3):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=100 + step)
        co = ot.batch(x, pi, v, lr=0.0)
        for i in range(n):
            w[i], vel[i], _ = solver_step(w[i], vel[i], ot.get_grad(i), lr, 1.0, mu, l2, 0)
            ot.set_param(i, w[i])
        cd = dt.batch(x, pi, v, lr=lr)
        assert abs(cd - co) <= 2e-5 * max(1.0, abs(co)), (step, cd, co)
    worst = 0.0
    for i in range(n):
        pd = dt.get_param(i)
        scale = float(np.abs(w[i]).max())
        err = float(np.abs(pd - w[i]).max())
        worst = max(worst, err / (1e-4 * scale + 1e-7))
        assert err <= 1e-4 * scale + 1e-7, (ot.param_name(i), err, scale)
    print("momentum trajectory against numpy over the oracle: worst parameter error %.3f of the bar" % worst)


# ---- 5. the headline width in the mode the step is timed in ------------------------------------------------------------------------------
@pytest.mark.parametrize("mu,l2,clip", OPTIONS)
def test_recurrence_at_the_headline_width_wino_h2(ctx, mu, l2, clip):
    fr = check_recurrence(ctx, HEADLINE, mu, l2, clip, 1.0, mode="wino_h2")
    if fr:
        print("headline options (%g, %g, c*): clamped fractions %s" % (mu, l2, ["%.2f" % f for f in fr]))


def test_fused_momentum_step_at_the_headline_width_wino_h2(ctx):
    """The heads' BatchNorm gamma / beta are drawn 0.05 times make_pair's here.  On a 19x19 board the policy FC layer has 722 inputs: with
    inputs of order one, ONE lr-0.1 step moves a logit by lr * |input|^2 ~ 70, the cost goes 2.8 -> 146 -> 11776 over the three steps
    (vanilla as well as momentum), and two trainers on the SAME path then differ by 1e-2 of a tensor's maximum after the third step
    (the weight gradient's float atomics, amplified through flipping ReLU units; measured with two two-pass twins).  Such a trajectory
    compares nothing.  With inputs of order 0.05 the logit step is ~0.1, the cost stays of order one, same-path twins agree to 5e-7
    and the bar measures the two kernels."""
    check_fused_equals_two_pass(ctx, HEADLINE, seed=21, mode="wino_h2", head_scale=0.05)


# ---- 6. checkpoints -------------------------------------------------------------------------------------------------------------------------
def _run_steps(t, case, seeds, fused):
    K, L, FC, W, H, F, Aspace, B = case
    for s in seeds:
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=s)
        if fused:
            t.batch(x, pi, v, lr=0.1)
        else:
            t.forward_backward(x, pi, v)
            t.apply(0.1)


@pytest.mark.parametrize("fused", [False, True])
def test_checkpoint_carries_the_velocity(ctx, tmp_path, fused):
    case = DETERMINISTIC if not fused else FUSED_CASE
    t1 = make_dev(ctx, case, seed=5)
    t1.set_solver(0.9, 1e-4, 0)
    _run_steps(t1, case, (1, 2), fused)
    path = tmp_path / "mom.agz"
    t1.save(path)
    _run_steps(t1, case, (3, 4), fused)
    assert open(path, "rb").read(8) == b"AGZTRN02"
    assert os.path.getsize(path) == 2 * v1_file_size(t1) - 56 + 16      # the 01 payload, agz_solver_conf, {n, n floats} per tensor again
    t2 = A.Trainer(ctx, *case)
    t2.load(path)                                                       # a fresh trainer: the file carries the options
    got = t2.get_solver()
    assert got["momentum"] == np.float32(0.9) and got["l2reg"] == np.float32(1e-4) and got["clip"] == 0.0
    _run_steps(t2, case, (3, 4), fused)
    for i in range(t1.num_params()):
        name = t1.param_info(i)[0]
        for a, b in ((t1.get_param(i), t2.get_param(i)), (t1.get_velocity(i), t2.get_velocity(i))):
            if fused:
                assert rel_diff(b, a) <= 2e-6, name
            else:
                assert a.tobytes() == b.tobytes(), name
    # a file of the earlier format zeroes the velocity and keeps the options
    plain = make_dev(ctx, case, seed=6)
    old = tmp_path / "plain.agz"
    plain.save(old)
    assert open(old, "rb").read(8) == b"AGZTRN01"
    t2.load(old)
    assert t2.get_solver()["momentum"] == np.float32(0.9)
    for i in range(t2.num_params()):
        assert not t2.get_velocity(i).any()
        assert t2.get_param(i).tobytes() == plain.get_param(i).tobytes()
    # reset_solver: velocity := 0, options kept
    assert any(a.any() for a in velocities(t1))
    t1.reset_solver()
    assert not any(a.any() for a in velocities(t1)) and t1.get_solver()["momentum"] == np.float32(0.9)
    # a truncated 02 file is rejected and changes nothing
    blob = open(path, "rb").read()
    for cut in (len(blob) - 4, len(blob) // 2 + 8, v1_file_size(t1) + 8):
        bad = tmp_path / "truncated.agz"
        open(bad, "wb").write(blob[:cut])
        before = t2.get_param(0)
        with pytest.raises(A.AgzError, match=r"\(-1\)"):
            t2.load(bad)
        assert t2.get_param(0).tobytes() == before.tobytes()


# ---- 7. validation --------------------------------------------------------------------------------------------------------------------------
def test_invalid_options_are_refused_and_change_nothing(ctx):
    t = A.Trainer(ctx, *CASES[0])
    t.set_solver(0.5, 1e-3, 2.0)
    want = t.get_solver()
    nan, inf = float("nan"), float("inf")
    for bad in [(1.0, 0, 0), (-0.1, 0, 0), (0.9, -1e-4, 0), (0.9, 0, -1.0), (nan, 0, 0), (0, nan, 0), (0, 0, nan), (inf, 0, 0), (0, inf, 0),
                (0, 0, inf), (1.5, 0, 0)]:
        with pytest.raises(A.AgzError, match=r"\(-1\)"):
            t.set_solver(*bad)
        assert t.get_solver() == want, bad
    with pytest.raises(A.AgzError, match=r"\(-1\)"):
        t.set_solver(0.9, 0, 0, reserved=1)
    assert t.get_solver() == want
    n = t.param_info(1)[1]
    with pytest.raises(A.AgzError, match=r"\(-1\)"):
        t.set_velocity(1, np.zeros(n + 1, np.float32))
    # set_velocity / get_velocity round trip in the layout of get_param; no velocity without a momentum
    vals = np.arange(n, dtype=np.float32)
    t.set_velocity(1, vals)
    np.testing.assert_array_equal(t.get_velocity(1), vals)
    assert not t.get_velocity(2).any()
    t.set_solver(0, 1e-3, 0)
    assert not t.get_velocity(1).any()
    with pytest.raises(A.AgzError, match=r"\(-4\)"):
        t.set_velocity(1, vals)


# ---- 8. agz_train_dev -----------------------------------------------------------------------------------------------------------------------
def _splitmix(seed):
    s = seed & 0xFFFFFFFFFFFFFFFF
    M = 0xFFFFFFFFFFFFFFFF
    while True:
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        yield z ^ (z >> 31)


def test_train_dev_with_momentum_is_a_loop_of_batch(ctx):
    """dual.Train over device tensors with the options set == batch after batch in the same row order (shuffleBatch's Fisher-Yates over
    the build's SplitMix64, meta.go:57-102, restated here), under the fused path's bar"""
    case = (32, 1, 16, 3, 3, 2, 10, 8)        # test_agz_train_loop_runs_and_shuffles's
    K, L, FC, W, H, F, Aspace, B = case
    batches, iterations, seed = 3, 2, 11
    x, pi, v = batch_data(B * batches, F, H, W, Aspace, seed=1)
    ex = A.Examples(ctx, F, H, W, Aspace)
    ex.append_host(x, pi, v)
    assert ex.prepare(B, 0, seed=77) == batches
    xd, pd, vd, _, _ = ex.tensors_dev()
    xs, ps, vs = [np.array(a) for a in ex.tensors()]
    xs = xs.reshape(B * batches, F, H, W)
    t1, t2 = make_dev(ctx, case, seed=3), make_dev(ctx, case, seed=3)
    for t in (t1, t2):
        t.set_solver(0.9, 1e-4, 0)
    c1 = t1.train_dev(xd, pd, vd, batches, iterations, seed=seed)
    perm = list(range(B * batches))
    rng = _splitmix(seed)
    for it in range(iterations):
        for b in range(batches):
            rows = perm[b * B:(b + 1) * B]
            c2 = t2.batch(xs[rows], ps[rows], vs[rows], lr=0.1)
        for i in range(len(perm)):
            j = next(rng) % (i + 1)
            perm[i], perm[j] = perm[j], perm[i]
    assert perm != list(range(B * batches))
    assert abs(c1 - c2) <= 1e-5 * max(1.0, abs(c2)), (c1, c2)
    for i in range(t1.num_params()):
        name = t1.param_info(i)[0]
        assert rel_diff(t1.get_param(i), t2.get_param(i)) <= 2e-6, name
    assert any(a.any() for a in velocities(t1))
    ex.close()
