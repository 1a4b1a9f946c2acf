"""GPU: the trainer's Adam solver (agz_trainer_set_adam), fused into the BatchNorm backward kernel for the batch-shaped gamma / beta and
swept by k_solver_sweep<SK_ADAM> for everything else.

The contract (include/agz.h, DESIGN §2 `solver-adam`), per learnable element in fp32, t the step counter the host advances:
    g1 = grad_scale * g;  g2 = g1 + l2 * w (l2 != 0);  g3 = clamp(g2, -c, c) (c > 0)
    m = b1 * m + (1 - b1) * g3;  v = b2 * v + (1 - b2) * g3^2;  w += (-lr) * ((m * rc1) / (sqrtf(v * rc2) + eps)),  rc = 1 / (1 - b^t)
restated in float32 numpy by test_adam_cpu.adam_step (checked there against float64).

Bars of the element-wise recurrence, c * 2^-24 * (|result| + |increment|) with c twice the number of chained roundings (each operation
rounds to half an ulp; sqrtf and the division are within one ulp, not half; the device may contract multiply-adds where numpy does not):
    m, v: three operations each (the two products and the sum)                                    -> c = 6
    w:    at most eight (m * rc1, v * rc2, sqrtf, + eps, the division, * (-lr), the sum; one spare for the two one-ulp ones) -> c = 16
What the roundings are counted FROM:
  - w's eight operations start at m' and v'.  The expected w is therefore the restatement's last line evaluated at the DEVICE's m', v'
    (which are themselves held to their own bars against the restatement): where b1 * m and (1 - b1) * g3 cancel, a half-ulp of either
    is many ulps of m', the quotient inherits it, and no count of w's own roundings covers that.
  - with L2 the increment of m is (1 - b1) * a and of v (1 - b2) * a^2, a = min(|g1| + |l2 * w|, c): the magnitude of the terms g3 is
    summed from, not of their sum.  The device contracts g1 + l2 * w into one rounding where numpy rounds the product first: half an ulp
    of l2 * w, which is many ulps of g3 where the two terms cancel.  Without L2 a = |g3|, the plain increment.
Fused against two-pass: 3 * max(e0, 2e-6) with e0 the vanilla pair's own difference in the same run; against the oracle the bars of
test_train_gpu.test_sgd_steps_and_export.

eps*: Adam's map g -> step is not Lipschitz near |g| ~ eps (at eps = 1e-8 an element whose gradient two paths compute as +1e-9 and -1e-9
steps by +lr on one and -lr on the other).  Wherever two computations of the same gradient are compared (fused / two-pass, the oracle,
train_dev) eps is eps* = the median |g| of a first scratch forward_backward, so that |d step| <= lr * |d g| / eps*; and there
lr = 0.1 * eps*, which makes that Lipschitz constant 0.1 — the learn rate of the vanilla pair beside it, whose map has exactly that
constant.  The pairs are then comparable on the same bar."""
import ctypes
import os
import struct

import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi
from test_adam_cpu import adam_consts, adam_step

pytestmark = pytest.mark.gpu

CASES = [
    # K, L, FC, W, H, F, A, B  (the shapes of test_solver_gpu.CASES)
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
FUSED_CASE = (64, 2, 32, 7, 7, 2, 50, 6)
ULP = 2.0 ** -24
B1, B2, EPS8 = 0.9, 0.999, 1e-8


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


def moments(t):
    return [t.get_moments(i) for i in range(t.num_params())]


def grads(t):
    return [t.get_grad(i) for i in range(t.num_params())]


def rel_diff(a, b):
    """max |a - b| relative to the tensor's maximum"""
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-3)


def v1_file_size(t):
    """AGZTRN01: magic, agz_net_conf (10 x 4 bytes), count, then {uint64 n, n floats} per tensor"""
    return 8 + 40 + 8 + sum(8 + 4 * t.param_info(i)[1] for i in range(t.num_params()))


def v4_file_size(t):
    """AGZTRN04: the 01 payload, agz_solver_conf, agz_adam_conf, uint64 t, the tensor block twice (m, then v)"""
    return v1_file_size(t) + 16 + 16 + 8 + 2 * (v1_file_size(t) - 56)


def eps_star(ctx, case, seed, x, pi, v, mode=None, head_scale=1.0):
    """the median |g| of a scratch forward_backward (on a trainer of its own: the ones under test see only the steps they are compared on);
    also max |g|"""
    t = make_dev(ctx, case, seed, mode=mode, head_scale=head_scale)
    t.forward_backward(x, pi, v)
    g = np.concatenate([np.abs(a) for a in grads(t)])
    t.close()
    e = float(np.median(g))
    assert e > 0
    return e, float(g.max())


# ---- 1. off is untouched ------------------------------------------------------------------------------------------------------------------
def test_adam_turned_on_and_off_again_leaves_the_vanilla_trainer(ctx, tmp_path):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    fresh, toggled = make_dev(ctx, case, seed=21), make_dev(ctx, case, seed=21)
    toggled.set_adam()
    assert toggled.get_adam()["on"]
    toggled.set_adam(on=False)
    for step in range(2):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        costs = []
        for t in (fresh, toggled):
            costs.append(t.forward_backward(x, pi, v))
            t.apply(0.1)
        assert costs[0] == costs[1], costs
    for i, (a, b) in enumerate(zip(params(fresh), params(toggled))):
        assert a.tobytes() == b.tobytes(), fresh.param_info(i)[0]
    for t in (fresh, toggled):
        st = t.get_adam()
        assert not st["on"] and st["t"] == 0
        assert (st["beta1"], st["beta2"], st["eps"]) == (np.float32(0.9), np.float32(0.999), np.float32(1e-8))
        for m, v in moments(t):
            assert not m.any() and not v.any()
    fresh.save(tmp_path / "fresh.agz")
    toggled.save(tmp_path / "toggled.agz")
    blob = open(tmp_path / "fresh.agz", "rb").read()
    assert blob[:8] == b"AGZTRN01" and len(blob) == v1_file_size(fresh)
    assert open(tmp_path / "toggled.agz", "rb").read() == blob


# ---- 2. the recurrence, element by element ---------------------------------------------------------------------------------------------
OPTIONS = [(0.0, 0.0), (1e-4, "c*")]


def check_recurrence(ctx, case, l2, clip, gs, mode=None, steps=3, lr=0.01):
    """three steps (t = 1, 2, 3: the bias corrections differ) of forward_backward, every gradient read, apply(lr, gs); w, m, v against the
    numpy restatement started from the device's state before the step and fed the device's own gradients"""
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5, mode=mode)
    dt.set_adam(B1, B2, EPS8)
    n = dt.num_params()
    fractions, worst = [], [0.0, 0.0, 0.0]
    f32 = np.float32
    om1, om2 = f32(1.0 - float(f32(B1))), f32(1.0 - float(f32(B2)))
    for step in range(steps):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B + step)
        dt.forward_backward(x, pi, v)
        g = grads(dt)
        c = clip
        if clip == "c*":                 # the median |g1| of the case: the clamp bites on about half of the elements
            c = float(np.median(np.concatenate([np.abs(np.float32(gs) * a) for a in g])))
            assert c > 0
        dt.set_solver(0, l2, c)
        w0, mv0 = params(dt), moments(dt)
        assert dt.get_adam()["t"] == step
        dt.apply(lr, gs)
        assert dt.get_adam()["t"] == step + 1
        w1, mv1 = params(dt), moments(dt)
        clamped = total = 0
        for i in range(n):
            _, me, ve, g3, _ = adam_step(w0[i], mv0[i][0], mv0[i][1], g[i], lr, gs, l2, c, B1, B2, EPS8, step + 1)
            _, _, _, _, rc1, rc2 = adam_consts(B1, B2, step + 1)
            inc = f32(-lr) * ((mv1[i][0] * rc1) / (np.sqrt(mv1[i][1] * rc2) + f32(EPS8)))      # (the last line, at the device's m', v')
            we = w0[i] + inc
            a = np.abs(g3)
            if l2 != 0:
                a = np.abs(f32(gs) * g[i]) + np.abs(f32(l2) * w0[i])
                if c > 0:
                    a = np.minimum(a, f32(c))
            bars = (16 * ULP * (np.abs(we) + np.abs(inc)), 6 * ULP * (np.abs(me) + om1 * a), 6 * ULP * (np.abs(ve) + om2 * (a * a)))
            name = dt.param_info(i)[0]
            for k, (got, want, bar) in enumerate(((w1[i], we, bars[0]), (mv1[i][0], me, bars[1]), (mv1[i][1], ve, bars[2]))):
                d = np.abs(got - want)
                nz = bar > 0
                if nz.any():
                    worst[k] = max(worst[k], float((d[nz] / bar[nz]).max()))
                j = int(np.argmax(d - bar))
                assert np.all(d <= bar), (name, "wmv"[k], step, int((d > bar).sum()), "worst element %d: got %r want %r bar %r; w0 %r g %r m0 %r v0 %r "
                                          "m1 %r v1 %r" % (j, got[j], want[j], bar[j], w0[i][j], g[i][j], mv0[i][0][j], mv0[i][1][j], mv1[i][0][j],
                                                           mv1[i][1][j]))
            if c > 0:
                clamped += int((np.abs(g3) == np.float32(c)).sum())
                total += g3.size
        if c > 0:
            fractions.append(clamped / total)
            assert 0.2 <= clamped / total <= 0.8, (step, clamped / total)
    print("case %s mode %s (l2 %g, clip %s, grad_scale %g): worst w / m / v %.2f / %.2f / %.2f of the bar; clamped %s" %
          (case, mode, l2, clip, gs, worst[0], worst[1], worst[2], ["%.2f" % f for f in fractions]))
    dt.close()


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("l2,clip", OPTIONS)
@pytest.mark.parametrize("case", CASES)
def test_two_pass_adam_step_is_the_recurrence_element_by_element(ctx, case, l2, clip, gs):
    check_recurrence(ctx, case, l2, clip, gs)


# ---- 3. the fused step equals the two-pass step -----------------------------------------------------------------------------------------------
def check_fused_equals_two_pass(ctx, case, seed, steps, mode=None, l2=1e-4, head_scale=1.0):
    K, L, FC, W, H, F, Aspace, B = case
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=300)
    eps, gmax = eps_star(ctx, case, seed, x, pi, v, mode=mode, head_scale=head_scale)
    lr = 0.1 * eps                       # the Lipschitz constant lr / eps* of Adam's map = the vanilla pair's learn rate
    van_f, van_t, adam_f, adam_t = [make_dev(ctx, case, seed, mode=mode, head_scale=head_scale) for _ in range(4)]
    for t in (adam_f, adam_t):
        t.set_adam(B1, B2, eps)
        t.set_solver(0, l2, 0)
    for step in range(steps):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        van_f.batch(x, pi, v, lr=0.1)
        van_t.forward_backward(x, pi, v)
        van_t.apply(0.1)
        adam_f.batch(x, pi, v, lr=lr)
        adam_t.forward_backward(x, pi, v)
        adam_t.apply(lr)
    assert adam_f.get_adam()["t"] == steps and adam_t.get_adam()["t"] == steps
    worst = (0.0, 0.0, 0.0, 0.0)
    pf, pt, qf, qt = params(van_f), params(van_t), params(adam_f), params(adam_t)
    mf, mt = moments(adam_f), moments(adam_t)
    assert any(a.any() for a, _ in mf) and any(b.any() for _, b in mf)
    print("fused vs two-pass, case %s mode %s: eps* %.3e, lr %.3e, max|g| / eps* %.1f" % (case, mode, eps, lr, gmax / eps))
    fails = []
    for i in range(len(pf)):
        e0 = rel_diff(pf[i], pt[i])            # the vanilla pair: the behaviour without any option, in this very run
        e = rel_diff(qf[i], qt[i])
        worst = max(worst, (e / (3 * max(e0, 2e-6)), e, e0, max(rel_diff(mf[i][0], mt[i][0]), rel_diff(mf[i][1], mt[i][1]))))
        if not e <= 3 * max(e0, 2e-6):
            fails.append((van_f.param_info(i)[0], e, e0))
    print("    worst Adam pair %.2f of the bar (%.2e; vanilla pair of that tensor e0 %.2e; its moments %.2e)" % worst)
    for t in (van_f, van_t, adam_f, adam_t):
        t.close()
    assert not fails, fails


def test_fused_adam_step_equals_the_two_pass_step(ctx):
    check_fused_equals_two_pass(ctx, FUSED_CASE, seed=21, steps=3)


# ---- 4. the headline width in the mode the step is timed in ------------------------------------------------------------------------------
@pytest.mark.parametrize("l2,clip", OPTIONS)
def test_adam_recurrence_at_the_headline_width_wino_h2(ctx, l2, clip):
    check_recurrence(ctx, HEADLINE, l2, clip, 1.0, mode="wino_h2")


def test_fused_adam_step_at_the_headline_width_wino_h2(ctx):
    """Compared after the FIRST step, where the vanilla pair's own spread is still small, and with the heads' BatchNorm gamma / beta drawn
    0.05 times make_pair's (test_solver_gpu.test_fused_momentum_step_at_the_headline_width_wino_h2 says why: with head inputs of order one a
    lr-0.1 vanilla step on a 19x19 board moves a logit by ~70 and the trajectory compares nothing)."""
    check_fused_equals_two_pass(ctx, HEADLINE, seed=21, steps=1, mode="wino_h2", head_scale=0.05)


# ---- 5. against the oracle: numpy carries w, m, v over the oracle's gradients -----------------------------------------------------------------
def test_adam_trajectory_matches_numpy_over_the_oracle(ctx):
    """Three steps of batch(lr) with Adam and L2 1e-4 against a trajectory the code under test has no part in: the oracle supplies the
    gradients (batch with lr = 0), float32 numpy carries w, m, v through the definition and sets the oracle's parameters each step.
    Bars: test_sgd_steps_and_export's (cost 2e-5, parameters 1e-4 * max|o| + 1e-7 per tensor).

    The case — CASES[0], seed 9, wscale 1.0, eps* = the median |g| of the oracle's first gradient (1.04e-2), lr 1e-3 — was fixed on the CPU
    beforehand: the numpy-over-oracle trajectory run twice, the second time with every gradient element perturbed by the project's gradient
    bar (2e-5 * max|g|, random signs), differs by 0.19 of the parameter bar and 0.31 of the cost bar (both <= 1/2: the bar measures the
    kernels, not the case's sensitivity).  At lr 3e-3 the same control gives 0.61 / 0.79 and at lr 1e-2 224 / 1.4, so those were not used."""
    case = CASES[0]
    K, L, FC, W, H, F, Aspace, B = case
    l2, lr = 1e-4, 1e-3
    ot, dt = make_pair(ctx, *case, seed=9, wscale=1.0)
    n = ot.num_params()
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=100)
    ot.batch(x, pi, v, lr=0.0)               # (lr = 0: the oracle's parameters stay; only its gradients are read)
    eps = float(np.median(np.concatenate([np.abs(ot.get_grad(i)) for i in range(n)])))
    assert 0.9e-2 < eps < 1.2e-2, eps        # the value the control above was run at
    dt.set_adam(B1, B2, eps)
    dt.set_solver(0, l2, 0)
    w = [ot.get_param(i) for i in range(n)]
    m = [np.zeros_like(a) for a in w]
    u = [np.zeros_like(a) for a in w]
    for step in range(3):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=100 + step)
        co = ot.batch(x, pi, v, lr=0.0)
        for i in range(n):
            w[i], m[i], u[i], _, _ = adam_step(w[i], m[i], u[i], ot.get_grad(i), lr, 1.0, l2, 0, B1, B2, eps, step + 1)
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
    print("Adam trajectory against numpy over the oracle: worst parameter error %.3f of the bar" % worst)


# ---- 6. checkpoints -------------------------------------------------------------------------------------------------------------------------
def _run_steps(t, case, seeds, fused, lr=0.01):
    K, L, FC, W, H, F, Aspace, B = case
    for s in seeds:
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=s)
        if fused:
            t.batch(x, pi, v, lr=lr)
        else:
            t.forward_backward(x, pi, v)
            t.apply(lr)


def _state(t):
    return (t.get_adam(), t.get_solver(), [a.tobytes() for a in params(t)], [(m.tobytes(), v.tobytes()) for m, v in moments(t)])


@pytest.mark.parametrize("fused", [False, True])
def test_checkpoint_carries_the_moments_and_the_counter(ctx, tmp_path, fused):
    case = DETERMINISTIC
    t1 = make_dev(ctx, case, seed=5)
    t1.set_adam(0.8, 0.99, 1e-6)
    t1.set_solver(0, 1e-4, 0.5)
    _run_steps(t1, case, (1, 2), fused)
    path = tmp_path / "adam.agz"
    t1.save(path)
    blob = open(path, "rb").read()
    v1 = v1_file_size(t1)
    assert blob[:8] == b"AGZTRN04" and len(blob) == v4_file_size(t1)
    assert struct.unpack("<fffi", blob[v1:v1 + 16])[3] == 0 and struct.unpack("<fffiQ", blob[v1 + 16:v1 + 40])[3:] == (1, 2)
    t2 = A.Trainer(ctx, *case)
    t2.load(path)                                                       # a fresh trainer: the file carries options, t and moments
    want = {"beta1": np.float32(0.8), "beta2": np.float32(0.99), "eps": np.float32(1e-6), "on": True, "t": 2}
    assert t2.get_adam() == want and t1.get_adam() == want
    assert t2.get_solver() == {"momentum": 0.0, "l2reg": np.float32(1e-4), "clip": 0.5}
    assert _state(t2) == _state(t1)
    assert any(m.any() for m, _ in moments(t2)) and any(v.any() for _, v in moments(t2))
    _run_steps(t1, case, (3,), fused)
    _run_steps(t2, case, (3,), fused)
    assert _state(t2) == _state(t1) and t2.get_adam()["t"] == 3       # the third step, to the bit
    # every truncation point of the Adam block's structure, one byte more, and inconsistent blocks of the right length: rejected, nothing changed
    before = _state(t2)
    cuts = {v1, v1 + 1, v1 + 15, v1 + 16, v1 + 17, v1 + 31, v1 + 32, v1 + 33, v1 + 39, v1 + 40, len(blob) - 1, len(blob) - 4}
    pos = v1 + 40
    for rep in range(2):
        for i in range(t1.num_params()):
            n = t1.param_info(i)[1]
            cuts.update((pos + 1, pos + 7, pos + 8, pos + 9, pos + 8 + 4 * (n // 2), pos + 8 + 4 * n - 1, pos + 8 + 4 * n))
            pos += 8 + 4 * n
    assert pos == len(blob)
    cuts.discard(len(blob))
    bads = [blob[:c] for c in sorted(cuts)] + [blob + b"\0\0\0\0"]
    for off, val in ((v1, struct.pack("<f", 0.9)),                     # a momentum beside Adam
                     (v1 + 16, struct.pack("<f", 1.5)),                 # beta1 out of range
                     (v1 + 24, struct.pack("<f", 0.0)),                 # eps = 0
                     (v1 + 28, struct.pack("<i", 0)),                   # an Adam block that says Adam is off
                     (v1 + 40, struct.pack("<Q", 3)),                   # the first moment tensor's count word
                     (len(blob) - 4 * t1.param_info(t1.num_params() - 1)[1] - 8, struct.pack("<Q", 1))):   # the last one's
        bads.append(blob[:off] + val + blob[off + len(val):])
    bad = tmp_path / "bad.agz"
    for b in bads:
        open(bad, "wb").write(b)
        with pytest.raises(A.AgzError, match=r"\(-1\)"):
            t2.load(bad)
    assert _state(t2) == before
    # an 01 file loaded into an Adam trainer: the moments and t zeroed, the setting kept
    plain = make_dev(ctx, case, seed=6)
    plain.save(tmp_path / "plain.agz")
    assert open(tmp_path / "plain.agz", "rb").read(8) == b"AGZTRN01"
    t2.load(tmp_path / "plain.agz")
    assert t2.get_adam() == dict(want, t=0)
    assert not any(m.any() or v.any() for m, v in moments(t2))
    assert [a.tobytes() for a in params(t2)] == [a.tobytes() for a in params(plain)]
    # an 02 file: the file's solver, Adam off
    plain.set_solver(0.9, 0, 0)
    _run_steps(plain, case, (7,), fused)
    plain.save(tmp_path / "mom.agz")
    assert open(tmp_path / "mom.agz", "rb").read(8) == b"AGZTRN02"
    t2.load(tmp_path / "mom.agz")
    assert not t2.get_adam()["on"] and t2.get_adam()["t"] == 0 and t2.get_solver()["momentum"] == np.float32(0.9)
    assert [t2.get_velocity(i).tobytes() for i in range(t2.num_params())] == [plain.get_velocity(i).tobytes() for i in range(t2.num_params())]
    # and the Adam file into that momentum trainer: the velocity goes, Adam comes back
    t2.load(path)
    assert t2.get_adam() == want and t2.get_solver()["momentum"] == 0.0
    # with running BatchNorm statistics as well: AGZTRN03 with inner form 3, and the state survives
    t1.set_bn_tracking(True)
    _run_steps(t1, case, (4,), fused)
    t1.save(tmp_path / "adam_bn.agz")
    head = open(tmp_path / "adam_bn.agz", "rb").read(12)
    assert head[:8] == b"AGZTRN03" and struct.unpack("<I", head[8:])[0] == 3
    t3 = A.Trainer(ctx, *case)
    t3.load(tmp_path / "adam_bn.agz")
    assert _state(t3) == _state(t1) and t3.get_adam()["t"] == 4
    assert t3.get_bn_tracking() == t1.get_bn_tracking()
    for t in (t1, t2, t3, plain):
        t.close()


# ---- 7. validation --------------------------------------------------------------------------------------------------------------------------
def test_invalid_adam_settings_are_refused_and_change_nothing(ctx):
    t = make_dev(ctx, CASES[0], seed=5)
    t.set_adam(0.5, 0.9, 1e-3)
    want = t.get_adam()
    nan, inf = float("nan"), float("inf")
    for bad in [(1.0, 0.9, 1e-3, 1), (-0.1, 0.9, 1e-3, 1), (0.5, 1.0, 1e-3, 1), (0.5, -0.1, 1e-3, 1), (0.5, 0.9, 0.0, 1), (0.5, 0.9, -1e-3, 1),
                (nan, 0.9, 1e-3, 1), (0.5, nan, 1e-3, 1), (0.5, 0.9, nan, 1), (inf, 0.9, 1e-3, 1), (0.5, inf, 1e-3, 1), (0.5, 0.9, inf, 1),
                (0.5, 0.9, 1e-3, 2), (0.5, 0.9, 1e-3, -1), (1.5, 0.9, 1e-3, 0), (0.5, 0.9, 0.0, 0)]:
        ac = capi.AdamConf(*bad)
        assert capi.lib().agz_trainer_set_adam(t.h, ctypes.byref(ac)) == -1, bad
        assert t.get_adam() == want, bad
    # Adam and a momentum exclude each other, both ways, and nothing changes
    solver = t.get_solver()
    with pytest.raises(A.AgzError, match=r"\(-4\)"):
        t.set_solver(0.9, 0, 0)
    assert t.get_solver() == solver and t.get_adam() == want
    t.set_solver(0, 1e-3, 2.0)                 # (L2 and clip go with Adam)
    t.set_adam(on=False)
    t.set_solver(0.9, 0, 0)
    off = t.get_adam()
    with pytest.raises(A.AgzError, match=r"\(-4\)"):
        t.set_adam()
    assert t.get_adam() == off and not off["on"] and t.get_solver()["momentum"] == np.float32(0.9)
    # no moments while Adam is off: get returns zeros, set is refused
    n = t.param_info(1)[1]
    vals = np.arange(n, dtype=np.float32)
    m, v = t.get_moments(1)
    assert not m.any() and not v.any()
    with pytest.raises(A.AgzError, match=r"\(-4\)"):
        t.set_moments(1, vals, vals)
    # round trip in the layout of get_param; a wrong length is refused
    t.set_solver(0, 0, 0)
    t.set_adam(0.5, 0.9, 1e-3)
    with pytest.raises(A.AgzError, match=r"\(-1\)"):
        t.set_moments(1, np.zeros(n + 1, np.float32), np.zeros(n + 1, np.float32))
    t.set_moments(1, vals, 2 * vals)
    m, v = t.get_moments(1)
    np.testing.assert_array_equal(m, vals)
    np.testing.assert_array_equal(v, 2 * vals)
    assert not t.get_moments(2)[0].any()
    # reset_solver: moments and t zeroed, the options kept
    K, L, FC, W, H, F, Aspace, B = CASES[0]
    x, pi, vv = batch_data(B, F, H, W, Aspace, seed=1)
    t.set_bn_tracking(True)                    # (agz_trainer_eval needs running statistics)
    t.batch(x, pi, vv, lr=0.001)
    assert t.get_adam()["t"] == 1 and all(a.any() for a in t.get_moments(0))
    held = [(m.tobytes(), v.tobytes()) for m, v in moments(t)]
    t.eval(x, pi, vv)                          # the forward-only pass touches neither t nor the moments
    assert t.get_adam()["t"] == 1 and [(m.tobytes(), v.tobytes()) for m, v in moments(t)] == held
    t.reset_solver()
    assert t.get_adam() == dict(want, t=0)
    assert not any(a.any() or b.any() for a, b in moments(t))
    # lr = 0: the moments move, w does not
    w0 = params(t)
    t.batch(x, pi, vv, lr=0.0)
    assert t.get_adam()["t"] == 1 and all(a.any() for a in t.get_moments(0))
    assert [a.tobytes() for a in params(t)] == [a.tobytes() for a in w0]
    t.close()


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


def test_train_dev_with_adam_is_a_loop_of_batch(ctx):
    """dual.Train over device tensors with Adam on == batch after batch in the same row order (shuffleBatch's Fisher-Yates over the build's
    SplitMix64, meta.go:57-102, restated here).  dual.Train's learn rate is 0.1 whatever the solver; eps = eps*."""
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
    eps, _ = eps_star(ctx, case, 3, xs[:B], ps[:B], vs[:B])
    t1, t2 = make_dev(ctx, case, seed=3), make_dev(ctx, case, seed=3)
    for t in (t1, t2):
        t.set_adam(B1, B2, eps)
        t.set_solver(0, 1e-4, 0)
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
    assert t1.get_adam()["t"] == batches * iterations == t2.get_adam()["t"]
    assert any(m.any() for m, _ in moments(t1))
    ex.close()
