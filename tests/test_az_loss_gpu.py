"""GPU: the AlphaZero loss of the trainer (agz_trainer_set_loss(AGZ_LOSS_ALPHAZERO), agz_trainer_get_costs; include/agz.h, DESIGN §2
`az-loss`): softmax cross-entropy of the logits against Pi, a mean over the rows, and an MSE of tanh(o) against V.

Reference: tests/f64_train_az.py, float64 autograd (the oracle keeps the reference loss and is no yardstick here).  Bars, the project's
standing ones: cost, and each of its two terms, 1e-4 * max(1, |float64|); every gradient tensor 2e-5 * max|float64| + 1e-7.

Draws.  Parameters and batches come from f64_train_az.draw_params / draw_batch; the seeds below were chosen on the CPU with the float64
module alone so that every ReLU argument (each BatchNorm's pre-activation, the value head's hidden layer) is at least 1e-5 of its layer's
rms away from zero — an fp32 forward is 2e-6 off at most, so a ReLU that flips cannot be what a failure shows.  Each reference
re-asserts the margin.  Measured margins: TWO_PASS 2.1e-4, ODD_C 6.0e-4, DETERMINISTIC 3.2e-4 (tied 5.4e-4), SINGLE_PASS 2.0e-5 (tied
1.7e-5), A65 3.7e-4, A512 1.5e-3."""
import functools

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from f64_train_az import draw_batch, draw_params, f64_train_az, param_shapes, relu_margin

pytestmark = pytest.mark.gpu

# K, L, FC, W, H, F, A, B
SHAPES = {
    "TWO_PASS": (32, 1, 16, 3, 3, 2, 10, 4),
    "ODD_C": (3, 3, 8, 3, 3, 2, 10, 5),
    "DETERMINISTIC": (32, 2, 24, 3, 3, 2, 10, 6),          # every reduction of a step runs in one workgroup
    "SINGLE_PASS": (32, 1, 16, 19, 19, 2, 362, 12),        # A = 362: more than one 256-column tile, six logits per lane
    "A65": (3, 1, 8, 3, 3, 2, 65, 2),                      # one column past a wave
    "A512": (32, 1, 16, 3, 3, 2, 512, 3),                  # the lane loop's bound: eight logits per lane
}
SEEDS = {("TWO_PASS", False): 1, ("ODD_C", False): 1, ("DETERMINISTIC", False): 1, ("SINGLE_PASS", False): 496, ("A65", False): 1,
         ("A512", False): 1, ("DETERMINISTIC", True): 2, ("SINGLE_PASS", True): 37}
MARGIN = 1e-5
FIRST_FORM = 1 | 4            # agz_trainer_set_dma_forward: bit 0 as it is by default, bit 2 = the first form of the head kernels
E_INVALID, E_STATE = r"\(-1\)", r"\(-4\)"


def names_of(case, tied=False):
    return [nm for nm, _ in param_shapes(case, tied)]


@functools.lru_cache(maxsize=None)
def reference(name, tied=False, pi_kind="softmax", variant=None):
    """the draw and its float64 cost / gradients, computed once per configuration and shared"""
    case = SHAPES[name]
    seed = SEEDS[(name, tied)]
    P = draw_params(case, seed, tied)
    x, pi, v = draw_batch(case, seed + 1000, pi_kind)
    if variant == "stability":      # logits of +-100, value outputs of +-20
        nms = names_of(case, tied)
        for nm, amp in (("Policy_b", 100.0), ("ValueOutput_b", 20.0)):
            p = P[nms.index(nm)]
            p[:] = np.where(np.arange(p.size) % 2 == 0, amp, -amp).astype(np.float32)
    out = {}
    cost, grads, pre = f64_train_az(P, x, pi, v, *case, want_pre=True, tied=tied, out=out)
    m = relu_margin(pre)
    assert m >= MARGIN, "%s: a ReLU argument lies %.3g of its layer's rms from zero" % (name, m)
    return {"case": case, "P": P, "x": x, "pi": pi, "v": v, "cost": cost, "pcost": out["pcost"], "vcost": out["vcost"], "grads": grads,
            "logits": out["logits"], "o": out["o"]}


def make(ctx, ref, tied=False, az=True):
    dt = A.Trainer(ctx, *ref["case"], tied=tied)
    want = param_shapes(ref["case"], tied)
    assert dt.num_params() == len(want)
    for i, ((nm, shp), p) in enumerate(zip(want, ref["P"])):
        assert dt.param_info(i) == (nm, int(np.prod(shp))), (i, dt.param_info(i), nm, shp)
        dt.set_param(i, p)
    if az:
        dt.set_loss(capi.LOSS_ALPHAZERO)
    return dt


def grads(t):
    return [t.get_grad(i) for i in range(t.num_params())]


def check_costs(tag, got, ref):
    """got = (cost, policy term, value term); prints every figure before it asserts"""
    want = (ref["cost"], ref["pcost"], ref["vcost"])
    print("%s: cost %.9g (float64 %.9g)  policy %.9g (%.9g)  value %.9g (%.9g)" % (tag, got[0], want[0], got[1], want[1], got[2], want[2]))
    assert all(np.isfinite(got)), got
    for what, g, w in zip(("cost", "policy", "value"), got, want):
        assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (tag, what, g, w)


def check_grads(tag, names, GD, G64):
    worst, missed = 0.0, []
    for nm, gd, g64 in zip(names, GD, G64):
        assert gd.shape == g64.shape, (nm, gd.shape, g64.shape)
        assert np.isfinite(gd).all(), (tag, nm)
        bar = 2e-5 * float(np.abs(g64).max()) + 1e-7
        err = float(np.abs(gd - g64).max())
        worst = max(worst, err / bar)
        if err > bar:
            missed.append((nm, err, bar))
    print("%s: worst gradient tensor at %.3f of its bar" % (tag, worst))
    assert not missed, (tag, missed)


def check_against_float64(tag, dt, ref, tied=False):
    cost = dt.forward_backward(ref["x"], ref["pi"], ref["v"])
    p, v = dt.costs()
    check_costs(tag, (cost, p, v), ref)
    assert abs(np.float32(p) + np.float32(v) - np.float32(cost)) <= 2.0 ** -23 * abs(cost), (p, v, cost)
    check_grads(tag, names_of(ref["case"], tied), grads(dt), ref["grads"])


# ---- 1. off is untouched --------------------------------------------------------------------------------------------------------------------
def test_the_reference_loss_is_untouched_by_the_option(ctx):
    ref = reference("DETERMINISTIC")
    dt = make(ctx, ref, az=False)
    assert dt.get_loss() == capi.LOSS_REFERENCE
    runs = []
    for prepare in (lambda: None, lambda: dt.set_loss(capi.LOSS_REFERENCE),
                    lambda: (dt.set_loss(capi.LOSS_ALPHAZERO), dt.set_loss(capi.LOSS_REFERENCE))):
        prepare()
        assert dt.get_loss() == capi.LOSS_REFERENCE
        cost = dt.forward_backward(ref["x"], ref["pi"], ref["v"])
        p, v = dt.costs()
        assert abs(np.float32(p) + np.float32(v) - np.float32(cost)) <= 2.0 ** -23 * abs(cost), (p, v, cost)
        runs.append((np.float32(cost).tobytes(), np.float32(p).tobytes(), np.float32(v).tobytes(), [g.tobytes() for g in grads(dt)]))
    assert runs[0] == runs[1] == runs[2]
    # and it IS the reference loss: -mean(Pi z + (1 - Pi)(1 - z)) + mean((o - V)^2) on the float64 logits / value outputs of the same draw
    z, o, Pi, V = ref["logits"], ref["o"], ref["pi"].astype(np.float64), ref["v"].astype(np.float64)
    want_p, want_v = float(-(Pi * z + (1 - Pi) * (1 - z)).mean()), float(((o - V) ** 2).mean())
    print("reference loss: policy %.9g (float64 %.9g) value %.9g (%.9g)" % (p, want_p, v, want_v))
    assert abs(p - want_p) <= 1e-4 * max(1.0, abs(want_p)) and abs(v - want_v) <= 1e-4 * max(1.0, abs(want_v))
    dt.close()


# ---- 2. against float64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_cost_and_gradients_against_float64(ctx, name):
    ref = reference(name)
    dt = make(ctx, ref)
    assert dt.get_loss() == capi.LOSS_ALPHAZERO
    check_against_float64(name, dt, ref)
    dt.close()


@pytest.mark.parametrize("pi_kind", ["onehot", "half_row"])
def test_one_hot_rows_and_a_row_that_sums_to_a_half(ctx, pi_kind):
    """(half_row pins the factor S_b of dz = (S_b p - Pi) / Bn: with S_b taken as 1 that row's gradient is off by p / (2 Bn))"""
    ref = reference("TWO_PASS", pi_kind=pi_kind)
    dt = make(ctx, ref)
    check_against_float64("TWO_PASS " + pi_kind, dt, ref)
    dt.close()


# ---- 3. both forms of the head kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TWO_PASS", "SINGLE_PASS"])
def test_first_form_of_the_head_kernels(ctx, name):
    ref = reference(name)
    dt = make(ctx, ref)
    dt.set_dma_forward(FIRST_FORM)
    check_against_float64(name + " first form", dt, ref)
    dt.close()


# ---- 4. stability ------------------------------------------------------------------------------------------------------------------------------
def test_logits_of_100_and_value_outputs_of_20_stay_finite(ctx):
    """Policy_b = +100 / -100 alternating, ValueOutput_b = +20 / -20: exp(100) is not an fp32 number, so a softmax that does not take the
    row maximum off first gives inf / nan here"""
    ref = reference("TWO_PASS", variant="stability")
    assert np.abs(ref["logits"]).min() > 50 and np.abs(ref["o"]).min() > 10
    dt = make(ctx, ref)
    check_against_float64("TWO_PASS stability", dt, ref)
    dt.close()


# ---- 5. tied -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["DETERMINISTIC", "SINGLE_PASS"])
def test_tied_trainer_against_the_tied_float64_module(ctx, name):
    ref = reference(name, tied=True)
    dt = make(ctx, ref, tied=True)
    check_against_float64(name + " tied", dt, ref, tied=True)
    dt.close()


# ---- 6. reproducible ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(ctx):
    ref = reference("DETERMINISTIC")
    runs = []
    for _ in range(2):
        dt = make(ctx, ref)
        cost = dt.forward_backward(ref["x"], ref["pi"], ref["v"])
        runs.append((np.float32(cost).tobytes(), [np.float32(c).tobytes() for c in dt.costs()], [g.tobytes() for g in grads(dt)]))
        cost2 = dt.forward_backward(ref["x"], ref["pi"], ref["v"])          # and again on the same trainer
        assert (np.float32(cost2).tobytes(), [g.tobytes() for g in grads(dt)]) == (runs[-1][0], runs[-1][2])
        dt.close()
    assert runs[0] == runs[1]


# ---- 7. the gradient belongs to the reported cost ----------------------------------------------------------------------------------------
def test_a_small_step_lowers_the_cost_by_lr_times_the_squared_gradient(ctx):
    """To first order cost(w - lr g) = cost(w) - lr |g|^2.  lr = 2e-4 on the TWO_PASS draw: the float64 module alone gives
    (cost_before - cost_after) / (lr |g|^2) = 0.9990 (|g|^2 = 53.11, a drop of 0.0106 — 4e4 fp32 roundings of the cost), well inside the
    10 % band; at lr = 1e-3 it gives 0.931, at 1e-4 0.9995."""
    lr = 2e-4
    ref = reference("TWO_PASS")
    dt = make(ctx, ref)
    before = dt.forward_backward(ref["x"], ref["pi"], ref["v"])
    gg = sum(float((g.astype(np.float64) ** 2).sum()) for g in grads(dt))
    dt.batch(ref["x"], ref["pi"], ref["v"], lr=lr)
    after = dt.forward_backward(ref["x"], ref["pi"], ref["v"])
    ratio = (before - after) / (lr * gg)
    print("cost %.9g -> %.9g, lr |g|^2 = %.9g, ratio %.4f" % (before, after, lr * gg, ratio))
    assert abs(ratio - 1.0) <= 0.10, (before, after, lr * gg, ratio)
    dt.close()


# ---- 8. eval -----------------------------------------------------------------------------------------------------------------------------------
def test_eval_is_a_held_out_cross_entropy(ctx):
    name = "TWO_PASS"
    ref = reference(name)
    case = ref["case"]
    dt = make(ctx, ref)
    dt.set_bn_tracking(True, 0.9)
    for k in range(3):
        x, pi, v = draw_batch(case, 2000 + k)
        dt.batch(x, pi, v, lr=0.05)
    x, pi, v = draw_batch(case, 2003)
    ev = dt.eval(x, pi, v)
    p, vc = dt.costs()
    stats = [dt.get_bn_stats(i) for i in range(dt.num_bn())]
    out = {}
    want, _ = f64_train_az([dt.get_param(i) for i in range(dt.num_params())], x, pi, v, *case, stats=stats, out=out)
    check_costs(name + " eval", (ev, p, vc), {"cost": want, "pcost": out["pcost"], "vcost": out["vcost"]})
    assert abs(np.float32(p) + np.float32(vc) - np.float32(ev)) <= 2.0 ** -23 * abs(ev), (p, vc, ev)
    dt.close()


# ---- 9. validation ---------------------------------------------------------------------------------------------------------------------------
def test_bad_kinds_are_rejected_and_costs_need_a_forward(ctx):
    ref = reference("TWO_PASS")
    dt = make(ctx, ref, az=False)
    with pytest.raises(capi.AgzError, match=E_STATE):
        dt.costs()
    for start in (capi.LOSS_REFERENCE, capi.LOSS_ALPHAZERO):
        dt.set_loss(start)
        for kind in (-1, 2):
            with pytest.raises(capi.AgzError, match=E_INVALID):
                dt.set_loss(kind)
            assert dt.get_loss() == start
    with pytest.raises(capi.AgzError, match=E_STATE):
        dt.costs()
    dt.forward_backward(ref["x"], ref["pi"], ref["v"])
    assert all(np.isfinite(dt.costs()))
    dt.close()
