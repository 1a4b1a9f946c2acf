"""GPU: a step of the trainer does not depend on the steps before it.

In AGZ_COMPUTE_WINO_H2 mode the vector BatchNorm pass of layer l (k_bn_apply_v, agogo_amd/csrc/train.hip) also writes the fp16 hi / lo planes
layer l + 1's DMA convolution and weight gradient read, scaled by the power of two of LAST step's range word (amax_prev); k_split_h2p_cond
keeps them when that word and this step's exact one prescribe the same power of two and splits the tensor again otherwise; the host's
planes_fused / x_amax_ready / TLayer::x_planes decide which applies.  The kernel's comment promises "the results do not depend on the
history".  Here every compared step runs on a trainer WITH history (Th) and on a FRESH one (Tf: the same parameters, its first step — the
estimate word is 0, it always splits), in COMPUTE_WINO_H2 | COMPUTE_FORCE, and holds

    paths      agz_trainer_last_paths: the expected DMA forward on every block, on both trainers (test_train_wide_gpu.expected_paths)
    cost       equal in bytes
    gradient   |Th - Tf| <= 2e-6 * max|Tf| + 1e-9 per tensor   (the project's bar for identical products under another atomic order:
                                                               test_forward_dma_convolution_forms_agree)
    finite     everything

after a CONTROL — a second fresh trainer against the first — has met the same two bars on that very step.  What a layer did with its planes
is read from agz_trainer_last_planes (agz_debug.h) and judged by a restatement of the keep rule in this file (scale_exp / kept: written
from the rule, pinned on literals by a CPU test, never read back from the library).

Shapes (W, H, B, K, L), the smallest at which the path is live and boards cross inside a tile: P = (16, 17, 2, 256, 2) and
Q = (16, 9, 3, 256, 2) — cases c and g of test_train_wide_gpu.CASES with their graded draws — and R = (16, 16, 2, 128, 1).
Sequences: kept (the same draw twice: every block layer must report kept; on P and Q also test_train_wide_gpu's float64 bar), other draw,
range jump (gamma and beta of a BatchNorm stage times 2^k between two steps on one draw: the reading layer's range word is last step's times
2^k bit for bit, it must report not kept; k = +3 leaves Inf in the stale hi plane, so one surviving element shows), dead layer (range word
0), an eval between two steps, mode and A/B hook switches, checkpoint resume across a range-exponent change (learn rates chosen in float64
by scripts/debug/history_lr_scan.py), and the tied trainer.  profiles/train_history.md holds the measured figures and the three mutations
of train.hip these tests catch."""
import struct

import numpy as np
import pytest

import agogo_amd as A
import test_train_wide_gpu as WB
from agogo_amd import capi
from f64_train import f64_train
from test_tied_cpu import is_batch_shaped
from test_train_gpu import batch_data, make_pair

gpu = pytest.mark.gpu

WINO = capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE
F32 = capi.COMPUTE_F32_MFMA | capi.COMPUTE_FORCE
DMA_FWD = (capi.PATH_FWD_H2DMA3, capi.PATH_FWD_H2DMA)
WIDE = {"P": "c_16x17_b2_k256_l2", "Q": "g_16x9_b3_k256_l2"}
SHAPE = {"P": WB.CASES[WIDE["P"]][0], "Q": WB.CASES[WIDE["Q"]][0], "R": (16, 16, 2, 128, 1)}
SEEDS = {"P": WB.CASES[WIDE["P"]][2], "Q": WB.CASES[WIDE["Q"]][2], "R": (101, 102, 103)}
GRAD_REL, GRAD_ABS = 2e-6, 1e-9
TIED_SEED = 101    # graded for the tied trainer as the plain draws were (scripts/debug/history_lr_scan.py draws): the fp32 oracle 2.5e-6 of a tensor's maximum from float64


# ---- the keep rule, restated (train.hip: wg_h2_scale, k_split_h2p_cond)
ONE = 127      # the biased exponent of the scale 1.0
def scale_exp(bits):
    """the biased exponent of the power of two a range word prescribes: 2^(13 - E), and 1.0 — exponent 127 — for an all-zero (or subnormal)
    or non-finite range"""
    e = (bits >> 23) & 255
    if e == 0 or e == 255:
        return ONE
    return min(max(127 + 13 - (e - 127), 1), 254)


def kept(fused, est, rng):
    return bool(fused) and est != 0 and scale_exp(est) == scale_exp(rng)


def bits_of(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_the_restated_keep_rule_on_literals():
    """CPU: scale_exp / kept on literal range words, so that a slip in the restatement is not 'confirmed' by a library with the same slip"""
    assert ONE == 127 == (bits_of(1.0) >> 23)
    assert scale_exp(0) == ONE
    assert scale_exp(0x00000001) == ONE and scale_exp(0x007fffff) == ONE            # subnormals
    assert scale_exp(0x7f800000) == ONE and scale_exp(0x7fc00000) == ONE            # +Inf, NaN
    assert scale_exp(bits_of(1.0)) == 140                                           # 2^13
    assert scale_exp(bits_of(1.9999999)) == 140 and scale_exp(bits_of(2.0)) == 139 and scale_exp(bits_of(0.5)) == 141
    assert scale_exp(bits_of(8192.0)) == 127 and scale_exp(bits_of(16383.0)) == 127 and scale_exp(bits_of(16384.0)) == 126   # [2^13, 2^14): scale 1
    assert scale_exp(bits_of(2.0 ** -120)) == 254 and scale_exp(bits_of(2.0 ** -114)) == 254 and scale_exp(bits_of(2.0 ** -113)) == 253   # clamped above
    assert scale_exp(bits_of(2.0 ** 120)) == 20 and scale_exp(bits_of(2.0 ** 127)) == 13
    assert kept(True, bits_of(5.0), bits_of(7.9)) and kept(1, bits_of(4.0), bits_of(4.0))
    assert not kept(True, bits_of(5.0), bits_of(8.0)) and not kept(True, bits_of(5.0), bits_of(5.0 / 2048))
    assert not kept(False, bits_of(5.0), bits_of(5.0)) and not kept(True, 0, bits_of(5.0)) and not kept(True, 0, 0)
    assert kept(True, bits_of(9000.0), 0) and not kept(True, bits_of(5.0), 0)       # an all-zero tensor under scale 1: only an estimate in [2^13, 2^14) matches
    assert kept(True, bits_of(2.0 ** -120), bits_of(2.0 ** -118))                   # both clamped to the same scale


# ---- trainers
_BASE = {}
STATS = {}        # sequence -> worst |Th - Tf| / max and worst control, printed per test (profiles/train_history.md)


def base(ctx, shape):
    """conf, names and make_pair's parameters of a shape (P and Q: the record test_train_wide_gpu keeps, with its references)"""
    if shape not in _BASE:
        if shape in WIDE:
            S = WB.reference(WIDE[shape])
            if S["ot"] is None:
                WB.trainer_for(ctx, S).close()
        else:
            c = WB.conf_of(*SHAPE[shape])
            ot, dt = make_pair(ctx, c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"])
            dt.close()
            S = dict(conf=c, ot=ot, params=[ot.get_param(i).copy() for i in range(ot.num_params())], names=[ot.param_name(i) for i in range(ot.num_params())])
        _BASE[shape] = S
    return _BASE[shape]


def tied_params(S):
    return [p.reshape(S["conf"]["B"], -1)[0].copy() if is_batch_shaped(nm) else p for nm, p in zip(S["names"], S["params"])]


def new_trainer(ctx, S, params=None, tied=False, mode=WINO, hook=None, track=False):
    c = S["conf"]
    t = A.Trainer(ctx, c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"], tied=tied)
    for i, p in enumerate((tied_params(S) if tied else S["params"]) if params is None else params):
        t.set_param(i, p)
    t.set_compute_mode(mode)
    if hook is not None:
        t.set_dma_forward(hook)
    if track:
        t.set_bn_tracking(True)
    return t


def data_of(S, seed):
    c = S["conf"]
    return batch_data(c["B"], c["F"], c["H"], c["W"], c["A"], seed=seed)


def report(S, t):
    """[(fused, est_bits, range_bits)] of layers 0 .. L after the last step"""
    return [t.last_planes(l) for l in range(S["conf"]["L"] + 1)]


def show(rep):
    return " ".join("L%d:%s(est %08x range %08x)" % (l, "kept" if kept(*r) else ("resplit" if r[0] else "unfused"), r[1], r[2]) for l, r in enumerate(rep) if l)


def same_bytes(a, b):
    return struct.pack("<f", a) == struct.pack("<f", b)


def assert_same_step(S, ta, ca, tb, cb, want, tag):
    """the bars of the module docstring between two trainers that just took the same step; returns the worst |a - b| / max|b| over the tensors"""
    for t in (ta, tb):
        got = [t.last_paths(l) for l in range(S["conf"]["L"] + 1)]
        assert got == want, (tag, "layers 0..L took", WB.names_of(got), "the rules say", WB.names_of(want))
        assert all(p[0] in DMA_FWD for p in got[1:]), (tag, WB.names_of(got))
    worst, bad = 0.0, []
    for i, nm in enumerate(S["names"]):
        ga, gb = ta.get_grad(i), tb.get_grad(i)
        assert np.all(np.isfinite(ga)) and np.all(np.isfinite(gb)), (tag, nm, "not finite", int((~np.isfinite(ga)).sum()), int((~np.isfinite(gb)).sum()))
        err, scale = float(np.abs(ga.astype(np.float64) - gb).max()), float(np.abs(gb).max())
        worst = max(worst, err / (scale + 1e-30))
        if err > GRAD_REL * scale + GRAD_ABS:
            bad.append("%s: %.3e of the maximum %.3e" % (nm, err / (scale + 1e-30), scale))
    print("    %s: cost %.9g / %.9g, worst gradient tensor %.2e of its maximum" % (tag, ca, cb, worst))
    assert np.isfinite(ca) and np.isfinite(cb), (tag, ca, cb)
    assert same_bytes(ca, cb), (tag, "cost", ca, cb)
    assert not bad, "%s:\n  " % tag + "\n  ".join(bad)
    return worst


def step_against_fresh(ctx, S, th, seed, seq, tag, mode=WINO, hook=None, track=False):
    """Th takes a forward / backward on draw `seed`; two fresh trainers with Th's parameters take it as their first step: the control (fresh
    against fresh), then Th against fresh.  Returns (Th's cost, Th's plane report)."""
    c = S["conf"]
    data = data_of(S, seed)
    params = [th.get_param(i) for i in range(th.num_params())]
    want = WB.expected_paths(c["W"], c["H"], c["B"], c["K"], c["L"], "wino_h2", 1 if hook is None else int(hook))
    tf = new_trainer(ctx, S, params, th.is_tied(), mode, hook, track)
    tc = new_trainer(ctx, S, params, th.is_tied(), mode, hook, track)
    cf, cc = tf.forward_backward(*data), tc.forward_backward(*data)
    for t in (tf, tc):
        assert all(r[1] == 0 for r in report(S, t)), (tag, "a fresh trainer with an estimate", show(report(S, t)))
    wc = assert_same_step(S, tc, cc, tf, cf, want, "%s draw %d control" % (tag, seed))
    ch = th.forward_backward(*data)
    rep = report(S, th)
    print("    %s draw %d history: %s" % (tag, seed, show(rep)))
    wh = assert_same_step(S, th, ch, tf, cf, want, "%s draw %d history against fresh" % (tag, seed))
    st = STATS.setdefault(seq, [0.0, 0.0])
    st[0], st[1] = max(st[0], wh), max(st[1], wc)
    print("HISTORY %s | %s draw %d | history/fresh %.2e control %.2e (worst so far %.2e / %.2e) | %s" % (seq, tag, seed, wh, wc, st[0], st[1], show(rep)))
    tf.close()
    tc.close()
    return ch, rep


def f64_of(S, shape, seed, tied):
    """(cost, gradients) of the float64 reference on a draw: test_train_wide_gpu's record for the plain trainer; for the tied one the same
    model with the tied tensor in every row, the row gradients summed (the declared definition, test_tied_cpu)"""
    if not tied:
        return WB.reference_draw(S, S["ot"], seed)[5:7]
    key = ("tied64", seed)
    if key not in S:
        c = S["conf"]
        full = [np.tile(p, c["B"]) if is_batch_shaped(nm) else p for nm, p in zip(S["names"], tied_params(S))]
        c64, g64 = f64_train(full, *data_of(S, seed), c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"])
        S[key] = (c64, [g.reshape(c["B"], -1).sum(axis=0) if is_batch_shaped(nm) else g for nm, g in zip(S["names"], g64)])
    return S[key]


# ---- the sequences
def run_kept(ctx, shape, seed, tied=False):
    S = base(ctx, shape)
    L = S["conf"]["L"]
    tag = "kept %s%s" % (shape, " tied" if tied else "")
    th = new_trainer(ctx, S, tied=tied)
    c1, _ = step_against_fresh(ctx, S, th, seed, "kept", tag + " step 1")
    c2, rep = step_against_fresh(ctx, S, th, seed, "kept", tag + " step 2")
    assert same_bytes(c1, c2), (tag, c1, c2)
    for l in range(1, L + 1):
        assert rep[l][0] and rep[l][1] == rep[l][2] != 0, (tag, "layer %d: the same draw, but the estimate is not the range" % l, show(rep))
        assert kept(*rep[l]), (tag, "layer %d did not keep its planes" % l, show(rep))
    if shape in WIDE:
        c64, g64 = f64_of(S, shape, seed, tied)
        worst = 0.0
        for i, nm in enumerate(S["names"]):
            gd, s64 = th.get_grad(i).astype(np.float64), float(np.abs(g64[i]).max())
            e64 = float(np.abs(gd - g64[i]).max())
            worst = max(worst, e64 / (s64 + 1e-30))
            print("    %s draw %d %s: kept step against float64 %.2e of the maximum %.3e" % (tag, seed, nm, e64 / (s64 + 1e-30), s64))
        for i, nm in enumerate(S["names"]):
            gd, s64 = th.get_grad(i).astype(np.float64), float(np.abs(g64[i]).max())
            assert float(np.abs(gd - g64[i]).max()) <= 2e-5 * s64 + 1e-7, (tag, seed, nm, float(np.abs(gd - g64[i]).max()) / (s64 + 1e-30))
        print("HISTORY kept | %s draw %d | worst against float64 %.2e of a tensor's maximum (cost %.7g, float64 %.7g)" % (tag, seed, worst, c2, c64))
    th.close()


STAGES = {"Init": (("Init",), 1), "block0": (("L1_0", "L2_0"), 2)}     # stage -> the BatchNorm ops scaled, the layer that reads their output


def run_jump(ctx, shape, seed, stage, k, tied=False):
    S = base(ctx, shape)
    L = S["conf"]["L"]
    ops, reader = STAGES[stage]
    assert reader <= L
    tag = "jump %s%s %s 2^%+d" % (shape, " tied" if tied else "", stage, k)
    th = new_trainer(ctx, S, tied=tied)
    th.forward_backward(*data_of(S, seed))
    rep1 = report(S, th)
    for i, nm in enumerate(S["names"]):
        if nm in [op + sfx for op in ops for sfx in ("_gamma", "_beta")]:
            p = th.get_param(i)
            q = np.ldexp(p, k).astype(np.float32)
            assert np.array_equal(np.ldexp(q.astype(np.float64), -k), p.astype(np.float64)), (tag, nm, "the scaling is not exact")
            th.set_param(i, q)
    _, rep2 = step_against_fresh(ctx, S, th, seed, "jump", tag)
    r1, (fused, est, rng) = rep1[reader][2], rep2[reader]
    assert 0 < ((r1 >> 23) & 255) + k < 255 and r1 != 0
    assert est == r1, (tag, "layer %d's estimate is not last step's range word" % reader, "%08x" % est, "%08x" % r1)
    assert rng == r1 + (k << 23), (tag, "layer %d's range word is not last step's times 2^%d" % (reader, k), "%08x" % rng, "%08x" % r1)
    assert fused, (tag, "layer %d read no fused planes" % reader, show(rep2))
    assert not kept(fused, est, rng), (tag, show(rep2))
    th.close()


def run_other_draw(ctx, shape, tied=False):
    S = base(ctx, shape)
    s1, s2, _ = SEEDS[shape]
    th = new_trainer(ctx, S, tied=tied)
    th.forward_backward(*data_of(S, s1))
    step_against_fresh(ctx, S, th, s2, "other draw", "other draw %s" % shape)
    th.close()


def run_resume(ctx, tmp_path, lr, adam, tied):
    S = base(ctx, "P")
    L = S["conf"]["L"]
    tag = "resume P%s %s lr %g" % (" tied" if tied else "", "adam" if adam else "sgd", lr)
    s1, s2, s3 = SEEDS["P"]
    th = new_trainer(ctx, S, tied=tied)
    if adam:
        th.set_adam()
    th.batch(*data_of(S, s1), lr)
    c2 = th.batch(*data_of(S, s2), lr)
    path = tmp_path / "history.agz"
    th.save(path)
    c3 = th.batch(*data_of(S, s3), lr)
    rep = report(S, th)
    tr = A.Trainer(ctx, *[S["conf"][k] for k in ("K", "L", "FC", "W", "H", "F", "A", "B")], tied=tied)
    tr.set_compute_mode(WINO)
    tr.load(path)
    c3r = tr.batch(*data_of(S, s3), lr)
    repr_ = report(S, tr)
    print("HISTORY resume | %s | costs %.7g %.7g | step 3 %.9g resumed %.9g | uninterrupted %s | resumed %s" % (tag, c2, c3, c3, c3r, show(rep), show(repr_)))
    assert np.isfinite(c3) and np.isfinite(c3r)
    assert any(r[0] and r[1] != 0 and r[2] != 0 and (r[1] >> 23) != (r[2] >> 23) for r in rep[1:]), (tag, "no block layer's range exponent moved between steps 2 and 3", show(rep))
    assert all(r[1] == 0 for r in repr_), (tag, "the resumed trainer has an estimate", show(repr_))
    for t in (th, tr):
        assert all(t.last_paths(l)[0] in DMA_FWD for l in range(1, L + 1)), (tag, [t.last_paths(l) for l in range(L + 1)])
    assert same_bytes(c3, c3r), (tag, c3, c3r)
    worst = 0.0
    for i, nm in enumerate(S["names"]):
        a, b = th.get_param(i), tr.get_param(i)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (tag, nm)
        d, bar = float(np.abs(a - b).max()), 1e-6 * max(float(np.abs(a).max()), 1e-3)
        worst = max(worst, d / bar)
        assert d <= bar, (tag, nm, d, bar)
    print("HISTORY resume | %s | parameters after step 3: worst %.3f of the bar" % (tag, worst))
    th.close()
    tr.close()


# learn rates: scripts/debug/history_lr_scan.py (float64).  The ranges of layers 1 / 2 at the parameters of steps 2 -> 3:
#   plain SGD 0.05: 5.94 -> 154, 8.52 -> 880 (3x-Glorot filters: the steps overshoot, which is what moves the ranges by octaves; 0.02 moves none)
#   tied SGD 0.03: 7.64 -> 85.7, 10.8 -> 439;  plain Adam 1.5: 14.3 -> 18.1, 24.2 -> 34.8;  tied Adam 1.5: 13.1 -> 17.4, 21.2 -> 39.3
# (both layers cross a power of two, each range 8 % or more away from it; the test needs one)
RESUME_LR = {(False, False): 0.05, (False, True): 0.03, (True, False): 1.5, (True, True): 1.5}      # (adam, tied) -> lr


@gpu
@pytest.mark.parametrize("seed_i", [0, 1, 2])
@pytest.mark.parametrize("shape", ["P", "Q", "R"])
def test_same_draw_twice_keeps_the_planes(ctx, shape, seed_i):
    run_kept(ctx, shape, SEEDS[shape][seed_i])


@gpu
@pytest.mark.parametrize("shape", ["P", "Q", "R"])
def test_another_draw_after_a_step(ctx, shape):
    run_other_draw(ctx, shape)


@gpu
@pytest.mark.parametrize("k", [-11, -1, 1, 3])
def test_range_jump_r(ctx, k):
    run_jump(ctx, "R", SEEDS["R"][0], "Init", k)


@gpu
@pytest.mark.parametrize("k", [-1, 3])
@pytest.mark.parametrize("stage", ["Init", "block0"])
@pytest.mark.parametrize("shape", ["P", "Q"])
def test_range_jump_two_blocks(ctx, shape, stage, k):
    run_jump(ctx, shape, SEEDS[shape][0], stage, k)


@gpu
@pytest.mark.parametrize("shape", ["P", "R"])
def test_dead_layer_and_back(ctx, shape):
    """Init_gamma = 0, Init_beta = -1: layer 1's input is all zero, its range word 0 (wg_h2_scale: scale 1); then the parameters come back"""
    S = base(ctx, shape)
    s1, s2, _ = SEEDS[shape]
    th = new_trainer(ctx, S)
    th.forward_backward(*data_of(S, s1))
    saved = {}
    for i, nm in enumerate(S["names"]):
        if nm in ("Init_gamma", "Init_beta"):
            saved[i] = th.get_param(i)
            th.set_param(i, np.full_like(saved[i], 0.0 if nm == "Init_gamma" else -1.0))
    _, rep = step_against_fresh(ctx, S, th, s1, "dead layer", "dead %s" % shape)
    assert rep[1][2] == 0 and rep[1][1] != 0, show(rep)
    for i, p in saved.items():
        th.set_param(i, p)
    _, rep = step_against_fresh(ctx, S, th, s2, "dead layer", "dead %s restored" % shape)
    assert rep[1][1] == 0 and rep[1][2] != 0 and not kept(*rep[1]), show(rep)
    th.close()


@gpu
@pytest.mark.parametrize("shape", ["P", "R"])
def test_eval_between_two_steps(ctx, shape):
    S = base(ctx, shape)
    L = S["conf"]["L"]
    s1, s2, s3 = SEEDS[shape]
    th = new_trainer(ctx, S, track=True)
    th.forward_backward(*data_of(S, s1))
    ce = th.eval(*data_of(S, s3))
    rep = report(S, th)
    te = new_trainer(ctx, S, track=True)
    for bi in range(th.num_bn()):
        te.set_bn_stats(bi, *th.get_bn_stats(bi))
    cf = te.eval(*data_of(S, s3))
    print("HISTORY eval | %s | eval cost after a step %.9g, fresh %.9g | %s | fresh %s" % (shape, ce, cf, show(rep), show(report(S, te))))
    for t in (th, te):
        assert all(t.last_paths(l)[0] in DMA_FWD for l in range(1, L + 1)), [t.last_paths(l) for l in range(L + 1)]
    assert np.isfinite(ce) and same_bytes(ce, cf), (ce, cf)
    te.close()
    step_against_fresh(ctx, S, th, s2, "eval between", "eval between %s" % shape, track=True)
    th.close()


@gpu
@pytest.mark.parametrize("shape", ["P", "R"])
def test_mode_and_hook_switches(ctx, shape):
    S = base(ctx, shape)
    s1, s2, s3 = SEEDS[shape]
    # a WINO_H2 step, a step in f32 mode, WINO_H2 again
    th = new_trainer(ctx, S)
    th.forward_backward(*data_of(S, s1))
    th.set_compute_mode(F32)
    th.forward_backward(*data_of(S, s2))
    assert all(th.last_paths(l)[0] == capi.PATH_FWD_F32 for l in range(S["conf"]["L"] + 1))
    th.set_compute_mode(WINO)
    step_against_fresh(ctx, S, th, s3, "switches", "f32 then wino_h2 %s" % shape)
    th.close()
    # the DMA forward off, then on
    th = new_trainer(ctx, S)
    th.forward_backward(*data_of(S, s1))
    th.set_dma_forward(0)
    th.forward_backward(*data_of(S, s2))
    assert all(th.last_paths(l)[0] == capi.PATH_FWD_H2W for l in range(1, S["conf"]["L"] + 1))
    th.set_dma_forward(1)
    step_against_fresh(ctx, S, th, s3, "switches", "hook 0 then 1 %s" % shape, hook=1)
    th.close()
    # one tap per step, nine taps, and back
    th = new_trainer(ctx, S, hook=1 | 32)
    th.forward_backward(*data_of(S, s1))
    th.set_dma_forward(1)
    step_against_fresh(ctx, S, th, s2, "switches", "hook 33 then 1 %s" % shape, hook=1)
    th.set_dma_forward(1 | 32)
    step_against_fresh(ctx, S, th, s3, "switches", "hook 33, 1, then 33 %s" % shape, hook=1 | 32)
    th.close()


@gpu
@pytest.mark.parametrize("adam", [False, True])
def test_resume_across_a_range_exponent_change(ctx, tmp_path, adam):
    run_resume(ctx, tmp_path, RESUME_LR[(adam, False)], adam, False)


@gpu
def test_tied_same_draw_twice_keeps_the_planes(ctx):
    run_kept(ctx, "P", TIED_SEED, tied=True)


@gpu
def test_tied_range_jump(ctx):
    run_jump(ctx, "P", TIED_SEED, "Init", 3, tied=True)


@gpu
@pytest.mark.parametrize("adam", [False, True])
def test_tied_resume_across_a_range_exponent_change(ctx, tmp_path, adam):
    run_resume(ctx, tmp_path, RESUME_LR[(adam, True)], adam, True)

