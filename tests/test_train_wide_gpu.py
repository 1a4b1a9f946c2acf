"""GPU: the trainer's wide-board kernels (board width >= 16) at every geometry they dispatch on, against float64 autograd AND the oracle.

agogo_amd/csrc/train.hip picks its kernels by shape; the fastest ones open at W >= 16 and K = 256 / 512 and had only been compared with a
reference at 19x19 (and one 16x17, K = 64 case).  Here: the smallest instance of every geometry those launchers distinguish (CASES), the
A/B forms of the DMA forward convolution on the geometries with board crossings inside a tile, and a fixed-seed family over
W 16..21 x H 3..20 x K 64..512.  Every run first asserts WHICH kernels ran (agz_trainer_last_paths, agz_debug.h) against a restatement
of the launchers' rules in this file (expected_paths: written from the rules, never read back from the library), then holds

    cost      |device - oracle|   <= 1e-4 * max(1, |oracle|)        (the bar of test_forward_backward_headline_width_19x19)
    gradient  |device - float64|  <= 2e-5 * max|float64| + 1e-7     per tensor (the project's bar; tests/f64_train.py is the reference)
    gradient  |device - oracle|   <= 2e-5 * max|oracle|  + 1e-7     per tensor (kept as a second assertion)

on three data draws per case.  The draws were chosen on the CPU with the oracle alone (scripts/debug/wide_seed_scan.py): only seeds where the
fp32 oracle is within HALF the bar of float64 (1e-5 of the tensor maximum) on every tensor are used, and the test re-asserts that, so a
failure can be attributed: the message names the outlier (device or fp32 oracle) and the element.  profiles/train_wide_boards.md holds the
measured ratios."""
import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from conftest import fuzz_seeds
from f64_train import f64_train
from test_train_gpu import batch_data, make_pair

gpu = pytest.mark.gpu

F_PLANES, FC_UNITS = 18, 32
CD3_IMG = 372          # rows of k_conv_h2dma3's x image (conv_maps.hpp)

FWD = {0: "-", capi.PATH_FWD_F32: "f32", capi.PATH_FWD_BF16X3: "bf16x3", capi.PATH_FWD_H2W: "h2w", capi.PATH_FWD_H2DMA: "h2dma", capi.PATH_FWD_H2DMA3: "h2dma3"}
WGRAD = {0: "-", capi.PATH_WGRAD_F32: "wgrad", capi.PATH_WGRAD_X3: "wgrad_x3", capi.PATH_WGRAD_H2: "wgrad_h2", capi.PATH_WGRAD_H2T3: "wgrad_h2t3"}
DGRAD = {0: "-", capi.PATH_DGRAD_RAW: "raw", capi.PATH_DGRAD_X3: "x3", capi.PATH_DGRAD_WINO_H2: "wino_h2"}
BN2 = {0: "-", capi.PATH_BN2_SCALAR: "bn_bwd2", capi.PATH_BN2_V: "bn_bwd2_v"}
MODES = {"f32": capi.COMPUTE_F32_MFMA, "bf16x3": capi.COMPUTE_BF16X3, "wino_h2": capi.COMPUTE_WINO_H2}


def names_of(paths):
    return [(FWD[f], WGRAD[w], DGRAD[d], BN2[b]) for f, w, d, b in paths]


# ---- the launchers' rules, restated (train.hip: dma_layer, conv3_layer, use_h2_fwd, use_x3, use_wino and the branches of forward_backward_dev;
# every "fills the chip" clause is true under COMPUTE_FORCE, which every run here sets)
def conv3_image_rows(W, H, B):
    """rows of the largest x image a 256-row tile of k_conv_h2dma3 needs: padded distance of the tile's last pixel from its first + 2 Wp + 3"""
    HW, Hp, Wp, M = H * W, H + 2, W + 2, B * H * W

    def pix(m):
        return ((m // HW) * Hp + (m % HW) // W + 1) * Wp + (m % HW) % W + 1
    return max(pix(min(m0 + 255, M - 1)) - pix(m0) + 2 * Wp + 3 for m0 in range(0, M, 256))


def expected_paths(W, H, B, K, L, mode, hook=1):
    Kp = (K + 31) // 32 * 32
    wino, x3 = mode == "wino_h2", mode in ("bf16x3", "wino_h2")
    dma_on, nine_taps = bool(hook & 1), not hook & 32
    n_pad = B * (H + 2) * (W + 2)
    out = []
    for l in range(L + 1):
        cin, cout = (32, Kp) if l == 0 else (Kp, 2 * Kp)     # layer 0: padded planes -> K; a dual block: K -> [a | b]
        h2 = wino and cin >= 64 and cin % 32 == 0 and cout % 256 == 0 and n_pad * max(cin, cout) * 4 < 2 ** 32
        dma = dma_on and h2 and W >= 16 and n_pad * cin * 2 < 2 ** 31
        # the DMA convolution reads planes split under the input's range word, which only the vector BatchNorm pass of the layer before writes
        x_range = l > 0 and wino and Kp % 4 == 0 and Kp // 4 <= 256 and 256 % (Kp // 4) == 0
        if dma and x_range:
            fwd = capi.PATH_FWD_H2DMA3 if nine_taps and conv3_image_rows(W, H, B) <= CD3_IMG else capi.PATH_FWD_H2DMA
        elif h2:
            fwd = capi.PATH_FWD_H2W
        elif x3 and cin % 16 == 0 and cin >= 64:
            fwd = capi.PATH_FWD_BF16X3
        else:
            fwd = capi.PATH_FWD_F32
        bn2 = capi.PATH_BN2_V if wino and cout % 4 == 0 and cout // 4 <= 256 and 256 % (cout // 4) == 0 else capi.PATH_BN2_SCALAR
        off31 = n_pad * max(cin, cout) * 4 < 2 ** 31
        if wino and off31 and cout % 4 == 0 and cin % 4 == 0:
            wg = capi.PATH_WGRAD_H2T3 if W >= 16 and cout % 8 == 0 and cin % 8 == 0 else capi.PATH_WGRAD_H2
        elif x3 and off31:
            wg = capi.PATH_WGRAD_X3
        else:
            wg = capi.PATH_WGRAD_F32
        if l == 0:
            dg = 0
        elif wino and cout % 32 == 0 and cout >= 64:
            dg = capi.PATH_DGRAD_WINO_H2
        elif x3 and cout % 16 == 0 and cout >= 64:
            dg = capi.PATH_DGRAD_X3
        else:
            dg = capi.PATH_DGRAD_RAW
        out.append((fwd, wg, dg, bn2))
    return out


# ---- the cases: id -> (W, H, B, K, L), what the issue's table says the dual blocks take in wino_h2 mode, the three data draws.
# SEEDS: chosen by scripts/debug/wide_seed_scan.py — the first three seeds from 100 upwards at which the fp32 oracle is within 1e-5 of the
# tensor maximum of float64 on every gradient tensor.  Skipped there, the ORACLE being the one off (a ReLU unit of its own fp32 forward on the
# other side of zero: 1.2e-2, 2.1e-4 and 1.7e-5 of a tensor's maximum): seed 100 of (c) and of (g), seed 102 of (j, K = 384).
# REPLACED once, by the rule for the function's discontinuity at ReLU zero (a unit whose float64 pre-activation is within fp32 rounding of zero
# and whose sign the device flips; `wide_seed_scan.py --unit` prints the float64 pre-activation): seed 103 of (c) -> 106 (104 and 105: the
# oracle itself is off).  There L1_0, board 0, channel 90, pixel (3, 4) has the float64 pre-activation -3.6e-7 on a layer of rms 1.05 — a plain
# fp32 forward of the same network is 3.2e-7 rms (2e-6 at most) from float64 at that BatchNorm — and bf16x3 and wino_h2 (not fp32-MFMA) both
# turn the unit on: every tensor below it then moves by 1e-3 .. 2.5e-2 of its maximum.
H2T3, WINO, V, SC = capi.PATH_WGRAD_H2T3, capi.PATH_DGRAD_WINO_H2, capi.PATH_BN2_V, capi.PATH_BN2_SCALAR
DMA3, DMA1, H2W = capi.PATH_FWD_H2DMA3, capi.PATH_FWD_H2DMA, capi.PATH_FWD_H2W
CASES = {
    "a_16x16_b1_k256": ((16, 16, 1, 256, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # M = 256: one whole tile = one board; HW % 32 == 0
    "b_16x16_b3_k256": ((16, 16, 3, 256, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # every tile boundary is a board boundary
    "c_16x17_b2_k256_l2": ((16, 17, 2, 256, 2), (DMA3, H2T3, WINO, V), (101, 102, 106)),   # 8.5 wgrad steps per board; partial last tile of 32 rows; planes chain
    "d_17x16_b2_k256": ((17, 16, 2, 256, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # the transpose of (c)
    "e_20x16_b2_k256": ((20, 16, 2, 256, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # the image needs exactly 372 rows
    "f_21x16_b2_k256": ((21, 16, 2, 256, 1), (DMA1, H2T3, WINO, V), (100, 101, 102)),      # 374+ rows: one tap per step ...
    "f_21x16_b1_k256": ((21, 16, 1, 256, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # ... the same board alone fits (328)
    "g_16x9_b3_k256_l2": ((16, 9, 3, 256, 2), (DMA3, H2T3, WINO, V), (101, 102, 103)),     # 360 rows; two board crossings in one tile
    "h_16x3_b6_k256": ((16, 3, 6, 256, 1), (DMA1, H2T3, WINO, V), (100, 101, 102)),        # does not fit; 128-row tiles over three boards; 1.5 wgrad steps; one ragged Winograd tile row
    "i_16x16_b2_k512": ((16, 16, 2, 512, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # first K = 512 trainer: 2 Kp at its limit
    "j_16x16_b2_k384": ((16, 16, 2, 384, 1), (H2W, H2T3, WINO, SC), (100, 101, 103)),      # no DMA forward; c_tiles 3; scalar k_bn_bwd2 + k_absmax
    "j_16x16_b2_k192": ((16, 16, 2, 192, 1), (capi.PATH_FWD_BF16X3, H2T3, WINO, SC), (100, 101, 102)),   # 2 Kp = 384: no fp16x2 forward at all (bf16x3)
    "k_19x19_b2_k128": ((19, 19, 2, 128, 1), (DMA3, H2T3, WINO, V), (100, 101, 102)),      # one 128-channel tile
}
ALL_MODE_CASES = ("a_16x16_b1_k256", "c_16x17_b2_k256_l2", "h_16x3_b6_k256", "i_16x16_b2_k512")
FORM_CASES = ("b_16x16_b3_k256", "c_16x17_b2_k256_l2", "e_20x16_b2_k256", "g_16x9_b3_k256_l2")
COST_LIMIT = 2 * 16 * 16 * 512 ** 2   # B H W K^2 of case (i): the family rejects anything dearer


def conf_of(W, H, B, K, L):
    return dict(K=K, L=L, FC=FC_UNITS, W=W, H=H, F=F_PLANES, A=H * W + 1, B=B)


def test_the_restated_rules_give_what_the_table_says():
    """CPU: expected_paths / conv3_image_rows against the literal entries of the issue's table, so a slip in the restatement is not
    silently 'confirmed' by a library with the same slip."""
    rows = {(20, 16, 2): 372, (21, 16, 1): 328, (16, 9, 3): 360, (16, 9, 5): 396, (16, 3, 5): 450}
    for (W, H, B), want in rows.items():
        assert conv3_image_rows(W, H, B) == want, (W, H, B, conv3_image_rows(W, H, B))
    assert 374 <= conv3_image_rows(21, 16, 2) <= 376
    for B in (2, 3, 5):
        for H in range(16, 21):
            assert conv3_image_rows(20, H, B) <= CD3_IMG < conv3_image_rows(21, H, B), (H, B)
    for name, ((W, H, B, K, L), block, _) in CASES.items():
        paths = expected_paths(W, H, B, K, L, "wino_h2")
        assert paths[0] == (capi.PATH_FWD_F32, H2T3, 0, V if 256 % (K // 4) == 0 else SC), (name, names_of(paths))   # 32 padded planes in: fp32 forward
        assert all(p == block for p in paths[1:]), (name, names_of(paths))
        assert B * H * W * K * K <= COST_LIMIT


# ---- references, computed once per case and shared by the modes and forms
_REF = {}


def reference(name):
    """the oracle trainer with make_pair's parameters and, per draw, (data, oracle cost, oracle gradients, float64 cost, float64 gradients)"""
    if name not in _REF:
        c = conf_of(*CASES[name][0]) if name in CASES else conf_of(*family_draw(int(name[4:]))[:5])
        _REF[name] = dict(conf=c, ot=None, params=None, draws={})
    return _REF[name]


def reference_draw(R, ot, seed):
    if seed not in R["draws"]:
        c = R["conf"]
        x, pi, v = batch_data(c["B"], c["F"], c["H"], c["W"], c["A"], seed=seed)
        co = ot.batch(x, pi, v, lr=0.0)
        go = [ot.get_grad(i).copy() for i in range(ot.num_params())]
        c64, g64 = f64_train(R["params"], x, pi, v, c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"])
        R["draws"][seed] = (x, pi, v, co, go, c64, g64)
    return R["draws"][seed]


def trainer_for(ctx, R):
    """a device trainer holding the case's parameters (the first call builds the oracle half too, through make_pair)"""
    c = R["conf"]
    if R["ot"] is None:
        R["ot"], dt = make_pair(ctx, c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"])
        R["params"] = [R["ot"].get_param(i).copy() for i in range(R["ot"].num_params())]
        R["names"] = [R["ot"].param_name(i) for i in range(R["ot"].num_params())]
        return dt
    dt = A.Trainer(ctx, c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"])
    for i, p in enumerate(R["params"]):
        dt.set_param(i, p)
    return dt


def where(R, i, flat):
    """the element of tensor i in words: out-channel / in-channel / tap of a filter, board / channel / pixel of gamma / beta"""
    c, nm = R["conf"], R["names"][i]
    n = R["params"][i].size
    if nm.startswith("Filter"):
        k = 3 if n % 9 == 0 and not nm.endswith("Head") else 1
        cin = c["F"] if nm == "FilterInit" else c["K"]
        o, ci, t = np.unravel_index(flat, (n // (cin * k * k), cin, k * k))
        return "out-channel %d, in-channel %d, tap (%d,%d)" % (o, ci, t // k, t % k)
    if nm.endswith("_gamma") or nm.endswith("_beta"):
        b, ch, y, x = np.unravel_index(flat, (c["B"], n // (c["B"] * c["H"] * c["W"]), c["H"], c["W"]))
        return "board %d, channel %d, pixel (row %d, column %d)" % (b, ch, y, x)
    return "flat element %d of %d" % (flat, n)


def check_step(R, dt, seed, tag):
    """one forward / backward of `dt` on draw `seed` against both references; returns (worst ratio to float64, to the oracle, oracle's own)"""
    ot = R["ot"]
    x, pi, v, co, go, c64, g64 = reference_draw(R, ot, seed)
    cd = dt.forward_backward(x, pi, v)
    print("%s draw %d: cost device %.7g oracle %.7g float64 %.7g" % (tag, seed, cd, co, c64))
    assert abs(cd - co) <= 1e-4 * max(1.0, abs(co)), (tag, seed, "cost", cd, co, c64)
    w64 = wo = wref = 0.0
    bad = []
    for i in range(len(go)):
        gd = dt.get_grad(i).astype(np.float64)
        s64, so = float(np.abs(g64[i]).max()), float(np.abs(go[i]).max())
        e64, eo, eref = np.abs(gd - g64[i]), np.abs(gd - go[i]), np.abs(go[i] - g64[i])
        w64, wo, wref = max(w64, e64.max() / (s64 + 1e-30)), max(wo, eo.max() / (so + 1e-30)), max(wref, eref.max() / (s64 + 1e-30))
        # the reference must stand on its own: the oracle within half the bar of float64 (how the seeds were chosen)
        assert eref.max() <= 1e-5 * s64 + 5e-8, (tag, seed, R["names"][i], "the fp32 ORACLE is %.2e of the tensor maximum from float64: not a usable draw" % (eref.max() / (s64 + 1e-30)))
        if e64.max() > 2e-5 * s64 + 1e-7 or eo.max() > 2e-5 * so + 1e-7:
            j = int(np.argmax(e64))
            outlier = "the DEVICE is the outlier" if e64[j] > eref[j] else "the fp32 ORACLE is the outlier"
            bad.append("%s: device-float64 %.2e, device-oracle %.2e, oracle-float64 %.2e of the tensor maximum %.3e; worst at %s: device %.8g oracle %.8g float64 %.8g — %s"
                       % (R["names"][i], e64.max() / (s64 + 1e-30), eo.max() / (so + 1e-30), eref.max() / (s64 + 1e-30), s64, where(R, i, j), gd[j], go[i][j], g64[i][j], outlier))
    assert not bad, "%s draw %d:\n  " % (tag, seed) + "\n  ".join(bad)
    assert any(np.abs(g).max() > 1e-6 for g in go)      # the gradient is not trivially zero
    return w64, wo, wref


def run_case(ctx, name, mode, seeds, hook=None, expect=None):
    R = reference(name)
    c = R["conf"]
    dt = trainer_for(ctx, R)
    dt.set_compute_mode(MODES[mode] | capi.COMPUTE_FORCE)
    if hook is not None:
        dt.set_dma_forward(hook)
    want = expected_paths(c["W"], c["H"], c["B"], c["K"], c["L"], mode, 1 if hook is None else int(hook))
    tag = "%s %s%s" % (name, mode, "" if hook is None else " hook %d" % int(hook))
    worst = (0.0, 0.0, 0.0)
    for seed in seeds:
        worst = tuple(max(a, b) for a, b in zip(worst, check_step(R, dt, seed, tag)))
        got = [dt.last_paths(l) for l in range(c["L"] + 1)]
        assert got == want, (tag, "layers 0..L took", names_of(got), "the rules say", names_of(want))
        if expect is not None:
            assert all(g == expect for g in got[1:]), (tag, names_of(got))
    print("WIDE %s | %dx%d B=%d K=%d L=%d | %s | worst/max: float64 %.2e oracle %.2e (oracle's own %.2e)"
          % (tag, c["W"], c["H"], c["B"], c["K"], c["L"], " ; ".join("/".join(p) for p in names_of(got)), *worst))
    dt.close()
    return got


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wide_board_wino_h2(ctx, name):
    _, block, seeds = CASES[name]
    run_case(ctx, name, "wino_h2", seeds, expect=block)


@gpu
def test_k_above_512_is_refused(ctx):
    """the documented limit (2 Kp <= 1024 channels of a dual block): K = 512 — case (i) — is the widest trainer, the next width is refused"""
    with pytest.raises(A.AgzError, match="K > 512"):
        A.Trainer(ctx, 544, 1, FC_UNITS, 16, 16, F_PLANES, 257, 2)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", ALL_MODE_CASES)
def test_wide_board_f32_and_bf16x3(ctx, name, mode):
    """k_wgrad / conv3x3_raw and k_wgrad_x3 / conv3x3_raw_x3 on wide boards at K >= 256"""
    got = run_case(ctx, name, mode, CASES[name][2])
    if mode == "f32":
        assert all(p == (capi.PATH_FWD_F32, capi.PATH_WGRAD_F32, capi.PATH_DGRAD_RAW, SC) for p in got[1:])
    else:
        assert all(p == (capi.PATH_FWD_BF16X3, capi.PATH_WGRAD_X3, capi.PATH_DGRAD_X3, SC) for p in got[1:])


@gpu
@pytest.mark.parametrize("name", FORM_CASES)
def test_wide_board_forward_forms_agree(ctx, name):
    """default (k_conv_h2dma3) against one tap per step (k_conv_h2dma, hook 1 | 32): the same products in the same order per accumulator —
    the cost bit-equal, the gradients within the weight gradient's atomics (2e-6 of the maximum + 1e-9, as in
    test_forward_dma_convolution_forms_agree); and the staged split (conv3x3_h2w, hook 0) under the float64 bar.  The hook's report must
    show that each form really ran another kernel."""
    R = reference(name)
    c = R["conf"]
    d3, d1 = trainer_for(ctx, R), trainer_for(ctx, R)
    for dt in (d3, d1):
        dt.set_compute_mode(capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE)
    d1.set_dma_forward(1 | 32)
    for seed in CASES[name][2][:2]:
        x, pi, v = batch_data(c["B"], c["F"], c["H"], c["W"], c["A"], seed=seed)
        c3, c1 = d3.forward_backward(x, pi, v), d1.forward_backward(x, pi, v)
        assert c3 == c1, (name, seed, c3, c1)
        for i in range(d3.num_params()):
            g3, g1 = d3.get_grad(i), d1.get_grad(i)
            assert float(np.abs(g3 - g1).max()) <= 2e-6 * float(np.abs(g1).max()) + 1e-9, (name, seed, R["names"][i])
        for l in range(1, c["L"] + 1):
            assert d3.last_paths(l)[0] == DMA3 and d1.last_paths(l)[0] == DMA1, (name, l, d3.last_paths(l), d1.last_paths(l))
    d3.close()
    d1.close()
    run_case(ctx, name, "wino_h2", CASES[name][2], hook=1 | 32, expect=(DMA1, H2T3, WINO, V))
    run_case(ctx, name, "wino_h2", CASES[name][2], hook=0, expect=(H2W, H2T3, WINO, V))


# ---- a small fixed-seed family
def family_draw(seed):
    """(W, H, B, K, L, mode) of a family seed: drawn until B H W K^2 — per dual block: times L — is within case (i)'s"""
    rng = np.random.default_rng(7100 + seed)
    while True:
        W, H = int(rng.integers(16, 22)), int(rng.integers(3, 21))
        K = int(rng.choice([64, 128, 192, 256, 384, 512]))
        B, L = int(rng.integers(1, 7)), int(rng.integers(1, 3))
        mode = ["f32", "bf16x3", "wino_h2"][int(rng.integers(0, 3))]
        if B * H * W * K * K * L <= COST_LIMIT:
            return W, H, B, K, L, mode


# the data draw of each family seed: 200 + seed unless the oracle alone misses half the bar there (scripts/debug/wide_seed_scan.py)
# (206..208 of seed 6 and 208 of seed 8: the oracle itself 4e-4 .. 5e-2 of a beta tensor's maximum from float64.)  REPLACED once each, same rule as
# in CASES: seed 4's draw 204 -> 216 (L1_1, board 0, channel 100, pixel (7, 4): float64 pre-activation -1.06e-6, the device turns it on) and seed
# 6's draw 209 -> 218 (L1_1, board 0, channel 29, pixel (1, 11): +1.05e-6, the device turns it off); a plain fp32 forward is 4.6e-7 rms, 3.4e-6 at
# most, from float64 at that second-block BatchNorm.
FAMILY_DATA_SEED = {4: 216, 6: 218, 8: 209}


def test_the_family_reaches_every_path():
    """CPU: over the 12 graded seeds every value of the path report occurs, apart from k_wgrad_h2 (boards narrower than 16: the narrow
    cases of test_train_gpu.py run it; no A/B bit reaches it at W >= 16).  Restated dispatch, so the seeds were chosen without a GPU."""
    seen = [set(), set(), set(), set()]
    for seed in range(12):
        W, H, B, K, L, mode = family_draw(seed)
        for p in expected_paths(W, H, B, K, L, mode):
            for s, val in zip(seen, p):
                s.add(val)
    assert seen[0] == {1, 2, 3, 4, 5}, sorted(FWD[x] for x in seen[0])
    assert seen[1] == {capi.PATH_WGRAD_F32, capi.PATH_WGRAD_X3, capi.PATH_WGRAD_H2T3}, sorted(WGRAD[x] for x in seen[1])
    assert seen[2] == {0, 1, 2, 3}, sorted(DGRAD[x] for x in seen[2])
    assert seen[3] == {1, 2}, sorted(BN2[x] for x in seen[3])


@gpu
@pytest.mark.parametrize("seed", fuzz_seeds(12))
def test_wide_board_family(ctx, seed):
    """one data draw per family seed, the same assertions as the cases; prints the paths the seed took.  (A soak run on fresh seeds —
    AGZ_FUZZ_BASE / AGZ_FUZZ_N — can meet a draw the fp32 oracle itself flips a ReLU unit on: check_step then says 'not a usable draw'.)"""
    W, H, B, K, L, mode = family_draw(seed)
    name = "fam_%d" % seed
    got = run_case(ctx, name, mode, (FAMILY_DATA_SEED.get(seed, 200 + seed),))
    print("family seed %d: %dx%d B=%d K=%d L=%d %s -> %s" % (seed, W, H, B, K, L, mode, names_of(got)))
    _REF.pop(name, None)
