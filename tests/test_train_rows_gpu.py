"""GPU: the batch-sized loops of dual.Train's step — every branch of agogo_amd/csrc/train.hip that opens on M = B H W rows or on B boards —
against float64 autograd, at the smallest shapes that take them.

The other trainer tests stop at 2 520 rows per checked step; the measured step is 92 416.  Between the two lies a layer of code whose loops run
once, or not at all, on every shape those tests use: the 2048-row chunks of k_wgrad / k_wgrad_x3 / k_wgrad_h2 (a second chunk, a partial
last one, an edge inside a board row, a second round over the eight XCDs), the board chunks of k_wgrad_h2t3, the single-pass BatchNorm
statistics (M >= 4096), the row groups of k_bn_apply_v / k_bn_bwd2_v, the capped grids of the range / split passes and of the second-form
head kernels.  CASES lists one shape per edge.  Every run first asserts WHICH kernels ran (agz_trainer_last_paths against
test_train_wide_gpu.expected_paths) and HOW their rows were dealt (agz_trainer_last_rows against row_plan below: written from the
launchers' rules, never read back from the library, and pinned on literal numbers by a CPU test — so a changed rows_per_block fails here
instead of silently going back to one chunk), then compares one forward / backward on two draws per case.

The judge is float64 alone, on draws made well-posed.  At these row counts an fp32 reference fails before any device is involved.  Measured on
the CPU with the oracle and float64 torch only — oracle against float64, worst tensor as a fraction of its maximum, draws 100 / 101:

    K, L, WxH, B           rows     fp32 oracle, plain draw                      fp32 oracle, conditioned draw
    128, 1, 9x9, 26        2 106    2.0e-6 / 1.9e-6                              2.4e-6 / 2.3e-6
    256, 1, 16x3, 50       2 400    2.8e-6 / 3.3e-6                              3.3e-6 / 3.6e-6
    256, 2, 19x19, 23      8 303    3.3e-2 / 7.5e-2 (L1_1_beta, L2_0_beta: flipped units; 55 s per draw)   8.2e-6 / 1.5e-5
    64, 1, 13x13, 98      16 562    2.1e-5 / 2.7e-5 (FilterInit)                 2.1e-5 / 2.7e-5
    32, 1, 13x13, 390     65 910    9.0e-3 / 1.5e-1 (L2_0_beta, L1_0_beta: flipped units)   5.0e-5 / 4.8e-5

(1) With millions of ReLU units some float64 pre-activation lies within fp32 rounding of zero on EVERY draw (the smallest seen: 6e-8 to 5e-7);
picking seeds until none flips, as test_train_wide_gpu.py does, cannot work.  (2) The oracle's sequential fp32 sums lose half the bar (1e-5)
from about 8 000 rows even without a flip, and it takes a minute per draw at 8 303 rows, K = 256, L = 2.  So: f64_train.condition moves the beta (the
bias b1) of every unit within tau of zero out to +-2 tau — the untied trainer has one per unit — with tau measured per draw
(f64_train.measured_tau: 16 times the float32 torch model's largest pre-activation error, rounded up to a power of two), under the condition
that fewer than 1e-3 of the units move.  The loss is then smooth on a ball that holds every fp32 evaluation of it, and one CPU test shows on
the 65 910-row shape that the oracle's 9e-3 falls below 1e-4 once the draw is conditioned: the flip was the reference's own.

Per draw:
    cost      |device - float64| <= 1e-4 * max(1, |float64|)                              (the project's bar)
    gradient  max|device - float64| <= max(2e-5, c * m32) * max|float64| + 1e-7  per tensor,  m32 the float32 torch model's own error on that
              tensor and draw, c = 4 in f32 mode and 8 in the split-product modes (the factors of test_tower_f64_gpu.py)
    model     m32 <= 1e-5 on every tensor: the ruler itself is usable.  (Its convolutions run over chunks of boards of at most 2048 rows, so
              that the filter gradients are summed per chunk and then over chunks, whatever torch's thread count: f64_train, chunk_rows.
              Unchunked, FilterInit alone is 6e-6 .. 1.4e-5 at eight threads and 2e-5 .. 6e-5 at one; chunked, 1.5e-6 .. 4.2e-6 at any.)
    oracle    cases a to d only (there it is within half the bar of float64 and takes about a second): the bars of test_train_wide_gpu.py as
              a second assertion.  NOT on e to i: the table above — the oracle is 2e-5 to 5e-5 from float64 there on its own, conditioned or not,
              and a minute per draw at K = 256.
profiles/train_rows.md holds the measured table and the mutations that these tests, and no earlier one, turn red."""
import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi
from f64_train import condition, f64_train, measured_tau, relu_margin
from test_train_gpu import batch_data, make_pair
from test_train_wide_gpu import MODES, expected_paths, names_of, where

gpu = pytest.mark.gpu

NUM_CUS = 256
H2, H2T3 = capi.PATH_WGRAD_H2, capi.PATH_WGRAD_H2T3
SEEDS = (100, 101)        # the data draws of every case (batch_data); each is conditioned before use
MOVED_CAP = 1e-3          # conditioning may move fewer than this fraction of the ReLU units
MODEL_BAR = 1e-5          # the float32 torch model's own error, per tensor, of the tensor's maximum
FACTOR = {"f32": 4.0, "bf16x3": 8.0, "wino_h2": 8.0}

# id -> (K, L, FC, W, H, F, A, B)
CASES = {
    "a_8x8_b32_k64": (64, 1, 32, 8, 8, 2, 65, 32),            # 2 048 rows: exactly one whole chunk, r_end == M with no masked row
    "b_12x9_b19_k64": (64, 1, 32, 12, 9, 2, 109, 19),         # 2 052: a second chunk of four rows, less than a wave's eight-row group
    "c_9x9_b26_k128": (128, 1, 32, 9, 9, 18, 82, 26),         # 2 106: the chunk edge at board 25, row 2, column 5; k_wgrad_h2 with two N tiles
    "d_15x13_b21_k64": (64, 1, 32, 15, 13, 3, 196, 21),       # 4 095: the last shape of the two-pass statistics
    "d_16x16_b16_k64": (64, 1, 32, 16, 16, 3, 257, 16),       # 4 096: the first of k_bn_stats + k_bn_fin2
    "e_13x13_b98_k64": (64, 1, 32, 13, 13, 3, 170, 98),       # 16 562: nine chunks = a second XCD round + seven empty ids; k_bn_bwd2_v rpb = 2 tpr; head grids capped
    "f_13x13_b390_k32": (32, 1, 16, 13, 13, 2, 170, 390),     # 65 910: 33 chunks, the last of 374 rows; k_head_stats_part strided; 49 FC row blocks; rpb 64 / 48
    "g_16x3_b50_k256": (256, 1, 32, 16, 3, 18, 49, 50),       # 2 400: k_wgrad_h2t3 deals 50 boards into 40 chunks
    "h_19x19_b46_k256": (256, 1, 32, 19, 19, 18, 362, 46),    # 16 606: the measured step's kernels at its board; 65 M tiles; rpb 12 / 10; split passes strided
    "i_19x19_b23_k256_l2": (256, 2, 32, 19, 19, 18, 362, 23),  # 8 303: the planes chain across two blocks under single-pass statistics, rpb > tpr
}
ALL_MODE_CASES = ("a_8x8_b32_k64", "b_12x9_b19_k64", "c_9x9_b26_k128", "e_13x13_b98_k64", "f_13x13_b390_k32")
WINO_ONLY_CASES = ("d_15x13_b21_k64", "d_16x16_b16_k64", "g_16x3_b50_k256", "h_19x19_b46_k256", "i_19x19_b23_k256_l2")
ORACLE_CASES = ("a_8x8_b32_k64", "b_12x9_b19_k64", "c_9x9_b26_k128", "d_15x13_b21_k64", "d_16x16_b16_k64")
H_CASE, F_CASE = "h_19x19_b46_k256", "f_13x13_b390_k32"


def conf_of(name):
    return dict(zip(("K", "L", "FC", "W", "H", "F", "A", "B"), CASES[name]))


# ---- the launchers' row rules, restated (train.hip: forward_backward_dev; NUM_CUS compute units)
def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


def board_chunks(B, n):
    """boards per chunk as k_wgrad_h2t3 deals them: chunk c takes boards [c B / n, (c + 1) B / n)"""
    return [(c + 1) * B // n - c * B // n for c in range(n)]


def row_plan(W, H, B, K, L, mode):
    """what agz_trainer_last_rows reports for tower layers 0 .. L: tuples of eight words (capi.ROWS_*); head_plan: layer L + 1"""
    Kp, M, HW, n_pad = round_up(K, 32), B * H * W, H * W, B * (H + 2) * (W + 2)
    wino = mode == "wino_h2"
    paths = expected_paths(W, H, B, K, L, mode)
    out = []
    for l in range(L + 1):
        cin, cout = (32, Kp) if l == 0 else (Kp, 2 * Kp)
        wg = paths[l][1]
        if wg == H2T3:     # chunks of whole boards: about two rounds of an XCD's workgroup slots, never more chunks than boards
            per_chunk = ceil_div(cout, 128) * ceil_div(cin, 128) * 3
            chunks = min(B, 8 * max(1, 2 * (NUM_CUS // 8 * 2) // per_chunk))
        else:              # row chunks of rows_per_block = 2048
            chunks = ceil_div(M, 2048)
        single = int(cout % 4 == 0 and cout <= 1024 and M >= 4096)

        def rpb(c):        # the vector BatchNorm passes: tpr rows in flight per workgroup, at most 2048 workgroups; 0 = the scalar kernel
            if not (wino and c % 4 == 0 and c // 4 <= 256 and 256 % (c // 4) == 0):
                return 0
            tpr = 256 // (c // 4)
            return round_up(max(tpr, ceil_div(M, 2048)), tpr)
        ra, rb = rpb(Kp), rpb(cout)     # apply: over the layer's Kp output channels; backward 2: over dz's [a | b] channels
        need = ceil_div(n_pad * cout // 4, 256) if wg in (H2, H2T3) else 0
        out.append((chunks, single, ra, rb, int(0 < ra <= HW), int(0 < rb <= HW), min(need, 8 * NUM_CUS), need))
    return out


def head_plan(W, H, B, A, FC):
    """the heads' words: second form (the FC kernels' LDS tiles fit: eight rows of 2 HW, of B, of max(A, FC) floats), grid of k_head_conv2 (four rows per workgroup, <= 16 per CU), of k_head_stats_part / k_head_bn_bwd_a
    (256 rows, <= one per CU), of k_cost_part (256 elements of [B][A], <= 64)"""
    M = B * H * W
    assert max(8 * 2 * H * W, 8 * B, 8 * max(A, FC)) * 4 <= 60000, "first-form heads: not a shape of this file"
    return (1, min(ceil_div(M, 4), 16 * NUM_CUS), min(ceil_div(M, 256), NUM_CUS), min(ceil_div(B * A, 256), 64), 0, 0, 0, 0)


def test_row_plan_gives_the_literal_numbers():
    """CPU: row_plan / head_plan / expected_paths against literal numbers worked out by hand from the rules, so that a slip in the
    restatement is not silently 'confirmed' by a library with the same slip."""
    R = capi
    CH, SP, RA, RB, WA, WB, SB, SN = (R.ROWS_WGRAD_CHUNKS, R.ROWS_SINGLE_PASS, R.ROWS_APPLY_RPB, R.ROWS_BWD2_RPB, R.ROWS_APPLY_BOARD_WORDS,
                                      R.ROWS_BWD2_BOARD_WORDS, R.ROWS_SPLIT_BLOCKS, R.ROWS_SPLIT_NEED)

    def plan(name, mode="wino_h2"):
        c = conf_of(name)
        return row_plan(c["W"], c["H"], c["B"], c["K"], c["L"], mode), head_plan(c["W"], c["H"], c["B"], c["A"], c["FC"]), \
            expected_paths(c["W"], c["H"], c["B"], c["K"], c["L"], mode), c["B"] * c["H"] * c["W"]
    for mode in MODES:
        p, _, _, M = plan("a_8x8_b32_k64", mode)        # one whole chunk
        assert M == 2048 and [x[CH] for x in p] == [1, 1]
        p, _, _, M = plan("b_12x9_b19_k64", mode)       # ... and four rows
        assert M == 2052 and [x[CH] for x in p] == [2, 2] and M - 2048 == 4
        p, _, _, M = plan("c_9x9_b26_k128", mode)
        assert M == 2106 and [x[CH] for x in p] == [2, 2]
        assert (2048 // 81, 2048 % 81 // 9, 2048 % 9) == (25, 2, 5)          # the chunk edge: board 25, row 2, column 5
        p, h, _, M = plan("e_13x13_b98_k64", mode)
        assert M == 16562 and [x[CH] for x in p] == [9, 9] and round_up(9, 8) - 9 == 7 and all(x[SP] == 1 for x in p)
        assert h == (1, 4096, 65, 64, 0, 0, 0, 0) and ceil_div(M, 4) == 4141 and ceil_div(98 * 170, 256) == 66     # conv2 and cost capped
        p, h, _, M = plan("f_13x13_b390_k32", mode)
        assert M == 65910 and [x[CH] for x in p] == [33, 33] and M - 32 * 2048 == 374
        assert h == (1, 4096, 256, 64, 0, 0, 0, 0) and ceil_div(M, 256) == 258 and ceil_div(390, 8) == 49
        if mode != "wino_h2":
            assert all(x[RA:] == (0, 0, 0, 0, 0, 0) for x in p)               # scalar BatchNorm kernels, no split pass
    p, _, paths, _ = plan("c_9x9_b26_k128")
    assert [q[1] for q in paths] == [H2, H2] and ceil_div(256, 128) == 2      # k_wgrad_h2, two N tiles on the block
    assert paths[1][0] == capi.PATH_FWD_H2W and paths[1][2] == capi.PATH_DGRAD_WINO_H2
    assert plan("d_15x13_b21_k64")[3] == 4095 and [x[SP] for x in plan("d_15x13_b21_k64")[0]] == [0, 0]
    assert plan("d_16x16_b16_k64")[3] == 4096 and [x[SP] for x in plan("d_16x16_b16_k64")[0]] == [1, 1]
    p, _, paths, _ = plan("e_13x13_b98_k64")
    assert [q[1] for q in paths] == [H2, H2] and p[1][RB] == 16 and p[1][RB] == 2 * (256 // (128 // 4)) and p[0][RA] == 16
    p, _, paths, _ = plan("f_13x13_b390_k32")
    assert (p[0][RA], p[1][RA], p[1][RB]) == (64, 64, 48) and (p[1][WA], p[1][WB]) == (1, 1)
    assert p[1][SB] == 2048 < p[1][SN] == ceil_div(390 * 15 * 15 * 64 // 4, 256) == 5485
    p, _, paths, _ = plan("g_16x3_b50_k256")
    assert [q[1] for q in paths] == [H2T3, H2T3] and [x[CH] for x in p] == [50, 40]
    deal = board_chunks(50, 40)
    assert sorted(deal) == [1] * 30 + [2] * 10 and sum(deal) == 50
    p, h, paths, M = plan(H_CASE)
    assert M == 16606 and paths[1] == (capi.PATH_FWD_H2DMA3, H2T3, capi.PATH_DGRAD_WINO_H2, capi.PATH_BN2_V) and ceil_div(M, 256) == 65
    assert [x[CH] for x in p] == [46, 40] and sorted(board_chunks(46, 40)) == [1] * 34 + [2] * 6
    assert (p[1][RA], p[1][RB], p[1][WA], p[1][WB], p[1][SP]) == (12, 10, 1, 1, 1)
    assert p[1][SB] == 2048 < p[1][SN] and p[0][SB] == 2048 < p[0][SN] and h[3] == 64 < ceil_div(46 * 362, 256)
    p, _, paths, M = plan("i_19x19_b23_k256_l2")
    assert M == 8303 and len(p) == 3 and all(x[SP] == 1 for x in p) and (p[1][RA], p[2][RA], p[2][RB]) == (8, 8, 6) and 8 > 256 // 64
    assert paths[1] == paths[2] == (capi.PATH_FWD_H2DMA3, H2T3, capi.PATH_DGRAD_WINO_H2, capi.PATH_BN2_V)
    # the case lists are the issue's: five cases in every mode, five in wino_h2 alone
    assert sorted(ALL_MODE_CASES + WINO_ONLY_CASES) == sorted(CASES)


# ---- references, computed once per case on the CPU and shared by the modes
_REF = {}


def reference(name):
    """the case's oracle trainer with make_pair's parameters (the same recipe: test_train_gpu.make_pair builds the device half of it)"""
    if name not in _REF:
        c = conf_of(name)
        ot = O.TrainNet(c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"])
        ot.init_random(5)
        rng = np.random.default_rng(5)
        for i in range(ot.num_params()):
            nm, p = ot.param_name(i), ot.get_param(i)
            if nm.endswith("_gamma"):
                p = rng.uniform(0.5, 1.5, p.size).astype(np.float32)
            elif nm.endswith("_beta") or nm.endswith("_b"):
                p = rng.normal(0, 0.1, p.size).astype(np.float32)
            else:
                p = (p * 3.0).astype(np.float32)
            ot.set_param(i, p)
        _REF[name] = dict(conf=c, ot=ot, params=[ot.get_param(i).copy() for i in range(ot.num_params())],
                          names=[ot.param_name(i) for i in range(ot.num_params())], draws={}, checked_pair=False)
    return _REF[name]


def shape_args(c):
    return c["K"], c["L"], c["FC"], c["W"], c["H"], c["F"], c["A"], c["B"]


def reference_draw(name, seed):
    """a conditioned draw and its references: the data, tau and what conditioning did, the parameters to run (float32), the float64 cost
    and gradients, m32 per tensor — and asserts on the spot that the draw is well-posed and the fp32 model a usable ruler"""
    R = reference(name)
    if seed not in R["draws"]:
        c = R["conf"]
        s = shape_args(c)
        x, pi, v = batch_data(c["B"], c["F"], c["H"], c["W"], c["A"], seed=seed)
        tau, d32 = measured_tau(R["params"], x, pi, v, *s)
        params, moved, units, _ = condition(R["params"], x, pi, v, *s, tau)
        c64, g64, pre = f64_train(params, x, pi, v, *s, want_pre="all")
        lo, near, units2 = relu_margin(pre, tau)
        del pre
        print("%s draw %d: tau %.3g (fp32 model's largest pre-activation error %.2e), moved %d of %d units, min |pre64| %.3g"
              % (name, seed, tau, d32, moved, units, lo))
        assert lo >= tau and near == 0 and units2 == units, (name, seed, "conditioning left a unit within tau", lo, tau, near)
        assert moved < MOVED_CAP * units, (name, seed, "conditioning moved %d of %d units" % (moved, units))
        _, g32 = f64_train(params, x, pi, v, *s, dtype=np.float32, chunk_rows=2048)
        m32 = [float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)) for a, b in zip(g32, g64)]
        j = int(np.argmax(m32))
        assert m32[j] <= MODEL_BAR, (name, seed, "the float32 torch model is %.2e of the maximum from float64 on %s" % (m32[j], R["names"][j]))
        assert any(np.abs(g).max() > 1e-6 for g in g64)      # the gradient is not trivially zero
        R["draws"][seed] = dict(x=x, pi=pi, v=v, tau=tau, d32=d32, moved=moved, units=units, lo=lo, params=params, c64=c64, g64=g64,
                                m32=m32, oracle=None)
    return R["draws"][seed]


def oracle_step(R, params, x, pi, v):
    """the oracle's cost and gradients on `params` (left in the oracle)"""
    ot = R["ot"]
    for i, p in enumerate(params):
        ot.set_param(i, p)
    co = ot.batch(x, pi, v, lr=0.0)
    return co, [ot.get_grad(i).astype(np.float64) for i in range(ot.num_params())]


def worst_ratio(g, g64):
    return max(float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)) for a, b in zip(g, g64))


@pytest.mark.parametrize("name", list(CASES))
def test_conditioning_reaches_its_margin_under_the_cap(name):
    """CPU: on both draws of every case no float64 pre-activation is left within tau of zero, fewer than 1e-3 of the units were moved, only
    betas and b1 differ from the unconditioned parameters, and the float32 model is within 1e-5 (reference_draw asserts the first two and
    the last; its results stay cached for the GPU tests of the same session)."""
    R = reference(name)
    for seed in SEEDS:
        D = reference_draw(name, seed)
        assert D["lo"] >= D["tau"] > 0 and D["moved"] < MOVED_CAP * D["units"]
        assert 2.0 ** round(np.log2(D["tau"])) == D["tau"] and D["tau"] >= 16 * D["d32"]
        for nm, p, q in zip(R["names"], R["params"], D["params"]):
            assert q.dtype == np.float32
            if not (nm.endswith("_beta") or nm == R["names"][-3]):      # (the value head's hidden bias: third from the end)
                np.testing.assert_array_equal(p, q, err_msg=nm)
            else:
                assert int((p != q).sum()) <= D["moved"], nm
        assert sum(int((p != q).sum()) for p, q in zip(R["params"], D["params"])) == D["moved"] > 0


def test_the_oracles_flip_is_its_own():
    """CPU, the witness: on the 65 910-row shape the fp32 oracle is more than 1e-3 of a tensor's maximum from float64 on the plain draw (a
    ReLU unit of its own forward on the other side of zero: measured 9.0e-3, L2_0_beta) and less than 1e-4 on the conditioned one (5.0e-5:
    what its sequential fp32 sums lose at this many rows).  Nothing but the betas of 7e2 of 6.5e6 units differs between the two."""
    R = reference(F_CASE)
    D = reference_draw(F_CASE, SEEDS[0])
    s = shape_args(R["conf"])
    _, g64_plain = f64_train(R["params"], D["x"], D["pi"], D["v"], *s)
    plain = worst_ratio(oracle_step(R, R["params"], D["x"], D["pi"], D["v"])[1], g64_plain)
    cond = worst_ratio(oracle_step(R, D["params"], D["x"], D["pi"], D["v"])[1], D["g64"])
    print("oracle vs float64, worst tensor: plain draw %.2e, conditioned %.2e" % (plain, cond))
    assert plain > 1e-3, plain
    assert cond < 1e-4, cond


# ---- the device against them
def trainer_for(ctx, name):
    """a device trainer of the case; the first one comes from make_pair, whose parameters must be the reference's"""
    R = reference(name)
    c = R["conf"]
    if not R["checked_pair"]:
        ot, dt = make_pair(ctx, *shape_args(c))
        for i, p in enumerate(R["params"]):
            np.testing.assert_array_equal(ot.get_param(i), p)
        del ot
        R["checked_pair"] = True
        return dt
    return A.Trainer(ctx, *shape_args(c))


def check_draw(R, name, dt, seed, mode, tag):
    """one forward / backward of `dt` on the conditioned draw; returns (worst device ratio, worst m32, widest bar, oracle ratio or None)"""
    D = reference_draw(name, seed)
    for i, p in enumerate(D["params"]):
        dt.set_param(i, p)
    cd = dt.forward_backward(D["x"], D["pi"], D["v"])
    c64, g64 = D["c64"], D["g64"]
    print("%s draw %d: cost device %.7g float64 %.7g" % (tag, seed, cd, c64))
    assert abs(cd - c64) <= 1e-4 * max(1.0, abs(c64)), (tag, seed, "cost", cd, c64)
    if name in ORACLE_CASES and D["oracle"] is None:
        D["oracle"] = oracle_step(R, D["params"], D["x"], D["pi"], D["v"])
    worst = wbar = wo = 0.0
    bad = []
    for i in range(len(g64)):
        gd = dt.get_grad(i).astype(np.float64)
        s64 = float(np.abs(g64[i]).max())
        bar = max(2e-5, FACTOR[mode] * D["m32"][i])
        e64 = np.abs(gd - g64[i])
        j = int(np.argmax(e64))
        worst, wbar = max(worst, e64[j] / (s64 + 1e-30)), max(wbar, bar)
        if not e64[j] <= bar * s64 + 1e-7:     # (not: a NaN fails)
            bad.append("%s: device-float64 %.2e of the tensor maximum %.3e (bar %.2e, m32 %.2e); worst at %s: device %.8g float64 %.8g"
                       % (R["names"][i], e64[j] / (s64 + 1e-30), s64, bar, D["m32"][i], where(R, i, j), gd[j], g64[i][j]))
        if D["oracle"] is not None:
            co, go = D["oracle"]
            so, eo = float(np.abs(go[i]).max()), np.abs(gd - go[i])
            wo = max(wo, float(eo.max()) / (so + 1e-30))
            if not eo.max() <= 2e-5 * so + 1e-7:
                k = int(np.argmax(eo))
                bad.append("%s: device-oracle %.2e of the tensor maximum %.3e (oracle-float64 %.2e); worst at %s: device %.8g oracle %.8g float64 %.8g"
                           % (R["names"][i], eo[k] / (so + 1e-30), so, np.abs(go[i] - g64[i]).max() / (s64 + 1e-30), where(R, i, k), gd[k], go[i][k], g64[i][k]))
    if D["oracle"] is not None:
        assert abs(cd - D["oracle"][0]) <= 1e-4 * max(1.0, abs(D["oracle"][0])), (tag, seed, "cost against the oracle", cd, D["oracle"][0])
    assert not bad, "%s draw %d:\n  " % (tag, seed) + "\n  ".join(bad)
    return worst, max(D["m32"]), wbar, (wo if D["oracle"] is not None else None)


def run_case(ctx, name, mode, hook=None):
    R = reference(name)
    c = R["conf"]
    for seed in SEEDS:      # (CPU, before the device is touched: margin, cap and the model's bar are asserted in there)
        reference_draw(name, seed)
    dt = trainer_for(ctx, name)
    dt.set_compute_mode(MODES[mode] | capi.COMPUTE_FORCE)
    if hook is not None:
        dt.set_dma_forward(hook)
    want = expected_paths(c["W"], c["H"], c["B"], c["K"], c["L"], mode, 1 if hook is None else int(hook))
    plan = row_plan(c["W"], c["H"], c["B"], c["K"], c["L"], mode) + [head_plan(c["W"], c["H"], c["B"], c["A"], c["FC"])]
    tag = "%s %s%s" % (name, mode, "" if hook is None else " hook %d" % int(hook))
    # what ran, and how the rows were dealt: asserted BEFORE anything is compared (the report is the launchers', filled by the step itself)
    D = reference_draw(name, SEEDS[0])
    for i, p in enumerate(D["params"]):
        dt.set_param(i, p)
    dt.forward_backward(D["x"], D["pi"], D["v"])
    got = [dt.last_paths(l) for l in range(c["L"] + 1)]
    assert got == want, (tag, "layers 0..L took", names_of(got), "the rules say", names_of(want))
    rows = [dt.last_rows(l) for l in range(c["L"] + 2)]
    assert rows == plan, (tag, "agz_trainer_last_rows", rows, "the rules say", plan)
    out = []
    for seed in SEEDS:
        out.append(check_draw(R, name, dt, seed, mode, tag))
        assert [dt.last_paths(l) for l in range(c["L"] + 1)] == want and [dt.last_rows(l) for l in range(c["L"] + 2)] == plan, (tag, seed)
    print("ROWS %s | %dx%d B=%d K=%d L=%d M=%d | %s | rows %s heads %s | tau %s moved %s of %d | device/max %.2e m32 %.2e bar %.2e%s"
          % (tag, c["W"], c["H"], c["B"], c["K"], c["L"], c["B"] * c["H"] * c["W"], " ; ".join("/".join(p) for p in names_of(got)),
             " ".join(str(list(r)) for r in rows[:-1]), list(rows[-1][:4]), "/".join("%.3g" % reference_draw(name, s)["tau"] for s in SEEDS),
             "/".join(str(reference_draw(name, s)["moved"]) for s in SEEDS), D["units"], max(o[0] for o in out), max(o[1] for o in out),
             max(o[2] for o in out), "" if out[0][3] is None else " | oracle/max %.2e" % max(o[3] for o in out)))
    dt.close()


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rows_wino_h2(ctx, name):
    run_case(ctx, name, "wino_h2")


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", ALL_MODE_CASES)
def test_rows_f32_and_bf16x3(ctx, name, mode):
    """k_wgrad and k_wgrad_x3 chunk their rows as k_wgrad_h2 does"""
    run_case(ctx, name, mode)


@gpu
@pytest.mark.parametrize("hook", [1 | 32, 0])
def test_rows_measured_board_other_forward_forms(ctx, hook):
    """case h with the forward convolution one tap per step (k_conv_h2dma) and through the staged split (conv3x3_h2w)"""
    run_case(ctx, H_CASE, "wino_h2", hook=hook)
