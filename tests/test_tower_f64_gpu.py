"""GPU: the inference tower's output — the tensor the heads read, agz_net_tower_out — element-wise against float64, per kernel path.

Every other network test meets its reference after softmax / tanh (atol 2e-5 on a policy near 1/362): a wrong tap at one board edge in
one of 256 channels, a lost hi*lo term of the fp16x2 split or a stale Winograd edge row cannot show there.  Here each case
  * builds a random network (init_random, gamma / beta as tame()), draws N(0, 1) float planes and scales board i by 4^((i mod 5) - 2), so
    the per-board range words of the fp16x2 modes differ inside one batch;
  * runs the device at the smallest batch (from the case's start value) at which the dispatch, restated below, takes the wanted kernels,
    and asserts what agz_net_last_paths reports against that restatement;
  * compares a subset of boards (boards are independent) with the float64 tower of tests/f64_tower.py in two metrics,
      local    max over (board, channel) of max_hw |dev - f64| / max(max_hw |f64[b, c]|, 1e-3 max |f64[b]|)
      diffuse  max over boards of rms(dev - f64) / rms(f64);
  * takes its bars from the matching fp32 CPU model on the same draw and boards — m32 (conv2d) for the direct paths, w32(4) for
    AGZ_COMPUTE_WINO, w32(agz_wino_h2_tile) for AGZ_COMPUTE_WINO_H2 — times 4 for the exact-fp32-product paths (the MFMA summation order
    differs from the model's) and times 8 for the split-product paths (bf16x3, fp16x2, latency fp16x2, both Winograd modes: products
    2^-22 .. 2^-23 relative against 2^-24, agz.h).
The heads are pinned separately: the device's own tower output through the float64 heads against what the same forward returned.
Model value, device value and bar of every case: profiles/tower_parity.md (each test prints its line, `pytest -s`).
"""
import collections

import numpy as np
import pytest
import torch

import agogo_amd as A
from agogo_amd import capi
from f64_tower import Tower, conv_direct, conv_wino, diffuse_metric, local_metric

pytestmark = pytest.mark.gpu

F32, X3, H2, WINO, AUTO, WINO_H2 = (capi.COMPUTE_F32_MFMA, capi.COMPUTE_BF16X3, capi.COMPUTE_FP16X2, capi.COMPUTE_WINO,
                                    capi.COMPUTE_AUTO, capi.COMPUTE_WINO_H2)
NUM_CUS = 256          # MI355X: the dispatch rules below count workgroups against it (agz_ctx::num_cus)
FC = 64


def cdiv(a, b):
    return -(-a // b)


# ---- the dispatch of agz_net::forward_packed, restated (fwd_plan, wino_h2_tower, wino_h2c_ok, wino_h2_pick_tm; net.hip) -------------
def pick_tm(H, W):
    return 5 if 49 * cdiv(H, 5) * cdiv(W, 5) < 36 * cdiv(H, 4) * cdiv(W, 4) else 4


def h2c_ok(H, W, tm, Kp):
    tpb = cdiv(H, tm) * cdiv(W, tm)
    return (Kp % 128 == 0 and 16 % tpb == 0 and Kp // 32 in (4, 8, 12, 16) and
            (16 // tpb) * (tm * cdiv(H, tm) + 2) * (tm * cdiv(W, tm) + 2) * 128 <= 80 * 1024)


def lat_ok(Kp, Wp):
    return Kp in (64, 128, 256) and 48 + 2 * (47 // (Wp - 2) + 1) + 2 * (Wp + 1) <= 100


def expect_paths(B, K, H, W, L, mode, force, form=-1, queues=0):
    """-> (input, block, heads) NPATH_* constants, rows of the GEMM's M dimension per board, boards per chunk (0: one chunk)"""
    Kp, HW, M = cdiv(K, 32) * 32, H * W, B * H * W
    cfg = 0 if Kp % 64 == 0 else 1
    half_init = cfg == 0 and cdiv(M, 128) * cdiv(Kp, 128) < NUM_CUS
    half_dual = cfg == 0 and cdiv(M, 128) * cdiv(2 * Kp, 128) < NUM_CUS
    tiles_dual = cdiv(M, 128) * cdiv(2 * Kp, 64) if cfg else cdiv(M, 64) * cdiv(2 * Kp, 128)
    small = Kp >= 64 and (tiles_dual * 4 <= NUM_CUS or (Kp >= 256 and tiles_dual <= NUM_CUS))
    forced_split = force and cfg == 0 and L > 0 and mode in (WINO_H2, WINO, X3, H2)
    latency = small and not forced_split
    heads_spread = small or B <= 64 or Kp >= 256
    split_ok = cfg == 0 and not latency and (not half_dual or force) and L > 0
    run_mode = (WINO_H2 if cfg == 0 else X3) if mode == AUTO else mode
    tm = pick_tm(H, W)
    tpb = cdiv(H, tm) * cdiv(W, tm)
    lat_h2 = latency and cfg == 0 and mode != F32 and L > 0 and lat_ok(Kp, W + 2) and cdiv(HW, 48) * (Kp // 8) <= 256
    if lat_h2 and Kp % 64 == 0 and cdiv(HW, 8) * (Kp // 64) <= 256:
        pin = capi.NPATH_IN_LAT
    elif split_ok and run_mode != F32 and Kp % 128 == 0:
        pin = capi.NPATH_IN_X3
    elif cfg:
        pin = capi.NPATH_IN_F32_411
    else:
        pin = capi.NPATH_IN_F32_221 if half_init else capi.NPATH_IN_F32_222
    rows, chunk = HW, 0
    if split_ok and run_mode == WINO_H2:
        rows = tpb
        if form != 0 and h2c_ok(H, W, tm, Kp):
            blk = capi.NPATH_BLK_WINO_H2_CHAINED
        else:
            wide = (2 * Kp) % 256 == 0 and (tm + 2) ** 2 * cdiv(B * tpb, 128) * ((2 * Kp) // 256) >= NUM_CUS
            blk = capi.NPATH_BLK_WINO_H2_3K_WIDE if wide else capi.NPATH_BLK_WINO_H2_3K
        if (queues == 2 or (queues == 0 and B >= 256)) and B >= 64:
            chunk = (B + 1) // 2
    elif split_ok and run_mode == H2:
        blk = capi.NPATH_BLK_H2W if (2 * Kp) % 256 == 0 else capi.NPATH_BLK_H2
    elif split_ok and run_mode == WINO:
        blk, rows = capi.NPATH_BLK_WINO, cdiv(H, 4) * cdiv(W, 4)
    elif split_ok and run_mode == X3:
        blk = capi.NPATH_BLK_X3
    elif lat_h2:
        blk = capi.NPATH_BLK_LAT_H2
    else:
        blk = capi.NPATH_BLK_F32_411 if cfg else (capi.NPATH_BLK_F32_221 if half_dual else capi.NPATH_BLK_F32_222)
        if latency:
            blk += 3    # the _SPLITK constants
    heads = (capi.NPATH_HEADS_SPREAD_NB4 if B >= 32 else capi.NPATH_HEADS_SPREAD) if heads_spread else capi.NPATH_HEADS_ONE
    return (pin, blk, heads), rows, chunk


SPLIT_PRODUCT_BLOCKS = (capi.NPATH_BLK_X3, capi.NPATH_BLK_H2W, capi.NPATH_BLK_H2, capi.NPATH_BLK_WINO, capi.NPATH_BLK_WINO_H2_3K,
                        capi.NPATH_BLK_WINO_H2_3K_WIDE, capi.NPATH_BLK_WINO_H2_CHAINED, capi.NPATH_BLK_LAT_H2)

Case = collections.namedtuple("Case", "id mode force K W H L B F want form queues bn")


def C(id, mode, force, K, W, H, L, B, want, F=2, form=-1, queues=0, bn=capi.BN_IDENTITY):
    return Case(id, mode, force, K, W, H, L, B, F, want, form, queues, bn)


IN, BLK = "NPATH_IN_", "NPATH_BLK_"
CASES = [
    # id, mode, FORCE, K, W, H, L, B to start from, wanted (input, block) kernels
    C("a-f32-222", F32, 0, 256, 9, 9, 2, 102, ("F32_222", "F32_222")),              # every M tile cuts a board (128 = 81 + 47)
    C("b-f32-221", F32, 0, 64, 7, 6, 2, 64, ("F32_221", "F32_221")),                # half tiles, non-square board
    C("c-f32-411", F32, 0, 96, 9, 9, 2, 16, ("F32_411", "F32_411"), F=18),          # cfg != 0
    C("c-f32-411-splitk", F32, 0, 96, 9, 9, 2, 16, ("F32_411", "F32_411_SPLITK"), F=18),
    C("d-f32-splitk-B1", F32, 0, 256, 19, 19, 2, 1, ("F32_221", "F32_221_SPLITK"), F=18),
    C("d-f32-splitk-B3", F32, 0, 256, 19, 19, 2, 3, ("F32_221", "F32_221_SPLITK"), F=18),
    C("e-x3", X3, 1, 128, 9, 9, 2, 37, ("X3", "X3"), F=18),
    C("f-x3-k64", X3, 1, 64, 7, 6, 1, 21, ("F32_221", "X3")),
    C("g-h2w", H2, 1, 128, 19, 19, 2, 5, ("X3", "H2W"), F=18),
    C("h-h2", H2, 1, 192, 9, 9, 2, 16, ("F32_221", "H2"), F=18),
    C("i-wino-7x5", WINO, 1, 64, 7, 5, 2, 9, ("F32_221", "WINO")),                  # ragged tiles in both directions
    C("i-wino-19", WINO, 1, 128, 19, 19, 1, 3, ("X3", "WINO"), F=18),               # 19 = 4 * 4 + 3
    C("j-h2c-19-L1", WINO_H2, 1, 128, 19, 19, 1, 5, ("X3", "WINO_H2_CHAINED"), F=18),   # one block is first and last
    C("j-h2c-19-L2", WINO_H2, 1, 128, 19, 19, 2, 5, ("X3", "WINO_H2_CHAINED"), F=18),
    C("j-h2c-19-L3", WINO_H2, 1, 128, 19, 19, 3, 5, ("X3", "WINO_H2_CHAINED"), F=18),   # an interior block: x and y never in memory
    # k, l, m: with FORCE as e .. j — at these batches the mode keeps its own tower only under it (fwd_plan: split_ok)
    C("k-h2c-9x9", WINO_H2, 1, 256, 9, 9, 3, 37, ("X3", "WINO_H2_CHAINED"), F=18),      # F(5x5), 4 tiles per board
    C("k-h2c-7x6", WINO_H2, 1, 128, 7, 6, 3, 21, ("X3", "WINO_H2_CHAINED")),            # F(4x4), 4 tiles per board
    C("k-h2c-16x16", WINO_H2, 1, 384, 16, 16, 2, 4, ("X3", "WINO_H2_CHAINED"), F=18),   # F(4x4), 16 tiles per board, nk 12
    # 5x5: one F(5x5) tile per board, nk 16.  wino_h2c_ok refuses it (16 haloed boards of 7 x 7 x 128 B are 98 KB of LDS, over the 80 KB
    # of two workgroups per CU), so the shape runs the three-kernel block; one F(4x4) tile per board (4x4) is the chained one-tile shape
    C("k-h2-3k-5x5", WINO_H2, 1, 512, 5, 5, 2, 16, ("X3", "WINO_H2_3K")),
    C("k-h2c-4x4", WINO_H2, 1, 512, 4, 4, 2, 16, ("X3", "WINO_H2_CHAINED")),
    # ... and once without: the smallest batch at which AGZ_COMPUTE_WINO_H2 alone reports the chained tower (the dual layer's 128-row
    # tiles fill the chip: 100 boards), 8 boards of it on the float64 side
    C("k-h2c-9x9-unforced", WINO_H2, 0, 256, 9, 9, 3, 37, ("X3", "WINO_H2_CHAINED"), F=18),
    C("l-h2c-2queues", WINO_H2, 1, 256, 19, 19, 2, 64, ("X3", "WINO_H2_CHAINED"), F=18, queues=2),   # boards 31 | 32
    C("m-h2-3k-13", WINO_H2, 1, 128, 13, 13, 2, 6, ("X3", "WINO_H2_3K"), F=18),         # 9 tiles per board: not chained
    C("m-h2-3k-k64", WINO_H2, 1, 64, 9, 9, 2, 16, ("F32_221", "WINO_H2_3K"), F=18),     # K % 128 != 0
    C("m-h2-3k-form0", WINO_H2, 1, 128, 19, 19, 2, 5, ("X3", "WINO_H2_3K"), F=18, form=0),
    C("m-h2-3k-wide", WINO_H2, 1, 256, 13, 13, 2, 24, ("X3", "WINO_H2_3K_WIDE"), F=18),
    C("o-h2c-bn-running", WINO_H2, 1, 128, 19, 19, 2, 5, ("X3", "WINO_H2_CHAINED"), F=18, bn=capi.BN_RUNNING),
    C("o-h2c-bn-eps", WINO_H2, 1, 128, 19, 19, 2, 5, ("X3", "WINO_H2_CHAINED"), F=18, bn=capi.BN_DEGENERATE_EPS),
]
# n: AGZ_COMPUTE_AUTO without FORCE, the latency regime: lat_input_kernel + conv_lat_h2_launch
# (an input layer with Fp != 32, which would leave lat_input_kernel, does not exist: agz_net_create refuses Features > 32)
for K_, W_ in ((64, 9), (128, 19), (256, 19)):
    for L_ in (2, 3):
        for B_ in (1, 8):
            if (K_, B_) == (128, 8):
                # 8 boards of 19x19 at K = 128 are 92 dual tiles: past the latency regime (4 * tiles <= 256 CUs), whose largest batch
                # here is 5.  Both are pinned: 5 boards in the regime, and 8 boards on what AUTO then runs (the fp32 half-tile kernels)
                CASES.append(C("n-lat-k128-19-L%d-B5" % L_, AUTO, 0, K_, W_, W_, L_, 5, ("LAT", "LAT_H2"), F=18))
                CASES.append(C("n-auto-k128-19-L%d-B8" % L_, AUTO, 0, K_, W_, W_, L_, 8, ("F32_221", "F32_221"), F=18))
            else:
                CASES.append(C("n-lat-k%d-%d-L%d-B%d" % (K_, W_, L_, B_), AUTO, 0, K_, W_, W_, L_, B_, ("LAT", "LAT_H2"), F=18))
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def find_batch(c):
    want = (getattr(capi, IN + c.want[0]), getattr(capi, BLK + c.want[1]))
    for B in range(c.B, c.B + 400):
        paths, rows, chunk = expect_paths(B, c.K, c.H, c.W, c.L, c.mode, bool(c.force), c.form, c.queues)
        if paths[:2] == want:
            return B, paths, rows, chunk
    raise AssertionError("%s: no batch from %d on takes %s" % (c.id, c.B, c.want))


def subset(B, rows, chunk):
    """all boards up to 8; else first, last, both sides of every chunk boundary, the boards cut by the first and the last 128-row
    boundary of the GEMM's M dimension (rows per board: pixels, or Winograd tiles), filled up to 8 with evenly spaced boards"""
    if B <= 8:
        return list(range(B))
    s = {0, B - 1}
    if chunk:
        for b in range(chunk, B, chunk):
            s |= {b - 1, b}
    M = B * rows
    for k in (128, ((M - 1) // 128) * 128):
        if 0 < k < M:
            s |= {(k - 1) // rows, k // rows}
    for b in np.linspace(0, B - 1, 9).astype(int):
        if len(s) >= 8:
            break
        s.add(int(b))
    return sorted(s)


def build_net(ctx, c, seed):
    A_space = c.W * c.H + 1
    net = A.Net(ctx, c.K, c.L, FC, c.W, c.H, c.F, A_space, bn_mode=c.bn)
    net.init_random(seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(net.num_params()):      # tame() of test_oracle_torch_xcheck.py
        name, n = net.param_info(i)
        if name.endswith("_gamma"):
            s = rng.uniform(0.5, 1.5, n).astype(np.float32)
            net.set_param(i, s * np.float32(np.sqrt(1e-5) if c.bn == capi.BN_DEGENERATE_EPS else 1.0))
        elif name.endswith("_beta") or name.endswith("_b"):
            net.set_param(i, rng.normal(0, 0.1, n).astype(np.float32))
    stats = None
    if c.bn == capi.BN_RUNNING:
        stats = []
        for bi, ch in enumerate([c.K] + [c.K, c.K] * c.L + [2, 1]):
            mean = rng.normal(0, 0.1, ch).astype(np.float32)
            var = rng.uniform(0.5, 1.5, ch).astype(np.float32)
            net.set_bn_stats(bi, mean, var)
            stats.append((mean, var))
    net.commit()
    net.set_compute_mode(c.mode | (capi.COMPUTE_FORCE if c.force else 0))
    if c.form >= 0:
        net.set_wino_h2_form(c.form)
    if c.queues:
        net.set_tower_queues(c.queues)
    conf = dict(K=c.K, SharedLayers=c.L, FC=FC, Width=c.W, Height=c.H, Features=c.F, ActionSpace=A_space)
    return net, [net.get_param(i) for i in range(net.num_params())], conf, stats


def draw_planes(B, c, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, c.F, c.H, c.W)).astype(np.float32)
    scale = np.float32(4.0) ** ((np.arange(B) % 5) - 2).astype(np.float32)
    return x * scale.reshape(B, 1, 1, 1)


Run = collections.namedtuple("Run", "c B paths want_paths rows chunk x P conf stats tower pol val")
_runs = {}


def run_case(ctx, cid):
    """one device forward per case, kept for the tower test and the heads test of the same case"""
    if cid in _runs:
        return _runs[cid]
    c = BY_ID[cid]
    B, want_paths, rows, chunk = find_batch(c)
    seed = 1000 + 17 * CASES.index(c)
    net, P, conf, stats = build_net(ctx, c, seed)
    try:
        x = draw_planes(B, c, seed + 5)
        pol, val = net.infer(x)
        paths = net.last_paths()
        tower = net.tower_out(B)
    finally:
        net.close()
    _runs[cid] = Run(c, B, paths, want_paths, rows, chunk, x, P, conf, stats, tower, pol, val)
    return _runs[cid]


def model_of(c, paths):
    """(name, convolution of the fp32 CPU model, margin) for the block kernels a case ran"""
    margin = 8 if paths[1] in SPLIT_PRODUCT_BLOCKS else 4
    if paths[1] == capi.NPATH_BLK_WINO:
        return "w32(4)", conv_wino(4), margin
    if paths[1] in (capi.NPATH_BLK_WINO_H2_3K, capi.NPATH_BLK_WINO_H2_3K_WIDE, capi.NPATH_BLK_WINO_H2_CHAINED):
        m = capi.wino_h2_tile(c.H, c.W)
        assert m == pick_tm(c.H, c.W)
        return "w32(%d)" % m, conv_wino(m), margin
    return "m32", conv_direct, margin


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_tower_output_against_float64(ctx, cid):
    r = run_case(ctx, cid)
    c = r.c
    assert r.paths == r.want_paths, "%s at B = %d: the device reports %s, the dispatch restated here gives %s" % (cid, r.B, r.paths, r.want_paths)
    if c.mode == WINO_H2:
        assert capi.wino_h2_chained(c.H, c.W, c.K) == int(h2c_ok(c.H, c.W, pick_tm(c.H, c.W), cdiv(c.K, 32) * 32))
    assert r.tower.shape == (r.B, c.K, c.H, c.W) and np.all(np.isfinite(r.tower))
    sub = subset(r.B, r.rows, r.chunk)
    assert len(sub) >= min(r.B, 8)
    name, conv, margin = model_of(c, r.paths)
    f64 = Tower(r.P, r.conf, c.bn, r.stats, torch.float64, conv_direct).tower(r.x[sub]).numpy()
    mod = Tower(r.P, r.conf, c.bn, r.stats, torch.float32, conv).tower(r.x[sub]).numpy()
    dev = r.tower[sub]
    loc_m, floored = local_metric(mod, f64)
    loc_d, _ = local_metric(dev, f64)
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nTOWER_PARITY | %s | B %d, boards %s | paths %s | %s x%d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (cid, r.B, ",".join(map(str, sub)), r.paths, name, margin, loc_m, loc_d, margin * loc_m, dif_m, dif_d, margin * dif_m))
    assert floored <= 0.05, "the dead-channel floor applies to %.1f %% of the (board, channel) pairs" % (100 * floored)
    assert np.abs(f64).max(axis=(1, 2, 3)).min() > 0 and loc_m > 0 and dif_m > 0
    assert loc_d <= margin * loc_m, "local: device %.3e, %s %.3e, bar %.3e" % (loc_d, name, loc_m, margin * loc_m)
    assert dif_d <= margin * dif_m, "diffuse: device %.3e, %s %.3e, bar %.3e" % (dif_d, name, dif_m, margin * dif_m)


# ---- the heads, from the device's own tower output ----------------------------------------------------------------------------------
HEAD_CASES = [
    ("a-f32-222", capi.NPATH_HEADS_SPREAD_NB4),          # K = 256: the spread form at every batch
    ("b-f32-221", capi.NPATH_HEADS_ONE),                 # heads_kernel
    ("d-f32-splitk-B1", capi.NPATH_HEADS_SPREAD),
    ("d-f32-splitk-B3", capi.NPATH_HEADS_SPREAD),
    ("k-h2c-9x9", capi.NPATH_HEADS_SPREAD_NB4),
    ("n-lat-k256-19-L2-B1", capi.NPATH_HEADS_SPREAD),
    ("n-heads-19-B40", capi.NPATH_HEADS_SPREAD_NB4),     # above the B >= 32 switch
]
CASES.append(C("n-heads-19-B40", AUTO, 0, 256, 19, 19, 2, 40, ("X3", "WINO_H2_CHAINED"), F=18))
BY_ID[CASES[-1].id] = CASES[-1]


@pytest.mark.parametrize("cid,heads_path", HEAD_CASES)
def test_heads_from_the_devices_own_tower(ctx, cid, heads_path):
    """policy |dp| / p per entry and |dv| between the forward's outputs and the float64 heads of the tower tensor the SAME forward left:
    the tower's error is out of the comparison.  Bars: the float32 heads' distance from the float64 heads on that tensor, times 4."""
    r = run_case(ctx, cid)
    c = r.c
    assert r.paths == r.want_paths and r.paths[2] == heads_path, (r.paths, r.want_paths, heads_path)
    sub = subset(r.B, r.rows, r.chunk) if r.B > 8 else list(range(r.B))
    if r.B >= 32:
        sub = sorted(set(sub) | set(range(r.B - 5, r.B)) | {3, 4})     # a whole group of four boards and the ragged last group
    t = r.tower[sub]
    p64, v64 = Tower(r.P, r.conf, c.bn, r.stats, torch.float64).heads(t)
    p32, v32 = Tower(r.P, r.conf, c.bn, r.stats, torch.float32).heads(t)
    pm = float((np.abs(p32 - p64) / p64).max())
    pd = float((np.abs(r.pol[sub] - p64) / p64).max())
    vm = float(np.abs(v32 - v64).max())
    vd = float(np.abs(r.val[sub] - v64).max())
    print("\nHEADS_PARITY | %s | B %d, boards %s | heads path %d | policy |dp|/p: model %.3e device %.3e bar %.3e | value |dv|: model %.3e device %.3e bar %.3e"
          % (cid, r.B, ",".join(map(str, sub)), r.paths[2], pm, pd, 4 * pm, vm, vd, 4 * vm))
    assert p64.min() > 0 and pm > 0 and vm > 0
    assert np.abs(p64 - p64[0]).max() > 1e-6 or r.B == 1          # boards give different outputs
    assert pd <= 4 * pm, "policy: device %.3e, fp32 heads %.3e" % (pd, pm)
    assert vd <= 4 * vm, "value: device %.3e, fp32 heads %.3e" % (vd, vm)


def test_tower_out_needs_a_forward_and_the_cases_cover_the_paths(ctx):
    net = A.Net(ctx, 32, 1, 16, 3, 3, 2, 10, bn_mode=capi.BN_IDENTITY)
    net.init_random(1)
    net.commit()
    assert net.last_paths() == (0, 0, 0)
    with pytest.raises(A.AgzError):
        net.tower_out(1)
    net.infer(np.ones((2, 2, 3, 3), np.float32))
    with pytest.raises(A.AgzError):
        net.tower_out(3)                       # not the batch the last forward ran
    assert net.tower_out(2).shape == (2, 32, 3, 3)
    net.close()
    got = [find_batch(c)[1] for c in CASES]
    assert {p[0] for p in got} == set(range(1, 6))
    # every block constant but one: <2,2,2> wants the dual layer's 128-row tiles to fill the chip (>= 256), the latency regime at most 256
    # of its 64-row tiles; both hold only at K = 16384 and one tile of rows, so NPATH_BLK_F32_222_SPLITK is out of reach of a test
    assert {p[1] for p in got} == set(range(1, 15)) - {capi.NPATH_BLK_F32_222_SPLITK}
    assert {p[2] for p in got} == {1, 2, 3}
