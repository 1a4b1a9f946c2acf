"""GPU: AGZ_COMPUTE_BF16_ACT (conv_bf16a.hpp) — AGZ_COMPUTE_BF16's declared arithmetic with the activations between blocks kept as bf16 in
device memory and both operands DMA'd into LDS.  The producer's epilogue rounds what the consumer's staging rounded, so:

  equal      tower output, policy and value of a forward are those of AGZ_COMPUTE_BF16 on the same net and planes, bit for bit, at every
             (K, board, blocks) that takes another path through the kernel; test_bf16_tower_gpu.py pins that mode against float64.
  float64    the tower output against the UNROUNDED float64 tower, the rule of test_bf16_tower_gpu.py::test_whole_tower_cascade_and_heads.
             Lines printed: profiles/bf16_act.md.
  batches    a board's tower output alone, last of three and inside 64: bit for bit.
  halo       a smaller batch of other planes between two forwards of the same planes changes nothing (the bf16 buffers' zero halo).
  refusals   K = 96, SharedLayers = 0: AGZ_E_UNSUPPORTED, and the net goes on in the mode it had.
"""
import numpy as np
import pytest
import torch

import agogo_amd as A
from agogo_amd import capi
from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
from test_tower_f64_gpu import C, build_net, draw_planes

pytestmark = pytest.mark.gpu
BF16, ACT = capi.COMPUTE_BF16, capi.COMPUTE_BF16_ACT


def conv_r(t, w):
    r = lambda v: v.float().bfloat16().double().to(t.dtype)
    return conv_direct(r(t), r(w))


#        K, W, H, F, L, B
CASES = [(64, 7, 6, 2, 1, 3),        # one block: AGZ_COMPUTE_BF16's kernel
         (64, 7, 6, 2, 2, 3),        # one chunk, less than one row block, <fp32 in, bf16 out> then <bf16 in, fp32 out>
         (128, 9, 9, 18, 3, 5),      # two chunks, <bf16, bf16> in the middle, odd width for the swizzle
         (128, 19, 19, 18, 4, 3),    # both LDS stages reused, 14 DMA rounds, line-end parity
         (192, 19, 19, 18, 3, 2),    # three chunks and three n-tiles
         (64, 21, 20, 2, 3, 2)]      # 420 pixels > 384: two runs per board, bf16 slices with line0 > 0
_runs = {}


def run(ctx, case):
    """one net per case, the same planes (boards scaled over 4^+-2, the last all zero) in both modes: kept for the float64 test"""
    if case not in _runs:
        K, W, H, F, L, B = case
        c = C("act", BF16, 0, K, W, H, L, B, None, F=F)
        net, P, conf, _ = build_net(ctx, c, 5100 + K + W + L)
        try:
            x = draw_planes(B, c, 5200 + K + W + L)
            x[B - 1] = 0
            out = {}
            for mode in (BF16, ACT):
                net.set_compute_mode(mode)
                pol, val = net.infer(x)
                out[mode] = (net.tower_out(B), pol, val, net.last_paths()[1])
        finally:
            net.close()
        _runs[case] = (c, P, conf, x, out)
    return _runs[case]


@pytest.mark.parametrize("case", CASES, ids=lambda s: "K%d-%dx%d-F%d-L%d-B%d" % s)
def test_equal_to_bf16_bit_for_bit(ctx, case):
    _, _, _, _, out = run(ctx, case)
    (t6, p6, v6, path6), (t7, p7, v7, path7) = out[BF16], out[ACT]
    assert path6 == capi.NPATH_BLK_BF16 and path7 == (capi.NPATH_BLK_BF16_ACT if case[4] >= 2 else capi.NPATH_BLK_BF16)
    assert t6.any() and np.array_equal(t6, t7) and np.array_equal(p6, p7) and np.array_equal(v6, v7)


@pytest.mark.parametrize("case", [CASES[3], CASES[1]], ids=lambda s: "K%d-%dx%d-L%d" % (s[0], s[1], s[2], s[4]))
def test_whole_tower_against_float64(ctx, case):
    c, P, conf, x, out = run(ctx, case)
    dev, pol, val, _ = out[ACT]
    f64t = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64 = f64t.tower(x).numpy()
    mod = Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_ACT_TOWER | K %d %dx%d L %d B %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (case[0], case[1], case[2], case[4], case[5], loc_m, loc_d, 2 * loc_m, dif_m, dif_d, 2 * dif_m))
    assert loc_d <= 2 * loc_m and dif_d <= 2 * dif_m
    p64, v64 = f64t.heads(dev)                 # the heads: fp32-grade kernels on the device's own tower output
    assert np.all(np.abs(pol - p64) <= 2e-5 + 1e-4 * np.abs(p64)) and np.all(np.abs(val - v64) <= 1e-4)


def test_a_board_does_not_depend_on_its_batch(ctx):
    c = C("bat", ACT, 0, 128, 19, 19, 3, 64, None, F=18)
    net, _, _, _ = build_net(ctx, c, 5300)
    try:
        x = draw_planes(64, c, 5301)
        net.infer(x)
        whole = net.tower_out(64)
        for j in (7, 63):
            net.infer(x[j:j + 1])
            alone = net.tower_out(1)[0]
            net.infer(x[[0, 1, j]])
            last = net.tower_out(3)[2]
            assert alone.any() and np.array_equal(alone, last) and np.array_equal(alone, whole[j])
    finally:
        net.close()


def test_halo_survives_reuse(ctx):
    c = C("halo", ACT, 0, 128, 9, 9, 3, 5, None, F=18)
    net, _, _, _ = build_net(ctx, c, 5400)
    try:
        x = draw_planes(5, c, 5401)
        net.infer(x)
        first = net.tower_out(5)
        net.infer(np.zeros_like(x[:2]))
        net.infer(x)
        assert net.last_paths()[1] == capi.NPATH_BLK_BF16_ACT and first.any() and np.array_equal(first, net.tower_out(5))
    finally:
        net.close()


@pytest.mark.parametrize("K,L", [(96, 2), (64, 0)])
def test_refused_nets_keep_their_mode(ctx, K, L):
    net, _, _, _ = build_net(ctx, C("ref", capi.COMPUTE_F32_MFMA, 0, K, 7, 6, L, 2, None), 5600 + K)
    try:
        x = draw_planes(2, C("ref", 0, 0, K, 7, 6, L, 2, None), 5601)
        before = net.infer(x)
        for mode in (ACT, ACT | capi.COMPUTE_FORCE):
            with pytest.raises(A.AgzError, match=r"\(-6\)"):       # AGZ_E_UNSUPPORTED
                net.set_compute_mode(mode)
        after = net.infer(x)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        net.close()
