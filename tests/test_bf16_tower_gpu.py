"""GPU: AGZ_COMPUTE_BF16 (conv_bf16.hpp) — one bf16 product per multiply, NOT fp32-grade — against float64 models of its DECLARED arithmetic
(`bf16-tower`): conv_r(t, w) = conv2d(rne_bf16(t), rne_bf16(w)), everything else as the other modes.

  one block    agz_net_block_forward against the float64 block over conv_r: the device differs by fp32 accumulation order only.  Bar: the
               same block in float32 on the already-rounded operands against the float64 one, times 4 (the MFMA's summation order is not
               the model's) — the rule of test_tower_f64_gpu.py for exact-product paths.  A truncating conversion, a wrong tap, a lost halo
               row or a swapped branch is three orders of magnitude over it.
  whole tower  agz_net_tower_out against the UNROUNDED float64 tower.  Device and float32 model round at the same points but flip different
               elements: the bar is the model's own distance from that tower, times 2.  Lines printed: profiles/bf16_tower.md.
  batches      a board's tower output alone, last of three and inside 64: bit for bit.
  refusals     K = 96, SharedLayers = 0: AGZ_E_UNSUPPORTED, and the net goes on in the mode it had.
"""
import numpy as np
import pytest
import torch

import agogo_amd as A
from agogo_amd import capi
from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
from test_tower_f64_gpu import C, build_net, draw_planes

pytestmark = pytest.mark.gpu
BF16 = capi.COMPUTE_BF16


def rne_bf16(v):
    return v.float().bfloat16().double()


def conv_r(t, w):
    return conv_direct(rne_bf16(t).to(t.dtype), rne_bf16(w).to(t.dtype))


def block(tw, x, l):
    """dual block l of a Tower on x [B, K, H, W], in the Tower's dtype"""
    K, pi, bi = tw.c["K"], 3 + 6 * l, 1 + 2 * l
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).to(tw.dtype)
    a = tw._bn_relu(tw.conv(t, tw.P[pi].reshape(K, K, 3, 3)), pi + 1, bi, K)
    b = tw._bn_relu(tw.conv(t, tw.P[pi + 3].reshape(K, K, 3, 3)), pi + 4, bi + 1, K)
    return torch.relu(a + b).numpy()


def draw_block_input(B, K, H, W, seed):
    """N(0, 1) float32 (not bf16-representable), board i scaled by 4^((i mod 5) - 2), exact round-to-nearest-even ties with even and odd
    upper halves in every board, the last board all zero"""
    x = draw_planes(B, C("x", BF16, 0, K, W, H, 1, B, None, F=K), seed)
    u = x.reshape(B, -1).view(np.uint32)
    for k in range(8):
        u[:, 37 * k + 5] = (u[:, 37 * k + 5] & np.uint32(0xfffe0000)) | np.uint32(0x8000 | ((k & 1) << 16))
    x[B - 1] = 0
    return x


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("K,W,H,B", [(64, 7, 6, 3), (128, 9, 9, 5), (128, 19, 19, 3), (192, 19, 19, 2)])
def test_one_block_is_the_declared_arithmetic(ctx, K, W, H, B, layer):
    c = C("blk", BF16, 0, K, W, H, 2, B, None)
    net, P, conf, _ = build_net(ctx, c, 4100 + K + W)
    try:
        x = draw_block_input(B, K, H, W, 4200 + K + W + layer)
        dev = net.block_forward(layer, x)
    finally:
        net.close()
    f64 = block(Tower(P, conf, c.bn, None, torch.float64, conv_r), x, layer)
    mod = block(Tower(P, conf, c.bn, None, torch.float32, conv_r), x, layer)
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_BLOCK | K %d %dx%d B %d layer %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (K, W, H, B, layer, loc_m, loc_d, 4 * loc_m, dif_m, dif_d, 4 * dif_m))
    assert np.all(np.isfinite(dev)) and loc_m > 0 and dif_m > 0
    assert loc_d <= 4 * loc_m and dif_d <= 4 * dif_m


@pytest.mark.parametrize("K,W,H,F,B", [(128, 19, 19, 18, 5), (64, 7, 6, 2, 3)])
def test_whole_tower_cascade_and_heads(ctx, K, W, H, F, B):
    c = C("twr", BF16, 0, K, W, H, 3, B, None, F=F)
    net, P, conf, _ = build_net(ctx, c, 4300 + K)
    try:
        x = draw_planes(B, c, 4400 + K)
        pol, val = net.infer(x)
        paths, dev = net.last_paths(), net.tower_out(B)
    finally:
        net.close()
    assert paths[1] == capi.NPATH_BLK_BF16
    f64t = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64 = f64t.tower(x).numpy()
    mod = Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_TOWER | K %d %dx%d L 3 B %d | paths %s | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (K, W, H, B, paths, loc_m, loc_d, 2 * loc_m, dif_m, dif_d, 2 * dif_m))
    assert loc_d <= 2 * loc_m and dif_d <= 2 * dif_m
    p64, v64 = f64t.heads(dev)                 # the heads: fp32-grade kernels on the device's own tower output
    assert np.all(np.abs(pol - p64) <= 2e-5 + 1e-4 * np.abs(p64)) and np.all(np.abs(val - v64) <= 1e-4)


def test_a_board_does_not_depend_on_its_batch(ctx):
    c = C("bat", BF16, 0, 128, 19, 19, 2, 64, None, F=18)
    net, _, _, _ = build_net(ctx, c, 4500)
    try:
        x = draw_planes(64, c, 4501)
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


@pytest.mark.parametrize("K,L", [(96, 2), (64, 0)])
def test_refused_nets_keep_their_mode(ctx, K, L):
    net, _, _, _ = build_net(ctx, C("ref", capi.COMPUTE_F32_MFMA, 0, K, 7, 6, L, 2, None), 4600 + K)
    try:
        x = draw_planes(2, C("ref", 0, 0, K, 7, 6, L, 2, None), 4601)
        before = net.infer(x)
        for mode in (BF16, BF16 | capi.COMPUTE_FORCE):
            with pytest.raises(A.AgzError, match=r"\(-6\)"):       # AGZ_E_UNSUPPORTED
                net.set_compute_mode(mode)
        after = net.infer(x)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        net.close()
