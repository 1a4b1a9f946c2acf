"""GPU: AGZ_COMPUTE_FP16 — AGZ_COMPUTE_BF16_ACT's kernels and paths on IEEE half — against float64 models of its DECLARED arithmetic
(`fp16-tower`): conv_r(t, w) = conv2d(rne_half(clamp(t, +-65504)), rne_half(w 2^s_n) 2^-s_n), s_n per output filter.
Bars: one block, 4 x the same block in float32 on the rounded operands (test_bf16_tower_gpu.py's rule for exact-product paths); whole
tower against the UNROUNDED float64 tower, 2 x the float32 model's own distance (test_bf16_act_gpu.py's rule).  Lines printed: profiles/fp16_tower.md."""
import numpy as np
import pytest
import torch

import agogo_amd as A
from agogo_amd import capi
from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
from test_bf16_tower_gpu import block
from test_tower_f64_gpu import C, build_net, draw_planes

pytestmark = pytest.mark.gpu
FP16, ACT = capi.COMPUTE_FP16, capi.COMPUTE_BF16_ACT
P19, P20, P21, P22 = capi.NPATH_BLK_FP16, capi.NPATH_BLK_FP16_ACT, capi.NPATH_BLK_FP16_ACT_SMALL, capi.NPATH_BLK_FP16_ACT_PACKED


def conv_r(t, w):
    e = torch.frexp(w.double().abs().amax(dim=(1, 2, 3), keepdim=True))[1]       # max |w_n| = f 2^e, 0.5 <= f < 1
    s = torch.ldexp(torch.ones_like(e, dtype=torch.float64), 15 - e)              # 2^s_n: 2^14 <= max |w_n| 2^s_n < 2^15
    wr = (w.double() * s).float().half().double() / s
    return conv_direct(t.float().clamp(-65504, 65504).half().double().to(t.dtype), wr.to(t.dtype))


def distances(dev, mod, f64):
    return local_metric(mod, f64)[0], local_metric(dev, f64)[0], diffuse_metric(mod, f64), diffuse_metric(dev, f64)


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("K,W,H,B,shrink", [(64, 7, 6, 3, 0), (128, 9, 9, 5, 0), (128, 19, 19, 3, 0), (192, 19, 19, 2, 0), (64, 7, 6, 3, 1)])
def test_one_block_is_the_declared_arithmetic(ctx, K, W, H, B, shrink, layer):
    """shrink: every second filter of the block times 2^-20 and its gamma times 2^20 — without the per-filter scale fp16 zeros and subnormals"""
    c = C("blk", FP16, 0, K, W, H, 2, B, None)
    net, P, conf, _ = build_net(ctx, c, 8100 + K + W)
    try:
        if shrink:
            for i, f in ((3 + 6 * layer, 2.0 ** -20), (4 + 6 * layer, 2.0 ** 20), (6 + 6 * layer, 2.0 ** -20), (7 + 6 * layer, 2.0 ** 20)):
                P[i] = (P[i].reshape(K, -1) * np.where(np.arange(K) % 2, f, 1).reshape(K, 1)).astype(np.float32).ravel()
                net.set_param(i, P[i])
            net.commit()
        # boards scaled over 4^+-2, the last all zero, exact round-to-nearest-even ties of half (low 13 bits 0x1000) over even and odd bit 13
        x = draw_planes(B, C("x", FP16, 0, K, W, H, 1, B, None, F=K), 8200 + K + W + layer)
        u = x.reshape(B, -1).view(np.uint32)
        for k in range(8):
            u[:, 37 * k + 5] = (u[:, 37 * k + 5] & np.uint32(0xffffc000)) | np.uint32(0x1000 | ((k & 1) << 13))
        x[B - 1] = 0
        dev = net.block_forward(layer, x)
    finally:
        net.close()
    f64 = block(Tower(P, conf, c.bn, None, torch.float64, conv_r), x, layer)
    mod = block(Tower(P, conf, c.bn, None, torch.float32, conv_r), x, layer)
    loc_m, loc_d, dif_m, dif_d = distances(dev, mod, f64)
    sub = [local_metric(dev[i::5], f64[i::5])[0] for i in range(min(B - 1, 5))]     # per input scale 4^-2 .. 4^2: the subnormal operands are in the first
    print("\nFP16_BLOCK | K %d %dx%d B %d layer %d shrink %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e | local per scale %s"
          % (K, W, H, B, layer, shrink, loc_m, loc_d, 4 * loc_m, dif_m, dif_d, 4 * dif_m, " ".join("%.2e" % v for v in sub)))
    assert np.all(np.isfinite(dev)) and loc_m > 0 and dif_m > 0 and loc_d <= 4 * loc_m and dif_d <= 4 * dif_m


_towers = {}


def tower_run(ctx, K, W, H, F, L, B, scale=1.0):
    """one net per shape, the same planes under FP16 and BF16_ACT: (c, P, conf, x, {mode: (tower, policy, value)})"""
    if (K, W, H, L, B, scale) not in _towers:
        c = C("twr", FP16, 0, K, W, H, L, B, None, F=F)
        net, P, conf, _ = build_net(ctx, c, 8300 + K + L)
        try:
            x = draw_planes(B, c, 8400 + K + L) * np.float32(scale)
            out = {}
            for mode in (FP16, ACT):
                net.set_compute_mode(mode)
                pol, val = net.infer(x)
                out[mode] = (net.tower_out(B), pol, val)
        finally:
            net.close()
        _towers[K, W, H, L, B, scale] = (c, P, conf, x, out)
    return _towers[K, W, H, L, B, scale]


@pytest.mark.parametrize("K,W,H,F,L,B", [(128, 19, 19, 18, 4, 3), (64, 7, 6, 2, 2, 3)])
def test_whole_tower_against_float64_and_closer_than_bf16(ctx, K, W, H, F, L, B):
    c, P, conf, x, out = tower_run(ctx, K, W, H, F, L, B)
    (dev, pol, val), bf = out[FP16], out[ACT][0]
    f64t = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64, mod = f64t.tower(x).numpy(), Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    (loc_m, loc_d, dif_m, dif_d), loc_b, dif_b = distances(dev, mod, f64), local_metric(bf, f64)[0], diffuse_metric(bf, f64)
    print("\nFP16_TOWER | K %d %dx%d L %d B %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          "\nBF16_ACT_TOWER (same net and planes) | local: device %.3e | diffuse: device %.3e"
          % (K, W, H, L, B, loc_m, loc_d, 2 * loc_m, dif_m, dif_d, 2 * dif_m, loc_b, dif_b))
    assert loc_d <= 2 * loc_m and dif_d <= 2 * dif_m and loc_d < loc_b and dif_d < dif_b
    p64, v64 = f64t.heads(dev)                 # the heads: fp32-grade kernels on the device's own tower output
    assert np.all(np.abs(pol - p64) <= 2e-5 + 1e-4 * np.abs(p64)) and np.all(np.abs(val - v64) <= 1e-4)


@pytest.mark.parametrize("K,W,H", [(64, 7, 6)])
def test_activations_past_the_half_range_are_clamped(ctx, K, W, H):
    c, P, conf, x, _ = tower_run(ctx, K, W, H, 2, 2, 3)
    first = lambda v: Tower(P, dict(conf, SharedLayers=1), c.bn, None, torch.float64, conv_direct).tower(v).numpy()     # block 0's output
    scale = 2.0 ** np.ceil(np.log2(4 * 65504 / first(x).max()))
    c, P, conf, x, out = tower_run(ctx, K, W, H, 2, 2, 3, scale)
    b0 = first(x)
    assert np.all(np.isfinite(b0)) and (b0 > 65504).any() and not (b0 > 65504).all()
    dev, f64 = out[FP16][0], Tower(P, conf, c.bn, None, torch.float64, conv_direct).tower(x).numpy()
    mod = Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    loc_m, loc_d, dif_m, dif_d = distances(dev, mod, f64)
    print("\nFP16_CLAMP | K %d %dx%d planes x %g: %d of %d outputs of block 0 past 65504 | local: model %.3e device %.3e | diffuse: model %.3e device %.3e"
          % (K, W, H, scale, (b0 > 65504).sum(), b0.size, loc_m, loc_d, dif_m, dif_d))
    assert np.all(np.isfinite(dev)) and np.all(np.isfinite(mod)) and loc_d <= 2 * loc_m and dif_d <= 2 * dif_m


# (K, W, H, F, L, B): packed with G = 6 and a ragged last group; 9x9; 19x19, where no packed form exists; two runs per board; one block
@pytest.mark.parametrize("case", [(64, 7, 6, 2, 2, 7), (128, 9, 9, 18, 3, 5), (128, 19, 19, 18, 3, 2), (64, 21, 20, 2, 3, 2), (64, 7, 6, 2, 1, 3)],
                         ids=lambda s: "K%d-%dx%d-F%d-L%d-B%d" % s)
def test_the_forms_agree_bit_for_bit(ctx, case):
    K, W, H, F, L, B = case
    c = C("form", FP16, 0, K, W, H, L, B, None, F=F)
    net, _, _, _ = build_net(ctx, c, 8500 + K + W + L)
    try:
        x = draw_planes(B, c, 8600 + K + W + L)
        x[B - 1] = 0
        if L == 1:      # an input layer that copies plane k mod F to channel k exactly, so that the block's input is known on the host
            w = np.zeros((K, F, 3, 3), np.float32)
            w[np.arange(K), np.arange(K) % F, 1, 1] = 1
            [net.set_param(i, v.ravel()) for i, v in enumerate((w, np.ones(K * H * W, np.float32), np.zeros(K * H * W, np.float32)))]
            net.commit()                                       # rebuilds the fp16 images: the mode is on
        outs = []
        for small, packed in ((0, 0), (capi.BF16_SMALL_ALWAYS, 0), (0, capi.BF16_PACKED_ALWAYS)):
            net.set_bf16_small_batch(small)
            net.set_bf16_packed_boards(packed)
            pol, val = net.infer(x)
            outs.append((net.tower_out(B), pol, val, net.last_paths()[1]))
        alone = net.block_forward(0, np.maximum(x[:, np.arange(K) % F], 0)) if L == 1 else None
    finally:
        net.close()
    assert [o[3] for o in outs] == ([P19] * 3 if L == 1 else [P20, P21, P22 if capi.lib().agz_bf16_packed_boards_of(H, W) >= 2 else P20])
    assert outs[0][0].any() and all(np.array_equal(u, v) for o in outs[1:] for u, v in zip(outs[0][:3], o[:3]))
    assert alone is None or np.array_equal(alone, outs[0][0])


@pytest.mark.parametrize("K,W,H,L", [(128, 19, 19, 3), (64, 7, 6, 2)])
def test_batches_reuse_and_mode_switches(ctx, K, W, H, L):
    c = C("bat", ACT, 0, K, W, H, L, 64, None, F=18)
    net, _, _, _ = build_net(ctx, c, 8700 + K)
    tower = lambda v: (net.infer(v), net.tower_out(len(v)))[1]
    try:
        x = draw_planes(64, c, 8701 + K)
        bf, _, whole = tower(x[:5]), net.set_compute_mode(FP16), tower(x)
        for j in (7, 63):       # a board alone, last of three and inside 64
            alone = tower(x[j:j + 1])[0]
            assert alone.any() and np.array_equal(alone, tower(x[[0, 1, j]])[2]) and np.array_equal(alone, whole[j])
        first = tower(x[:5])
        tower(np.zeros_like(x[:2]))                            # a smaller forward of other planes in the same activation pair
        assert net.last_paths()[1] == P20 and np.array_equal(first, tower(x[:5])) and np.array_equal(first, whole[:5])
        for mode, want in ((ACT, bf), (FP16, first)):          # back and forth: each mode's own images and bits
            net.set_compute_mode(mode)
            assert np.array_equal(want, tower(x[:5])) and not np.array_equal(bf, first)
    finally:
        net.close()


@pytest.mark.parametrize("K,L", [(96, 2), (64, 0)])
def test_refused_nets_keep_their_mode(ctx, K, L):
    net, _, _, _ = build_net(ctx, C("ref", capi.COMPUTE_F32_MFMA, 0, K, 7, 6, L, 2, None), 8800 + K)
    try:
        x = draw_planes(2, C("ref", 0, 0, K, 7, 6, L, 2, None), 8801)
        before = net.infer(x)
        for mode in (FP16, FP16 | capi.COMPUTE_FORCE):
            with pytest.raises(A.AgzError, match=r"\(-6\)"):       # AGZ_E_UNSUPPORTED
                net.set_compute_mode(mode)
        assert all(np.array_equal(u, v) for u, v in zip(before, net.infer(x)))
    finally:
        net.close()
