"""GPU: AGZ_COMPUTE_BF16 in the trainer (train_bf16.hpp) — one bf16 product per multiply, NOT fp32-grade — against float64 models of its
DECLARED arithmetic (`bf16-train`); r(.) = one round to nearest even to bfloat16.

  kernels      agz_trainer_conv_bf16 (the step's rounding kernels and launchers) against float64 torch on r(.) of the operands: the device
               differs by fp32 summation order only.  Bar: the same in float32 on the already-rounded operands, times 4, on both metrics of
               f64_tower.py — test_bf16_tower_gpu.py's rule for exact-product paths.  The all-zero last board must come out exactly zero.
  whole step   K = 64, 7x6, L = 2, B = 8, plain and tied: the three *_BF16T paths on layers 1..2, the BF16X3 ones on layer 0, and every
               gradient tensor against tests/f64_train_bf16.py.  Device and float32 model round at the same points but flip different
               elements: the bar is that model's distance from the UNROUNDED float64 gradients, times 2, on the diffuse metric.  The plain
               draw is made well-posed by f64_train.condition with tau = 16 x the bf16 model's largest pre-activation distance from float64
               (measured_tau's rule on that model); a tied net has no per-unit beta to move and runs its draw as it is.
               Printed lines: profiles/train_bf16.md.
  off          a WINO_H2 | FORCE trainer before and after a round trip through BF16: same cost bits, same paths.
  refusals     K = 96, SharedLayers = 0: AGZ_E_UNSUPPORTED; BF16_ACT, FP16: AGZ_E_INVALID; the next step's cost is bit-equal.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import agogo_amd as A
from agogo_amd import capi
from f64_tower import diffuse_metric, local_metric
from f64_train import condition
from f64_train_az import draw_batch, draw_params
from f64_train_bf16 import f64_train_bf16, r
from test_bf16_tower_gpu import draw_block_input

pytestmark = pytest.mark.gpu
BF16, FORCE = capi.COMPUTE_BF16, capi.COMPUTE_FORCE


def judge(which, a, b, dtype):
    """a, b NCHW / [Cout, Cin, 3, 3] numpy -> the result of GEMM `which` on r(.) of them in `dtype`: [n, C, H, W] (which 2: [1, 9, Cout, Cin])"""
    a, b = r(torch.from_numpy(a).to(dtype)), r(torch.from_numpy(b).to(dtype))
    if which == 0:
        return Fn.conv2d(a, b, padding=1).numpy()
    if which == 1:
        return Fn.conv_transpose2d(a, b, padding=1).numpy()
    dw = Fn.conv2d(b.transpose(0, 1), a.transpose(0, 1), padding=1)          # [Cin, Cout, 3, 3]
    return dw.permute(2, 3, 1, 0).reshape(1, 9, a.shape[1], b.shape[1]).numpy()


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("K,W,H,B", [(64, 7, 6, 3), (128, 9, 9, 5), (64, 19, 19, 2), (192, 19, 19, 2)])
def test_each_kernel_is_the_declared_arithmetic(ctx, K, W, H, B, which):
    x = draw_block_input(B, K, H, W, 5100 + K + W)
    dz = draw_block_input(B, 2 * K, H, W, 5200 + K + W)
    w = np.random.default_rng(5300 + K + W).normal(0, 1.0 / np.sqrt(9 * K), (2 * K, K, 3, 3)).astype(np.float32)
    u = w.reshape(-1).view(np.uint32)
    for k in range(8):                                                        # exact ties, even and odd upper halves, in the filter too
        u[131 * k + 3] = (u[131 * k + 3] & np.uint32(0xfffe0000)) | np.uint32(0x8000 | ((k & 1) << 16))
    a, b = (x, w) if which == 0 else (dz, w) if which == 1 else (dz, x)
    nhwc = lambda t: np.ascontiguousarray(t.transpose(0, 2, 3, 1))
    dev = capi.trainer_conv_bf16(ctx, which, nhwc(a), b if which < 2 else nhwc(b))
    f64, mod = judge(which, a, b, torch.float64), judge(which, a, b, torch.float32)
    if which < 2:
        dev = dev.transpose(0, 3, 1, 2)
        assert not dev[B - 1].any() and not f64[B - 1].any()                  # the all-zero board: exactly zero, then left out of the ratios
        dev, f64, mod = dev[:B - 1], f64[:B - 1], mod[:B - 1]
    else:
        dev = dev.reshape(1, 9, 2 * K, K)
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_TRAIN_KERNEL | which %d K %d %dx%d B %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (which, K, W, H, B, loc_m, loc_d, 4 * loc_m, dif_m, dif_d, 4 * dif_m))
    assert np.all(np.isfinite(dev)) and loc_m > 0 and dif_m > 0
    assert loc_d <= 4 * loc_m and dif_d <= 4 * dif_m


CASE = (64, 2, 32, 7, 6, 2, 43, 8)          # K, L, FC, W, H, F, A, B


def rel_rms(g, ref):
    return float(np.sqrt(((g - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))


@pytest.mark.parametrize("tied", [False, True])
def test_a_whole_step_takes_the_new_paths_and_computes_the_declared_network(ctx, tied):
    K, L = CASE[0], CASE[1]
    P = draw_params(CASE, 5400, tied)
    x, pi, v = draw_batch(CASE, 5401, "onehot")
    if not tied:
        _, _, pre64 = f64_train_bf16(P, x, pi, v, *CASE, want_pre=True, rounded=False)
        _, _, prem = f64_train_bf16(P, x, pi, v, *CASE, want_pre=True, dtype=np.float32)
        d = max(float(np.abs(p.astype(np.float64) - q).max()) for p, q in zip(prem, pre64))
        tau = float(2.0 ** np.ceil(np.log2(16 * d)))
        P, moved, units, lo = condition(P, x, pi, v, *CASE, tau)
        print("\nBF16_TRAIN_STEP | plain | bf16 model's largest pre-activation distance %.3e tau %.3g moved %d of %d units, min |pre64| %.3g" % (d, tau, moved, units, lo))
    _, g64 = f64_train_bf16(P, x, pi, v, *CASE, tied=tied, rounded=False)      # the unrounded network
    _, g64r = f64_train_bf16(P, x, pi, v, *CASE, tied=tied)                    # the declared arithmetic in float64
    _, gm = f64_train_bf16(P, x, pi, v, *CASE, tied=tied, dtype=np.float32)    # ... in float32: the ruler
    dt = A.Trainer(ctx, *CASE, tied=tied)
    try:
        for i, p in enumerate(P):
            dt.set_param(i, p)
        dt.set_compute_mode(capi.COMPUTE_BF16X3 | FORCE)                       # what that mode runs for the input layer (18 -> K: below its
        dt.forward_backward(x, pi, v)                                          # own 64-channel limit the forward is the fp32 kernel)
        x3_layer0 = dt.last_paths(0)[:3]
        dt.set_compute_mode(BF16 | FORCE)
        dt.forward_backward(x, pi, v)
        paths = [dt.last_paths(l)[:3] for l in range(L + 1)]
        gd = [dt.get_grad(i).astype(np.float64) for i in range(len(P))]
    finally:
        dt.close()
    assert paths[0] == x3_layer0 and paths[0][1] == capi.PATH_WGRAD_X3, (paths, x3_layer0)
    assert paths[1:] == [(capi.PATH_FWD_BF16T, capi.PATH_WGRAD_BF16T, capi.PATH_DGRAD_BF16T)] * L, paths
    bad = []
    for i in range(len(P)):
        m, dv, dr = rel_rms(gm[i], g64[i]), rel_rms(gd[i], g64[i]), rel_rms(gd[i], g64r[i])
        print("BF16_TRAIN_STEP | %s | tensor %2d | from the unrounded float64: model %.3e device %.3e bar %.3e | device from the float64 model %.3e"
              % ("tied" if tied else "plain", i, m, dv, 2 * m, dr))
        if not dv <= 2 * m:
            bad.append(i)
    assert not bad, bad


def test_off_is_untouched(ctx):
    P = draw_params(CASE, 5500)
    x, pi, v = draw_batch(CASE, 5501, "onehot")
    dt = A.Trainer(ctx, *CASE)
    try:
        for i, p in enumerate(P):
            dt.set_param(i, p)
        dt.set_compute_mode(capi.COMPUTE_WINO_H2 | FORCE)
        c0 = dt.forward_backward(x, pi, v)
        p0 = [dt.last_paths(l) for l in range(CASE[1] + 1)]
        dt.set_compute_mode(BF16)
        dt.set_compute_mode(capi.COMPUTE_WINO_H2 | FORCE)
        c1 = dt.forward_backward(x, pi, v)
        assert np.float32(c0).tobytes() == np.float32(c1).tobytes() and p0 == [dt.last_paths(l) for l in range(CASE[1] + 1)]
    finally:
        dt.close()


@pytest.mark.parametrize("K,L", [(96, 2), (64, 0)])
def test_refusals_keep_the_mode(ctx, K, L):
    case = (K, L) + CASE[2:]
    P = draw_params(case, 5600)
    x, pi, v = draw_batch(case, 5601, "onehot")
    dt = A.Trainer(ctx, *case)
    try:
        for i, p in enumerate(P):
            dt.set_param(i, p)
        dt.set_compute_mode(capi.COMPUTE_BF16X3 | FORCE)
        c0 = dt.forward_backward(x, pi, v)
        for mode, code in ((BF16, -6), (BF16 | FORCE, -6), (capi.COMPUTE_BF16_ACT, -1), (capi.COMPUTE_FP16, -1)):
            with pytest.raises(A.AgzError, match=r"\(%d\)" % code):
                dt.set_compute_mode(mode)
        c1 = dt.forward_backward(x, pi, v)
        assert np.float32(c0).tobytes() == np.float32(c1).tobytes()
    finally:
        dt.close()
