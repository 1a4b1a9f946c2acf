"""CPU: the models test_tower_f64_gpu.py takes its bars from (tests/f64_tower.py).  The numpy Winograd convolution w(m), built from the
Cook-Toom tables compiled into the kernels, IS the direct convolution: in float64 the tower through it equals the tower through conv2d
to 1e-12 (of the tower's largest activation), on a board with 5+5+5+4 tiles, on a non-square one and on one with four tiles.  In float32
the same model is measurably further from float64 than the direct model — the reason the Winograd paths get a bar of their own."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from f64_tower import Tower, conv_direct, conv_wino, diffuse_metric, params_of
from test_oracle_torch_xcheck import tame


def _net(K, L, W, H, F, seed):
    net = O.Net(K, L, 16, W, H, F, W * H + 1, bn_mode=2)
    net.init_random(seed)
    tame(net, seed + 1, 2)
    rng = np.random.default_rng(seed + 2)
    x = rng.normal(0, 1, (3, F, H, W)).astype(np.float32)
    x *= np.float32(4.0) ** (np.arange(3) - 1).reshape(3, 1, 1, 1).astype(np.float32)
    return net, x


@pytest.mark.parametrize("m", [4, 5])
@pytest.mark.parametrize("W,H", [(19, 19), (7, 6), (9, 9)])
def test_winograd_model_equals_the_direct_tower_in_float64(W, H, m):
    net, x = _net(32, 2, W, H, 2, 10 * W + m)
    P = params_of(net)
    ref = Tower(P, net.conf, 2, None, torch.float64, conv_direct).tower(x).numpy()
    win = Tower(P, net.conf, 2, None, torch.float64, conv_wino(m)).tower(x).numpy()
    assert ref.shape == (3, 32, H, W) and np.abs(ref).max() > 0.1
    assert np.abs(win - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_float32_models_sit_where_expected():
    """m32 within a few fp32 ulps (rms) of float64; w32(5) further away than m32 but still fp32-grade"""
    net, x = _net(32, 2, 9, 9, 18, 77)
    P = params_of(net)
    ref = Tower(P, net.conf, 2, None, torch.float64, conv_direct).tower(x).numpy()
    m32 = Tower(P, net.conf, 2, None, torch.float32, conv_direct).tower(x).numpy()
    w32 = Tower(P, net.conf, 2, None, torch.float32, conv_wino(5)).tower(x).numpy()
    assert m32.dtype == np.float32 and w32.dtype == np.float32
    dm, dw = diffuse_metric(m32, ref), diffuse_metric(w32, ref)
    assert 0 < dm < 2.0 ** -20 and dm < dw < 2.0 ** -17, (dm, dw)
