"""The dual network restated with torch / numpy at a chosen precision: the tower's output BEFORE the heads, and the heads from a
given tower tensor.  Built only from the topology in dualnet/dual.go:50-103 (test_oracle_torch_xcheck.py imports torch_forward
from here).  Three evaluations serve test_tower_f64_gpu.py:

    f64     float64, conv2d                      the reference
    m32     float32, conv2d                      the plain direct model: what fp32 rounding alone costs
    w32(m)  float32, numpy F(m x m, 3x3)         the Winograd model: transforms and products in fp32 with the Cook-Toom tables
                                                 COMPILED into the kernels (parsed from conv_wino_h2.hpp), ragged edge tiles zero-filled

The convolution implementation applies to the dual blocks' 3x3 convolutions.  The input convolution is always conv2d: no device
path runs that layer in the Winograd domain.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from test_wino_h2_tables_cpu import tables

BN_DEGENERATE_EPS, BN_RUNNING, BN_IDENTITY = 0, 1, 2


def conv_direct(t, w):
    return Fn.conv2d(t, w, padding=1)


def conv_wino(m):
    """F(m x m, 3x3) on [B, C, H, W] x [N, C, 3, 3] in the dtype of its arguments (numpy: every product and sum rounds to that dtype)"""
    al, _, BT, AT, G = tables(m)

    def conv(t, w):
        x, g = t.numpy(), w.numpy()
        dt = x.dtype
        bt, at, gm = (np.array([[float(v) for v in r] for r in M], dtype=dt) for M in (BT, AT, G))
        B, C, H, W = x.shape
        N = g.shape[0]
        nty, ntx = -(-H // m), -(-W // m)
        xp = np.zeros((B, C, nty * m + 2, ntx * m + 2), dtype=dt)
        xp[:, :, 1:H + 1, 1:W + 1] = x
        d = np.empty((B, C, nty, ntx, al, al), dtype=dt)
        for ty in range(nty):
            for tx in range(ntx):
                d[:, :, ty, tx] = xp[:, :, ty * m:ty * m + al, tx * m:tx * m + al]
        V = np.matmul(np.matmul(bt, d), bt.T)                                  # [B, C, nty, ntx, al, al]
        U = np.matmul(np.matmul(gm, g), gm.T)                                  # [N, C, al, al]
        Vp = np.ascontiguousarray(V.transpose(4, 5, 1, 0, 2, 3)).reshape(al * al, C, B * nty * ntx)
        Up = np.ascontiguousarray(U.transpose(2, 3, 0, 1)).reshape(al * al, N, C)
        Mp = np.matmul(Up, Vp).reshape(al, al, N, B, nty, ntx)                 # one GEMM per transform point
        Mt = np.ascontiguousarray(Mp.transpose(3, 2, 4, 5, 0, 1))              # [B, N, nty, ntx, al, al]
        Y = np.matmul(np.matmul(at, Mt), at.T)                                 # [B, N, nty, ntx, m, m]
        y = Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, N, nty * m, ntx * m)[:, :, :H, :W]
        assert y.dtype == dt
        return torch.from_numpy(np.ascontiguousarray(y))
    return conv


class Tower:
    """params: the learnables in the network's order (numpy); conf: dict with K, SharedLayers, FC, Width, Height, Features, ActionSpace;
    stats: [(mean, var)] per BatchNorm in the order input, (a, b) per block, policy, value (bn_mode BN_RUNNING only)"""

    def __init__(self, params, conf, bn_mode, stats=None, dtype=torch.float64, conv=conv_direct, eps=1e-5):
        self.c, self.bn_mode, self.stats, self.dtype, self.conv, self.eps = conf, bn_mode, stats, dtype, conv, eps
        self.P = [torch.from_numpy(np.asarray(p, dtype=np.float64)).to(dtype) for p in params]

    def _bn_relu(self, y, pi, bi, cout):
        H, W = self.c["Height"], self.c["Width"]
        g = self.P[pi].reshape(1, cout, H, W)
        b = self.P[pi + 1].reshape(1, cout, H, W)
        if self.bn_mode == BN_DEGENERATE_EPS:
            y = y / torch.sqrt(torch.tensor(0.0 + self.eps, dtype=self.dtype))
        elif self.bn_mode == BN_RUNNING:
            mean, var = self.stats[bi]
            mean = torch.from_numpy(np.asarray(mean, dtype=np.float64)).to(self.dtype).reshape(1, -1, 1, 1)
            var = torch.from_numpy(np.asarray(var, dtype=np.float64)).to(self.dtype).reshape(1, -1, 1, 1)
            y = (y - mean) / torch.sqrt(var + self.eps)
        return torch.relu(y * g + b)

    def tower(self, x):
        """[B, F, H, W] planes -> the tower's output [B, K, H, W] (a torch tensor of this Tower's dtype)"""
        K, L, F = self.c["K"], self.c["SharedLayers"], self.c["Features"]
        t = torch.from_numpy(np.asarray(x, dtype=np.float64)).to(self.dtype)
        t = self._bn_relu(conv_direct(t, self.P[0].reshape(K, F, 3, 3)), 1, 0, K)
        for l in range(L):
            pi, bi = 3 + 6 * l, 1 + 2 * l
            a = self._bn_relu(self.conv(t, self.P[pi].reshape(K, K, 3, 3)), pi + 1, bi, K)
            b = self._bn_relu(self.conv(t, self.P[pi + 3].reshape(K, K, 3, 3)), pi + 4, bi + 1, K)
            t = torch.relu(a + b)
        return t

    def heads(self, t):
        """a tower tensor [B, K, H, W] (numpy or torch) -> (policy [B, A], value [B]) as numpy arrays of this Tower's dtype"""
        c = self.c
        K, L, FC, H, W, A = c["K"], c["SharedLayers"], c["FC"], c["Height"], c["Width"], c["ActionSpace"]
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.asarray(t, dtype=np.float64))
        t = t.to(self.dtype)
        pi, bi = 3 + 6 * L, 1 + 2 * L
        p = self._bn_relu(Fn.conv2d(t, self.P[pi].reshape(2, K, 1, 1)), pi + 1, bi, 2).reshape(-1, 2 * H * W)
        Wp, bp = self.P[pi + 3].reshape(2 * H * W, A), self.P[pi + 4]
        pol = torch.softmax(p @ Wp + bp, dim=1)
        v = self._bn_relu(Fn.conv2d(t, self.P[pi + 5].reshape(1, K, 1, 1)), pi + 6, bi + 1, 1).reshape(-1, H * W)
        W1, b1 = self.P[pi + 8].reshape(H * W, FC), self.P[pi + 9]
        W2, b2 = self.P[pi + 10].reshape(FC, 1), self.P[pi + 11]
        val = torch.tanh(torch.relu(v @ W1 + b1) @ W2 + b2).reshape(-1)
        return pol.numpy(), val.numpy()


def params_of(net):
    return [net.get_param(i) for i in range(net.num_params())]


def torch_forward(net, x, bn_mode, stats=None, eps=1e-5):
    """float64 forward of an oracle / device net object (conf as a dict): (policy, value)"""
    tw = Tower(params_of(net), net.conf, bn_mode, stats, torch.float64, conv_direct, eps)
    return tw.heads(tw.tower(x))


# ---- the two metrics of test_tower_f64_gpu.py (dev, ref: [n, K, H, W]; ref in float64) ----------------------------------------
def local_metric(dev, ref, floor_rel=1e-3):
    """per board b and channel c: max_hw |dev - ref| / max(max_hw |ref[b, c]|, floor_rel * max |ref[b]|): (maximum, fraction of (b, c)
    pairs the floor applies to).  A wrong tap, edge tile, index or epilogue constant moves this."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    err = np.abs(dev - ref).max(axis=(2, 3))
    cmax = np.abs(ref).max(axis=(2, 3))
    floor = floor_rel * np.abs(ref).max(axis=(1, 2, 3), keepdims=False)[:, None]
    return float((err / np.maximum(cmax, floor)).max()), float((cmax < floor).mean())


def diffuse_metric(dev, ref):
    """per board: rms(dev - ref) / rms(ref), the maximum.  A lost cross term or a dropped low piece moves this; rounding averages out."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    num = np.sqrt(((dev - ref) ** 2).mean(axis=(1, 2, 3)))
    den = np.sqrt((ref ** 2).mean(axis=(1, 2, 3)))
    return float((num / den).max())
