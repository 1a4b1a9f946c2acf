"""The training network under AGZ_COMPUTE_BF16 (`bf16-train`) restated in torch autograd: tests/f64_train.py's network,
line for line, with the dual blocks' 3x3 convolutions replaced by the declared arithmetic — r(.) one round-to-nearest-even to bfloat16:

    forward          z  = conv3x3(r(x), r(w))
    data gradient    dx = conv3x3(r(dz), r(w) transposed, taps flipped)
    weight gradient  dw = sum_m r(dz)[m] * r(x)[pix(m) + tap]

The input layer, BatchNorm, the heads and the loss are f64_train's; `tied` as in f64_train_az.  A plain module: no fixtures, no GPU."""
import numpy as np
import torch
import torch.nn.functional as Fn


def r(t):
    return t.float().bfloat16().to(t.dtype)


class ConvR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        xr, wr = r(x), r(w)
        ctx.save_for_backward(xr, wr)
        return Fn.conv2d(xr, wr, padding=1)

    @staticmethod
    def backward(ctx, dz):
        xr, wr = ctx.saved_tensors
        dzr = r(dz)
        dx = Fn.conv_transpose2d(dzr, wr, padding=1)
        dw = Fn.conv2d(xr.transpose(0, 1), dzr.transpose(0, 1), padding=1).transpose(0, 1)
        return dx, dw


def f64_train_bf16(params, x, pi, v, K, L, FC, W, H, F, A, B, eps=1e-5, dtype=np.float64, tied=False, want_pre=False, rounded=True):
    """(cost, grads[, pre]) as f64_train; the two convolutions of a block run as one ConvR over [a | b], as on the device (dz of both
    branches is one tensor, rounded once).  rounded=False: f64_train's own network (no r(.) anywhere), tied or not"""
    P = [torch.tensor(np.asarray(p, dtype=dtype).ravel(), requires_grad=True) for p in params]
    it = iter(range(len(P)))
    R = 1 if tied else B
    pre = []

    def bn_relu(y, cout):
        g = P[next(it)].reshape(R, cout, H, W)
        b = P[next(it)].reshape(R, cout, H, W)
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        a = (y - mean) / torch.sqrt(var + eps) * g + b
        pre.append(a.detach().numpy())
        return torch.relu(a)

    z = torch.tensor(np.asarray(x, dtype=dtype).reshape(B, F, H, W))
    z = bn_relu(Fn.conv2d(z, P[next(it)].reshape(K, F, 3, 3), padding=1), K)
    for _ in range(L):
        ia = next(it)
        wa, wb = P[ia].reshape(K, K, 3, 3), P[ia + 3].reshape(K, K, 3, 3)
        y = ConvR.apply(z, torch.cat([wa, wb])) if rounded else Fn.conv2d(z, torch.cat([wa, wb]), padding=1)
        a = bn_relu(y[:, :K], K)
        next(it)
        b = bn_relu(y[:, K:], K)
        z = torch.relu(a + b)
    p = bn_relu(Fn.conv2d(z, P[next(it)].reshape(2, K, 1, 1)), 2).reshape(B, 2 * H * W)
    logits = p @ P[next(it)].reshape(2 * H * W, A) + P[next(it)].reshape(R, A)
    vv = bn_relu(Fn.conv2d(z, P[next(it)].reshape(1, K, 1, 1)), 1).reshape(B, H * W)
    hpre = vv @ P[next(it)].reshape(H * W, FC) + P[next(it)].reshape(R, FC)
    pre.append(hpre.detach().numpy())
    o = (torch.relu(hpre) @ P[next(it)].reshape(FC, 1) + P[next(it)].reshape(R, 1)).reshape(B)
    assert next(it, None) is None, "parameter list longer than the network"
    Pi = torch.tensor(np.asarray(pi, dtype=dtype).reshape(B, A))
    V = torch.tensor(np.asarray(v, dtype=dtype).reshape(B))
    cost = -(Pi * logits + (1 - Pi) * (1 - logits)).mean() + ((o - V) ** 2).mean()
    cost.backward()
    grads = [q.grad.numpy().ravel().astype(np.float64) for q in P]
    return (cost.item(), grads, pre) if want_pre else (cost.item(), grads)
