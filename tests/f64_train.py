"""The training network of dual.Train restated in float64 torch autograd — the high-precision reference of the trainer tests.

One restatement, built only from the topology (dualnet/dual.go, ermahagerdmonards.go) and the semantics oracle/train.hpp documents:
cross-correlation convolutions with "same" zero padding, training-mode BatchNorm (batch mean, BIASED batch variance, eps inside the
root) with full batch-shaped gamma / beta [B][C][H][W], ReLU, the dual block relu(a + b), channel-major head flattens, batch-shaped FC
biases, the reference's linear 'xent' on the logits -mean(Pi * z + (1 - Pi) * (1 - z)) and the MSE on the PRE-tanh value.

Used by tests/test_oracle_torch_xcheck.py (pins the oracle's backward), tests/test_train_wide_gpu.py (judges device and oracle against
float64) and scripts/debug/oracle_train_vs_f64.py.  A plain module: no fixtures, no GPU."""
import numpy as np
import torch
import torch.nn.functional as Fn


def f64_train(params, x, pi, v, K, L, FC, W, H, F, A, B, eps=1e-5, want_pre=False):
    """params: the learnables in the oracle's parameter order (flat or shaped arrays, any float type; e.g. [t.get_param(i) ...] of an
    oracle_lib.TrainNet); x [B][F][H][W], pi [B][A], v [B].
    Returns (cost, grads) — grads flat float64 arrays in the same order — or, with want_pre, (cost, grads, pre): pre[k] the float64
    pre-activation gamma * xhat + beta [B][C][H][W] of the k-th BatchNorm in evaluation order (init; a, b of each block; policy head;
    value head), i.e. the argument of its ReLU."""
    P = [torch.tensor(np.asarray(p, dtype=np.float64).ravel(), requires_grad=True) for p in params]
    it = iter(range(len(P)))
    pre = []

    def conv_bn_relu(z, cin, cout, k):
        w = P[next(it)].reshape(cout, cin, k, k)
        g = P[next(it)].reshape(B, cout, H, W)
        b = P[next(it)].reshape(B, cout, H, W)
        y = Fn.conv2d(z, w, padding=k // 2)
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        a = (y - mean) / torch.sqrt(var + eps) * g + b
        if want_pre:
            pre.append(a.detach().numpy())
        return torch.relu(a)

    z = torch.tensor(np.asarray(x, dtype=np.float64).reshape(B, F, H, W))
    z = conv_bn_relu(z, F, K, 3)
    for _ in range(L):
        a = conv_bn_relu(z, K, K, 3)
        b = conv_bn_relu(z, K, K, 3)
        z = torch.relu(a + b)
    p = conv_bn_relu(z, K, 2, 1).reshape(B, 2 * H * W)
    logits = p @ P[next(it)].reshape(2 * H * W, A) + P[next(it)].reshape(B, A)
    vv = conv_bn_relu(z, K, 1, 1).reshape(B, H * W)
    hid = torch.relu(vv @ P[next(it)].reshape(H * W, FC) + P[next(it)].reshape(B, FC))
    o = (hid @ P[next(it)].reshape(FC, 1) + P[next(it)].reshape(B, 1)).reshape(B)
    assert next(it, None) is None, "parameter list longer than the network"
    Pi = torch.tensor(np.asarray(pi, dtype=np.float64).reshape(B, A))
    V = torch.tensor(np.asarray(v, dtype=np.float64).reshape(B))
    cost = -(Pi * logits + (1 - Pi) * (1 - logits)).mean() + ((o - V) ** 2).mean()
    cost.backward()
    grads = [q.grad.numpy().ravel() for q in P]
    return (cost.item(), grads, pre) if want_pre else (cost.item(), grads)


def f64_train_of(t, x, pi, v, K, L, FC, W, H, F, A, B, **kw):
    """f64_train on the current parameters of an oracle_lib.TrainNet"""
    return f64_train([t.get_param(i) for i in range(t.num_params())], x, pi, v, K, L, FC, W, H, F, A, B, **kw)
