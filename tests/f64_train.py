"""The training network of dual.Train restated in float64 torch autograd — the high-precision reference of the trainer tests.

One restatement, built only from the topology (dualnet/dual.go, ermahagerdmonards.go) and the semantics oracle/train.hpp documents:
cross-correlation convolutions with "same" zero padding, training-mode BatchNorm (batch mean, BIASED batch variance, eps inside the
root) with full batch-shaped gamma / beta [B][C][H][W], ReLU, the dual block relu(a + b), channel-major head flattens, batch-shaped FC
biases, the reference's linear 'xent' on the logits -mean(Pi * z + (1 - Pi) * (1 - z)) and the MSE on the PRE-tanh value.

Used by tests/test_oracle_torch_xcheck.py (pins the oracle's backward), tests/test_train_wide_gpu.py (judges device and oracle against
float64), tests/test_train_rows_gpu.py (float64 as the only judge, on draws made well-posed by condition() below, with the same network in
float32 — dtype — as the ruler of what fp32 arithmetic can hold) and scripts/debug/oracle_train_vs_f64.py.  A plain module: no fixtures, no GPU."""
import numpy as np
import torch
import torch.nn.functional as Fn


def f64_train(params, x, pi, v, K, L, FC, W, H, F, A, B, eps=1e-5, want_pre=False, dtype=np.float64, want_grad=True, chunk_rows=None):
    """params: the learnables in the oracle's parameter order (flat or shaped arrays, any float type; e.g. [t.get_param(i) ...] of an
    oracle_lib.TrainNet); x [B][F][H][W], pi [B][A], v [B].
    Returns (cost, grads) — grads flat float64 arrays in the same order — or, with want_pre, (cost, grads, pre): pre[k] the float64
    pre-activation gamma * xhat + beta [B][C][H][W] of the k-th BatchNorm in evaluation order (init; a, b of each block; policy head;
    value head), i.e. the argument of its ReLU; want_pre="all" appends the argument [B][FC] of the value head's hidden ReLU, so that pre then
    holds every ReLU unit of the network.  dtype=np.float32: the same network in float32 torch (the fp32 model; its gradients are returned
    as float64 arrays all the same).  want_grad=False: the forward alone, grads is None.  chunk_rows: every convolution runs over chunks of
    whole boards of at most that many rows (B H W), so its weight gradient is summed within a chunk first and over the chunks after — the
    order of any fp32 implementation at thousands of rows (the device's k_wgrad: 2048-row chunks), and one that does not depend on how
    torch's CPU kernel splits the batch over its threads."""
    nb = B if not chunk_rows else max(1, chunk_rows // (H * W))

    def conv(z, w, pad):
        if nb >= B:
            return Fn.conv2d(z, w, padding=pad)
        return torch.cat([Fn.conv2d(z[i:i + nb], w, padding=pad) for i in range(0, B, nb)])

    P = [torch.tensor(np.asarray(p, dtype=dtype).ravel(), requires_grad=want_grad) for p in params]
    it = iter(range(len(P)))
    pre = []

    def conv_bn_relu(z, cin, cout, k):
        w = P[next(it)].reshape(cout, cin, k, k)
        g = P[next(it)].reshape(B, cout, H, W)
        b = P[next(it)].reshape(B, cout, H, W)
        y = conv(z, w, k // 2)
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        a = (y - mean) / torch.sqrt(var + eps) * g + b
        if want_pre:
            pre.append(a.detach().numpy())
        return torch.relu(a)

    z = torch.tensor(np.asarray(x, dtype=dtype).reshape(B, F, H, W))
    z = conv_bn_relu(z, F, K, 3)
    for _ in range(L):
        a = conv_bn_relu(z, K, K, 3)
        b = conv_bn_relu(z, K, K, 3)
        z = torch.relu(a + b)
    p = conv_bn_relu(z, K, 2, 1).reshape(B, 2 * H * W)
    logits = p @ P[next(it)].reshape(2 * H * W, A) + P[next(it)].reshape(B, A)
    vv = conv_bn_relu(z, K, 1, 1).reshape(B, H * W)
    hpre = vv @ P[next(it)].reshape(H * W, FC) + P[next(it)].reshape(B, FC)
    if want_pre == "all":
        pre.append(hpre.detach().numpy())
    hid = torch.relu(hpre)
    o = (hid @ P[next(it)].reshape(FC, 1) + P[next(it)].reshape(B, 1)).reshape(B)
    assert next(it, None) is None, "parameter list longer than the network"
    Pi = torch.tensor(np.asarray(pi, dtype=dtype).reshape(B, A))
    V = torch.tensor(np.asarray(v, dtype=dtype).reshape(B))
    cost = -(Pi * logits + (1 - Pi) * (1 - logits)).mean() + ((o - V) ** 2).mean()
    grads = None
    if want_grad:
        cost.backward()
        grads = [q.grad.numpy().ravel().astype(np.float64) for q in P]
    return (cost.item(), grads, pre) if want_pre else (cost.item(), grads)


def f64_train_of(t, x, pi, v, K, L, FC, W, H, F, A, B, **kw):
    """f64_train on the current parameters of an oracle_lib.TrainNet"""
    return f64_train([t.get_param(i) for i in range(t.num_params())], x, pi, v, K, L, FC, W, H, F, A, B, **kw)


def relu_margin(pre, tau):
    """(smallest |pre-activation| over every ReLU unit, units with |pre| < tau, all units) of a want_pre="all" list"""
    return (min(float(np.abs(a).min()) for a in pre), sum(int((np.abs(a) < tau).sum()) for a in pre), sum(a.size for a in pre))


def condition(params, x, pi, v, K, L, FC, W, H, F, A, B, tau, eps=1e-5, max_rounds=8):
    """Make a draw well-posed for an fp32 evaluation: no ReLU unit within tau of its kink.

    The untied trainer's beta is batch-shaped [B][C][H][W] — every ReLU unit behind a BatchNorm has a beta of its own, and every unit of the
    value head's hidden layer a bias of its own (b1 [B][FC]).  One round walks the float64 forward in evaluation order; at each BatchNorm, and
    at the hidden layer, it moves the beta (bias) of every unit with |pre| < tau so that pre = +-2 tau with the sign kept (+ for an exact
    zero), rounds the moved values to float32 and goes on with them — a later layer never disturbs an earlier one.  Rounds repeat until a
    float64 forward on the rounded parameters has min |pre| >= tau (the rounding of a moved beta, half an ulp of it, is far below tau; one
    round is the rule, the loop is the proof).  The loss is then smooth on a ball that contains every evaluation whose pre-activations are
    within tau of float64's.

    Returns (params', moved, units, min|pre64|): the parameters as float32 arrays (only betas / b1 differ from the input, which is taken as
    float32), the number of units moved over all rounds, the number of ReLU units, the margin reached."""
    P = [np.asarray(p, dtype=np.float32).ravel().copy() for p in params]
    moved = 0
    for _ in range(max_rounds):
        T = [torch.tensor(p.astype(np.float64)) for p in P]
        it = iter(range(len(T)))
        n_moved = 0

        def fix(a, i_beta):
            """a: the float64 pre-activation computed with the current beta / bias T[i_beta]; returns it after the move"""
            nonlocal n_moved
            near = a.abs() < tau
            k = int(near.sum())
            if not k:
                return a
            n_moved += k
            sign = torch.where(a < 0, -1.0, 1.0).to(a.dtype)
            b = T[i_beta].reshape(a.shape)
            b_new = torch.where(near, b + (2 * tau * sign - a), b)
            b32 = b_new.numpy().astype(np.float32)
            P[i_beta] = b32.ravel()
            return a - b + torch.tensor(b32.astype(np.float64))

        def conv_bn_relu(z, cin, cout, k):
            w = T[next(it)].reshape(cout, cin, k, k)
            g = T[next(it)].reshape(B, cout, H, W)
            ib = next(it)
            y = Fn.conv2d(z, w, padding=k // 2)
            mean = y.mean(dim=(0, 2, 3), keepdim=True)
            var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
            a = (y - mean) / torch.sqrt(var + eps) * g + T[ib].reshape(B, cout, H, W)
            return torch.relu(fix(a, ib))

        with torch.no_grad():
            z = torch.tensor(np.asarray(x, dtype=np.float64).reshape(B, F, H, W))
            z = conv_bn_relu(z, F, K, 3)
            for _l in range(L):
                a = conv_bn_relu(z, K, K, 3)
                b = conv_bn_relu(z, K, K, 3)
                z = torch.relu(a + b)     # (a, b >= 0: no kink of its own)
            conv_bn_relu(z, K, 2, 1)
            next(it), next(it)            # policy FC: no ReLU behind it
            vv = conv_bn_relu(z, K, 1, 1).reshape(B, H * W)
            w1 = T[next(it)].reshape(H * W, FC)
            ib = next(it)
            fix(vv @ w1 + T[ib].reshape(B, FC), ib)
        moved += n_moved
        _, _, pre = f64_train(P, x, pi, v, K, L, FC, W, H, F, A, B, eps=eps, want_pre="all", want_grad=False)
        lo, near, units = relu_margin(pre, tau)
        if near == 0:
            return P, moved, units, lo
    raise AssertionError("condition: %d units still within tau = %g after %d rounds" % (near, tau, max_rounds))


def measured_tau(params, x, pi, v, K, L, FC, W, H, F, A, B, pre64=None):
    """tau of a draw, measured and not fixed: the largest |pre32 - pre64| over every ReLU unit, pre32 the same forward in float32 torch on
    the UNCONDITIONED draw, times 16 — the split-product modes are allowed 8 times the fp32 model (agz.h; tests/test_tower_f64_gpu.py), times
    2 for headroom — rounded up to a power of two.  Returns (tau, the largest |pre32 - pre64|)."""
    if pre64 is None:
        _, _, pre64 = f64_train(params, x, pi, v, K, L, FC, W, H, F, A, B, want_pre="all", want_grad=False)
    _, _, pre32 = f64_train(params, x, pi, v, K, L, FC, W, H, F, A, B, want_pre="all", want_grad=False, dtype=np.float32)
    d = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pre32, pre64))
    return float(2.0 ** np.ceil(np.log2(16 * d))), d
