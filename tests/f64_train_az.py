"""The training network under the AlphaZero loss (agz_trainer_set_loss(AGZ_LOSS_ALPHAZERO); include/agz.h, DESIGN §2 `az-loss`) restated in
float64 torch autograd — the reference of tests/test_az_loss_*.py.  The network is tests/f64_train.py's, line for line; the cost is

    pcost = (1/Bn) sum_b ( S_b lse_b - sum_j Pi_bj z_bj )      S_b = sum_j Pi_bj,  lse_b = logsumexp_j z_bj
    vcost = (1/Bn) sum_b (tanh(o_b) - V_b)^2                    cost = pcost + vcost

with `tied` (gamma / beta / biases at their row-0 shape, broadcast over the rows: agz_trainer_create_tied), `want_pre` as in f64_train, and
`stats` (a list of (mean, var) per BatchNorm op: the eval pass under running statistics).  Also the draws the tests share — parameters by
name and shape from the topology alone, batches whose Pi rows are a softmax of random logits — and the ReLU margin of a draw, so that
seeds can be chosen without a device.  A plain module: no fixtures, no GPU."""
import numpy as np
import torch
import torch.nn.functional as Fn


def f64_train_az(params, x, pi, v, K, L, FC, W, H, F, A, B, eps=1e-5, want_pre=False, tied=False, stats=None, out=None):
    """params in the trainer's parameter order; x [B][F][H][W], pi [B][A], v [B].  Returns (cost, grads) or, with want_pre, (cost, grads,
    pre): pre[k] the pre-activation of the k-th BatchNorm in evaluation order, then the value head's hidden layer before its ReLU.
    `out`, a dict, receives pcost, vcost, logits, o and the autograd gradients dlogits, do."""
    P = [torch.tensor(np.asarray(p, dtype=np.float64).ravel(), requires_grad=True) for p in params]
    it = iter(range(len(P)))
    pre = []
    R = 1 if tied else B
    n_bn = [0]

    def conv_bn_relu(z, cin, cout, k):
        w = P[next(it)].reshape(cout, cin, k, k)
        g = P[next(it)].reshape(R, cout, H, W)
        b = P[next(it)].reshape(R, cout, H, W)
        y = Fn.conv2d(z, w, padding=k // 2)
        if stats is None:
            mean = y.mean(dim=(0, 2, 3), keepdim=True)
            var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        else:
            m, s = stats[n_bn[0]]
            mean = torch.tensor(np.asarray(m, np.float64)).reshape(1, cout, 1, 1)
            var = torch.tensor(np.asarray(s, np.float64)).reshape(1, cout, 1, 1)
        n_bn[0] += 1
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
    logits = p @ P[next(it)].reshape(2 * H * W, A) + P[next(it)].reshape(R, A)
    vv = conv_bn_relu(z, K, 1, 1).reshape(B, H * W)
    hpre = vv @ P[next(it)].reshape(H * W, FC) + P[next(it)].reshape(R, FC)
    if want_pre:
        pre.append(hpre.detach().numpy())
    hid = torch.relu(hpre)
    o = (hid @ P[next(it)].reshape(FC, 1) + P[next(it)].reshape(R, 1)).reshape(B)
    assert next(it, None) is None, "parameter list longer than the network"
    logits.retain_grad()
    o.retain_grad()
    Pi = torch.tensor(np.asarray(pi, dtype=np.float64).reshape(B, A))
    V = torch.tensor(np.asarray(v, dtype=np.float64).reshape(B))
    pcost = (Pi.sum(dim=1) * torch.logsumexp(logits, dim=1) - (Pi * logits).sum(dim=1)).mean()
    vcost = ((torch.tanh(o) - V) ** 2).mean()
    cost = pcost + vcost
    cost.backward()
    grads = [q.grad.numpy().ravel() for q in P]
    if out is not None:
        out.update(pcost=pcost.item(), vcost=vcost.item(), logits=logits.detach().numpy(), o=o.detach().numpy(),
                   dlogits=logits.grad.numpy(), do=o.grad.numpy())
    return (cost.item(), grads, pre) if want_pre else (cost.item(), grads)


def closed_forms(logits, o, pi, v, Bn):
    """dz, do of the definition, in float64 numpy"""
    z = np.asarray(logits, np.float64)
    Pi, V = np.asarray(pi, np.float64), np.asarray(v, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    t = np.tanh(np.asarray(o, np.float64))
    return (Pi.sum(axis=1, keepdims=True) * p - Pi) / Bn, 2 * (t - V) * (1 - t * t) / Bn


def param_shapes(case, tied=False):
    """(name, shape) of every learnable in the trainer's order (agz_trainer_param_info)"""
    K, L, FC, W, H, F, A, B = case
    R = 1 if tied else B
    out = [("FilterInit", (K, F, 3, 3)), ("Init_gamma", (R, K, H, W)), ("Init_beta", (R, K, H, W))]
    for i in range(L):
        for br in (1, 2):
            out += [("FilterLayer%d of Shared Layer %d" % (br, i), (K, K, 3, 3)), ("L%d_%d_gamma" % (br, i), (R, K, H, W)),
                    ("L%d_%d_beta" % (br, i), (R, K, H, W))]
    out += [("FilterPolicyHead", (2, K, 1, 1)), ("PolicyHead_gamma", (R, 2, H, W)), ("PolicyHead_beta", (R, 2, H, W)),
            ("Policy_w", (2 * H * W, A)), ("Policy_b", (R, A)),
            ("FilterValueHead", (1, K, 1, 1)), ("ValueHead_gamma", (R, 1, H, W)), ("ValueHead_beta", (R, 1, H, W)),
            ("Value_w", (H * W, FC)), ("Value_b", (R, FC)), ("ValueOutput_w", (FC, 1)), ("ValueOutput_b", (R, 1))]
    return out


def draw_params(case, seed, tied=False):
    """float32 learnables: filters and FC weights normal with the fan-in's scale, gamma uniform in [0.5, 1.5], beta and biases N(0, 0.1)"""
    rng = np.random.default_rng(seed)
    P = []
    for nm, shp in param_shapes(case, tied):
        n = int(np.prod(shp))
        if nm.endswith("_gamma"):
            p = rng.uniform(0.5, 1.5, n)
        elif nm.endswith(("_beta", "_b")):
            p = rng.normal(0, 0.1, n)
        else:
            fan_in = int(np.prod(shp[1:])) if len(shp) == 4 else shp[0]
            p = rng.normal(0, 1.0 / np.sqrt(fan_in), n)
        P.append(p.astype(np.float32))
    return P


def draw_batch(case, seed, pi_kind="softmax"):
    """x of {-1, 0, 1, 0.001}; Pi rows a softmax of random logits (or one-hot rows; or the softmax rows with row 0 scaled by 0.5); V in
    [-1, 1]"""
    K, L, FC, W, H, F, A, B = case
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, 0.0, 1.0, 0.001], np.float32), size=(B, F, H, W)).astype(np.float32)
    z = rng.normal(0, 2.0, (B, A))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    pi = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    v = rng.uniform(-1, 1, B).astype(np.float32)
    if pi_kind == "onehot":
        pi = np.zeros((B, A), np.float32)
        pi[np.arange(B), rng.integers(0, A, B)] = 1.0
    elif pi_kind == "half_row":
        pi[0] *= np.float32(0.5)
    else:
        assert pi_kind == "softmax", pi_kind
    return x, pi, v


def relu_margin(pre):
    """the smallest |pre-activation| of any ReLU argument as a fraction of its layer's rms"""
    return min(float(np.abs(a).min() / np.sqrt((a * a).mean())) for a in pre)
