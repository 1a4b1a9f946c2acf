"""CPU: the tied-affine trainer's ABI (agz_trainer_create_tied, agz_trainer_is_tied) and the licence for its reference.

A tied trainer stores BatchNorm gamma / beta [C,H,W] and the FC biases [units] once, shared by every batch row (include/agz.h, DESIGN §2
`tied-affine`).  The oracle (oracle/train.hpp) only knows the batch-shaped form.  By the chain rule the gradient of a tied tensor is the
sum over the batch rows of the per-row gradients of the batch-shaped network that holds the tied tensor in every row: `oracle_tied` below
states that in numpy over the oracle, and the last test checks it against a float64 torch model that HAS tied tensors.  The GPU tests
(test_tied_gpu.py) then use `oracle_tied` as their reference."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as Fn

import oracle_lib as O
import test_go_shim_signatures_cpu as shim_sigs
from agogo_amd import capi

FUNCS = {"agz_trainer_create_tied": 3, "agz_trainer_is_tied": 2}
LICENCE_CASE = (32, 1, 16, 3, 3, 2, 10, 4)


def is_batch_shaped(name):
    return name.endswith(("_gamma", "_beta", "_b"))


def draw_tied(case, seed=5, wscale=3.0):
    """make_pair's draws (test_adam_gpu): the oracle's initialiser for filters and FC weights (times wscale), uniform gamma, normal beta /
    biases — then row 0 of every batch-shaped tensor.  Returns (names, tied parameters)"""
    K, L, FC, W, H, F, Aspace, B = case
    ot = O.TrainNet(K, L, FC, W, H, F, Aspace, B)
    ot.init_random(seed)
    rng = np.random.default_rng(seed)
    names, P = [], []
    for i in range(ot.num_params()):
        nm = ot.param_name(i)
        p = ot.get_param(i)
        if nm.endswith("_gamma"):
            p = rng.uniform(0.5, 1.5, p.size).astype(np.float32)
        elif nm.endswith("_beta") or nm.endswith("_b"):
            p = rng.normal(0, 0.1, p.size).astype(np.float32)
        else:
            p = (p * wscale).astype(np.float32)
        names.append(nm)
        P.append(p[:p.size // B].copy() if is_batch_shaped(nm) else p)
    return names, P


def oracle_tied(case, names, P, x, pi, v):
    """the declared definition over the oracle: every row of a batch-shaped tensor = the tied tensor, batch(lr = 0), the per-row gradients
    summed over the row axis in float64.  Returns (cost, gradients as float64, tied shapes)"""
    K, L, FC, W, H, F, Aspace, B = case
    ot = O.TrainNet(K, L, FC, W, H, F, Aspace, B)
    for i, (nm, p) in enumerate(zip(names, P)):
        ot.set_param(i, np.tile(p, B) if is_batch_shaped(nm) else p)
    cost = ot.batch(x, pi, v, lr=0.0)
    G = []
    for i, nm in enumerate(names):
        g = ot.get_grad(i).astype(np.float64)
        G.append(g.reshape(B, -1).sum(axis=0) if is_batch_shaped(nm) else g)
    return cost, G


def torch_tied(case, P, x, pi, v, eps=1e-5):
    """float64 torch model with tied tensors: per-element gamma / beta [C,H,W] broadcast over the batch, training-mode BatchNorm (biased
    variance), biases [units], the reference's loss (linear 'xent' on the logits + MSE on the pre-tanh value).  Returns (cost, gradients)"""
    K, L, FC, W, H, F, Aspace, B = case
    T = [torch.tensor(np.asarray(p, np.float64), requires_grad=True) for p in P]
    it = iter(T)

    def conv_bn_relu(z, cin, cout, k):
        w = next(it).reshape(cout, cin, k, k)
        g = next(it).reshape(1, cout, H, W)
        b = next(it).reshape(1, cout, H, W)
        y = Fn.conv2d(z, w, padding=k // 2)
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        return torch.relu((y - mean) / torch.sqrt(var + eps) * g + b)

    z = conv_bn_relu(torch.tensor(x.astype(np.float64)), F, K, 3)
    for _ in range(L):
        a = conv_bn_relu(z, K, K, 3)
        b = conv_bn_relu(z, K, K, 3)
        z = torch.relu(a + b)
    p = conv_bn_relu(z, K, 2, 1).reshape(B, 2 * H * W)
    logits = p @ next(it).reshape(2 * H * W, Aspace) + next(it).reshape(1, Aspace)
    vv = conv_bn_relu(z, K, 1, 1).reshape(B, H * W)
    hid = torch.relu(vv @ next(it).reshape(H * W, FC) + next(it).reshape(1, FC))
    o = (hid @ next(it).reshape(FC, 1) + next(it).reshape(1, 1)).reshape(B)
    Pi, V = torch.tensor(pi.astype(np.float64)), torch.tensor(v.astype(np.float64))
    cost = -(Pi * logits + (1 - Pi) * (1 - logits)).mean() + ((o - V) ** 2).mean()
    cost.backward()
    return float(cost.detach()), [t.grad.numpy().reshape(-1) for t in T]


def batch_data(B, F, H, W, Aspace, seed):
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, 0.0, 1.0, 0.001], np.float32), size=(B, F, H, W)).astype(np.float32)
    pi = np.zeros((B, Aspace), np.float32)
    pi[np.arange(B), rng.integers(0, Aspace, B)] = 1.0
    v = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=B).astype(np.float32)
    return x, pi, v


def test_the_two_functions_are_declared_exported_and_bound():
    protos = shim_sigs._c_prototypes()
    lib = capi.lib()
    for name, nargs in FUNCS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        fn = getattr(lib, name)                      # AttributeError if libagz.so does not export it
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    assert callable(capi.Trainer.is_tied)
    calls = {name for name, _, _ in shim_sigs._go_calls(open(shim_sigs.SHIM).read())}
    assert set(FUNCS) <= calls, "the Go shim does not call %s" % sorted(set(FUNCS) - calls)


def test_create_tied_without_a_context_fails_loudly():
    lib = capi.lib()
    conf = capi.NetConf(32, 1, 16, 4, 3, 3, 2, 10, 0, 1e-5)
    h = C.c_void_p()
    assert lib.agz_trainer_create_tied(None, C.byref(conf), C.byref(h)) == -1      # AGZ_E_INVALID: no context, no trainer, no fallback
    assert not h.value and b"NULL" in lib.agz_last_error()
    tied = C.c_int(7)
    assert lib.agz_trainer_is_tied(None, C.byref(tied)) == -1 and tied.value == 7


def test_summing_the_oracles_row_gradients_is_the_gradient_of_a_tied_model():
    """the oracle is float32: its bar against float64 torch is test_oracle_torch_xcheck's, 2e-5 of the tensor's largest gradient"""
    case = LICENCE_CASE
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B)
    cost_o, G = oracle_tied(case, names, P, x, pi, v)
    cost_t, T = torch_tied(case, P, x, pi, v)
    assert abs(cost_o - cost_t) < 1e-5 * max(1.0, abs(cost_t)), (cost_o, cost_t)
    worst = 0.0
    for nm, g, t in zip(names, G, T):
        assert g.shape == t.shape, (nm, g.shape, t.shape)
        scale = max(float(np.abs(t).max()), 1e-8)
        err = float(np.abs(g - t).max())
        worst = max(worst, err / (2e-5 * scale + 1e-9))
        assert err <= 2e-5 * scale + 1e-9, (nm, err, scale)
    assert any(np.abs(t).max() > 1e-6 for nm, t in zip(names, T) if is_batch_shaped(nm))
    print("row-summed oracle against the float64 tied model: worst tensor %.3f of the bar" % worst)
