"""CPU: the ABI of the loss kind (agz_trainer_set_loss, agz_trainer_get_loss, agz_trainer_get_costs) — declared in include/agz.h, exported
by libagz.so, bound in agogo_amd/capi.py, called by the Go shim with the declared argument counts — and the float64 reference of the
AlphaZero loss (tests/f64_train_az.py) checked against the closed forms of the definition.  None of this needs a device: the NULL-trainer
call returns before anything touches HIP."""
import ctypes as C
import os

import numpy as np

import test_go_shim_signatures_cpu as shim_sigs
from agogo_amd import capi
from f64_train_az import closed_forms, draw_batch, draw_params, f64_train_az, param_shapes

FUNCS = {"agz_trainer_set_loss": 2, "agz_trainer_get_loss": 2, "agz_trainer_get_costs": 3}
TWO_PASS = (32, 1, 16, 3, 3, 2, 10, 4)


def test_the_three_functions_are_declared_exported_and_bound():
    protos = shim_sigs._c_prototypes()
    lib = capi.lib()
    for name, nargs in FUNCS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        fn = getattr(lib, name)                      # AttributeError if libagz.so does not export it
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    hdr = open(os.path.join(shim_sigs.ROOT, "include", "agz.h")).read()
    assert "#define AGZ_LOSS_REFERENCE 0" in hdr and "#define AGZ_LOSS_ALPHAZERO 1" in hdr
    assert (capi.LOSS_REFERENCE, capi.LOSS_ALPHAZERO) == (0, 1)
    for method in ("set_loss", "get_loss", "costs"):
        assert callable(getattr(capi.Trainer, method)), method


def test_the_go_shim_calls_each_function_with_the_declared_argument_count():
    src = open(shim_sigs.SHIM).read()
    seen = {}
    for name, n, line in shim_sigs._go_calls(src):
        if name in FUNCS:
            assert n == FUNCS[name], "agzhip.go:%d: C.%s called with %d argument(s), the prototype has %d" % (line, name, n, FUNCS[name])
            seen[name] = seen.get(name, 0) + 1
    assert set(seen) == set(FUNCS), "the Go shim does not call %s" % sorted(set(FUNCS) - set(seen))
    got = shim_sigs.methods(src, ("*Trainer",))
    assert got["SetLoss"] == (["int"], ["error"]) and got["Loss"] == ([], ["int", "error"])
    assert got["Costs"] == ([], ["float32", "float32", "error"])


def test_calls_on_a_null_trainer_return_an_error_code():
    lib = capi.lib()
    kind, p, v = C.c_int(7), C.c_float(3), C.c_float(4)
    assert lib.agz_trainer_set_loss(None, capi.LOSS_ALPHAZERO) == -1          # AGZ_E_INVALID, and no crash
    assert lib.agz_trainer_get_loss(None, C.byref(kind)) == -1 and kind.value == 7
    assert lib.agz_trainer_get_costs(None, C.byref(p), C.byref(v)) == -1 and (p.value, v.value) == (3.0, 4.0)
    assert b"NULL" in lib.agz_last_error()


def test_the_float64_module_agrees_with_the_closed_forms():
    """autograd's d cost / d logits and d cost / d o (retained) against dz = (S p - Pi) / Bn, do = 2 (t - V)(1 - t^2) / Bn to 1e-12, on
    softmax rows, one-hot rows and with one row of Pi scaled by 0.5 (S_b != 1); the cost against its own restatement in numpy; the tied
    module against the untied one holding the tied tensor in every row"""
    case = TWO_PASS
    K, L, FC, W, H, F, A, B = case
    P = draw_params(case, seed=1)
    assert [p.size for p in P] == [int(np.prod(s)) for _, s in param_shapes(case)]
    for kind in ("softmax", "onehot", "half_row"):
        x, pi, v = draw_batch(case, seed=1001, pi_kind=kind)
        assert abs(float(pi[0].sum()) - (0.5 if kind == "half_row" else 1.0)) < 1e-6 and abs(float(pi[1].sum()) - 1.0) < 1e-6
        out = {}
        cost, grads = f64_train_az(P, x, pi, v, *case, out=out)
        dz, do = closed_forms(out["logits"], out["o"], pi, v, B)
        assert np.abs(out["dlogits"] - dz).max() <= 1e-12 and np.abs(out["do"] - do).max() <= 1e-12, kind
        assert np.abs(dz).max() > 1e-3 and np.abs(do).max() > 1e-3
        z, Pi = out["logits"], pi.astype(np.float64)
        logp = z - z.max(axis=1, keepdims=True)
        logp = logp - np.log(np.exp(logp).sum(axis=1, keepdims=True))
        # -sum Pi log softmax(z) over a row, written with S_b: Pi log p = Pi z - Pi lse
        want_p = float(-(Pi * logp).sum(axis=1).mean())
        want_v = float(((np.tanh(out["o"]) - v.astype(np.float64)) ** 2).mean())
        assert abs(out["pcost"] - want_p) <= 1e-12 and abs(out["vcost"] - want_v) <= 1e-12 and abs(cost - want_p - want_v) <= 1e-12
        # the biases' gradients are dz / do themselves
        names = [nm for nm, _ in param_shapes(case)]
        assert np.abs(grads[names.index("Policy_b")] - dz.ravel()).max() <= 1e-12
        assert np.abs(grads[names.index("ValueOutput_b")] - do).max() <= 1e-12


def test_the_tied_module_is_the_untied_one_with_the_tensor_in_every_row():
    case = TWO_PASS
    K, L, FC, W, H, F, A, B = case
    PT = draw_params(case, seed=3, tied=True)
    shapes = param_shapes(case, tied=True)
    batch_shaped = [nm.endswith(("_gamma", "_beta", "_b")) for nm, _ in shapes]
    PU = [np.tile(p, B) if bs else p for p, bs in zip(PT, batch_shaped)]
    x, pi, v = draw_batch(case, seed=1003)
    ct, GT = f64_train_az(PT, x, pi, v, *case, tied=True)
    cu, GU = f64_train_az(PU, x, pi, v, *case)
    assert abs(ct - cu) <= 1e-12
    for gt, gu, bs in zip(GT, GU, batch_shaped):
        want = gu.reshape(B, -1).sum(axis=0) if bs else gu
        assert np.abs(gt - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))
