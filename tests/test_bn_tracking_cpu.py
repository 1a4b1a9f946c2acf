"""CPU: the ABI of the running BatchNorm statistics (agz_trainer_set_bn_tracking and its companions, agz_trainer_eval) — declared in
include/agz.h, exported by libagz.so, bound in agogo_amd/capi.py, and called by the Go shim with the declared argument counts.  None of
this needs a device: the NULL-trainer call returns before anything touches HIP."""
import ctypes as C

import test_go_shim_signatures_cpu as shim_sigs
from agogo_amd import capi

FUNCS = {"agz_trainer_set_bn_tracking": 3, "agz_trainer_get_bn_tracking": 4, "agz_trainer_num_bn": 1, "agz_trainer_get_bn_stats": 5,
         "agz_trainer_set_bn_stats": 6, "agz_trainer_reset_bn_stats": 1, "agz_trainer_eval": 5, "agz_trainer_eval_dev": 5}


def test_the_eight_functions_are_declared_exported_and_bound():
    protos = shim_sigs._c_prototypes()
    lib = capi.lib()
    for name, nargs in FUNCS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        fn = getattr(lib, name)                      # AttributeError if libagz.so does not export it
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    assert lib.agz_trainer_set_bn_stats.argtypes[-1] is C.c_double and lib.agz_trainer_set_bn_tracking.argtypes[-1] is C.c_float
    for method in ("set_bn_tracking", "get_bn_tracking", "num_bn", "get_bn_stats", "set_bn_stats", "reset_bn_stats", "eval"):
        assert callable(getattr(capi.Trainer, method)), method


def test_the_go_shim_calls_each_function_with_the_declared_argument_count():
    calls = shim_sigs._go_calls(open(shim_sigs.SHIM).read())
    seen = {}
    for name, n, line in calls:
        if name in FUNCS:
            assert n == FUNCS[name], "agzhip.go:%d: C.%s called with %d argument(s), the prototype has %d" % (line, name, n, FUNCS[name])
            seen[name] = seen.get(name, 0) + 1
    assert set(seen) == set(FUNCS), "the Go shim does not call %s" % sorted(set(FUNCS) - set(seen))
    got = shim_sigs.methods(open(shim_sigs.SHIM).read(), ("*Trainer",))
    assert got["SetBNTracking"] == (["bool", "float32"], ["error"]) and got["BNTracking"] == ([], ["bool", "float32", "float64", "error"])
    assert got["NumBN"] == ([], ["int"]) and got["ResetBNStats"] == ([], ["error"])
    assert got["BNStats"] == (["int", "[]float32", "[]float32"], ["error"])
    assert got["SetBNStats"] == (["int", "[]float32", "[]float32", "float64"], ["error"])
    assert got["Eval"] == (["[]float32", "[]float32", "[]float32"], ["float32", "error"])


def test_calls_on_a_null_trainer_return_an_error_code():
    lib = capi.lib()
    buf = (C.c_float * 4)()
    on, m, w = C.c_int(0), C.c_float(0), C.c_double(0)
    assert lib.agz_trainer_set_bn_tracking(None, 1, 0.997) == -1          # AGZ_E_INVALID, and no crash
    assert lib.agz_trainer_get_bn_tracking(None, C.byref(on), C.byref(m), C.byref(w)) == -1
    assert lib.agz_trainer_num_bn(None) == 0
    assert lib.agz_trainer_get_bn_stats(None, 0, buf, buf, 4) == -1
    assert lib.agz_trainer_set_bn_stats(None, 0, buf, buf, 4, 1.0) == -1
    assert lib.agz_trainer_reset_bn_stats(None) == -1
    assert lib.agz_trainer_eval(None, buf, buf, buf, buf) == -1
    assert lib.agz_trainer_eval_dev(None, None, None, None, buf) == -1
    assert b"NULL" in lib.agz_last_error() or b"bad argument" in lib.agz_last_error()
