"""CPU: the solver-option ABI (agz_trainer_set_solver and its companions) — declared in include/agz.h, exported by libagz.so, bound in
agogo_amd/capi.py with the struct the header states, and called by the Go shim with the declared argument counts.  None of this needs
a device: the NULL-trainer call returns before anything touches HIP."""
import ctypes as C
import os
import re

import test_go_shim_signatures_cpu as shim_sigs
from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"agz_trainer_set_solver": 2, "agz_trainer_get_solver": 2, "agz_trainer_get_velocity": 4, "agz_trainer_set_velocity": 4,
         "agz_trainer_reset_solver": 1}


def test_the_five_functions_are_declared_exported_and_bound():
    protos = shim_sigs._c_prototypes()
    lib = capi.lib()
    for name, nargs in FUNCS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        fn = getattr(lib, name)                      # AttributeError if libagz.so does not export it
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    for method in ("set_solver", "get_solver", "get_velocity", "set_velocity", "reset_solver"):
        assert callable(getattr(capi.Trainer, method)), method


def test_solver_conf_is_the_16_byte_struct_of_the_header():
    assert C.sizeof(capi.SolverConf) == 16
    assert [(n, t) for n, t in capi.SolverConf._fields_] == [("momentum", C.c_float), ("l2reg", C.c_float), ("clip", C.c_float),
                                                            ("reserved", C.c_int32)]
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    m = re.search(r"typedef struct agz_solver_conf \{([^}]*)\} agz_solver_conf;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "float momentum, l2reg, clip; int32_t reserved;", m and m.group(1)


def test_the_go_shim_calls_each_function_with_the_declared_argument_count():
    calls = shim_sigs._go_calls(open(shim_sigs.SHIM).read())
    seen = {}
    for name, n, line in calls:
        if name in FUNCS:
            assert n == FUNCS[name], "agzhip.go:%d: C.%s called with %d argument(s), the prototype has %d" % (line, name, n, FUNCS[name])
            seen[name] = seen.get(name, 0) + 1
    assert set(seen) == set(FUNCS), "the Go shim does not call %s" % sorted(set(FUNCS) - set(seen))
    got = shim_sigs.methods(open(shim_sigs.SHIM).read(), ("*Trainer",))
    assert got["SetSolver"] == (["SolverConf"], ["error"]) and got["Solver"] == ([], ["SolverConf", "error"])
    assert got["Velocity"] == (["int", "[]float32"], ["error"]) and got["SetVelocity"] == (["int", "[]float32"], ["error"])
    assert got["ResetSolver"] == ([], ["error"])


def test_calls_on_a_null_trainer_return_an_error_code():
    lib = capi.lib()
    sc = capi.SolverConf(0.9, 1e-4, 0.0, 0)
    buf = (C.c_float * 4)()
    assert lib.agz_trainer_set_solver(None, C.byref(sc)) == -1          # AGZ_E_INVALID, and no crash
    assert lib.agz_trainer_get_solver(None, C.byref(sc)) == -1
    assert lib.agz_trainer_get_velocity(None, 0, buf, 4) == -1
    assert lib.agz_trainer_set_velocity(None, 0, buf, 4) == -1
    assert lib.agz_trainer_reset_solver(None) == -1
    assert b"NULL" in lib.agz_last_error()
