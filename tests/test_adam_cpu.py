"""CPU: the Adam ABI (agz_trainer_set_adam and its companions) — declared in include/agz.h, exported by libagz.so, bound in
agogo_amd/capi.py with the struct the header states, and called by the Go shim with the declared argument counts — and the float32 numpy
restatement of the declared definition (adam_step below, which the GPU tests compare the device against), itself checked against a
float64 Adam.  None of this needs a device: the NULL-trainer call returns before anything touches HIP."""
import ctypes as C
import os
import re

import numpy as np

import test_go_shim_signatures_cpu as shim_sigs
from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"agz_trainer_set_adam": 2, "agz_trainer_get_adam": 3, "agz_trainer_get_moments": 5, "agz_trainer_set_moments": 5}


def adam_consts(b1, b2, t):
    """what the host passes to the kernels at step t: beta, 1 - beta rounded to float, 1 / (1 - beta^t) in double rounded once"""
    f = np.float32
    b1d, b2d = float(f(b1)), float(f(b2))
    return f(b1), f(1.0 - b1d), f(b2), f(1.0 - b2d), f(1.0 / (1.0 - b1d ** t)), f(1.0 / (1.0 - b2d ** t))


def adam_step(w, m, v, g, lr, gs, l2, c, b1, b2, eps, t):
    """the declared definition (include/agz.h, DESIGN §2 `solver-adam`) restated in float32 numpy, one operation per rounding;
    returns w', m', v', g3 and the increment added to w"""
    f = np.float32
    fb1, omb1, fb2, omb2, rc1, rc2 = adam_consts(b1, b2, t)
    g = f(gs) * g
    if l2 != 0:
        g = g + f(l2) * w
    if c > 0:
        g = np.minimum(np.maximum(g, f(-c)), f(c))
    m = fb1 * m + omb1 * g
    v = fb2 * v + omb2 * (g * g)
    inc = f(-lr) * ((m * rc1) / (np.sqrt(v * rc2) + f(eps)))
    w = w + inc
    for a in (w, m, v, g, inc):
        assert a.dtype == np.float32
    return w, m, v, g, inc


def test_the_four_functions_are_declared_exported_and_bound():
    protos = shim_sigs._c_prototypes()
    lib = capi.lib()
    for name, nargs in FUNCS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        fn = getattr(lib, name)                      # AttributeError if libagz.so does not export it
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    for method in ("set_adam", "get_adam", "get_moments", "set_moments"):
        assert callable(getattr(capi.Trainer, method)), method


def test_adam_conf_is_the_16_byte_struct_of_the_header():
    assert C.sizeof(capi.AdamConf) == 16
    assert [(n, t) for n, t in capi.AdamConf._fields_] == [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("on", C.c_int32)]
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    m = re.search(r"typedef struct agz_adam_conf \{([^}]*)\} agz_adam_conf;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "float beta1, beta2, eps; int32_t on;", m and m.group(1)


def test_the_go_shim_calls_each_function_with_the_declared_argument_count():
    calls = shim_sigs._go_calls(open(shim_sigs.SHIM).read())
    seen = {}
    for name, n, line in calls:
        if name in FUNCS:
            assert n == FUNCS[name], "agzhip.go:%d: C.%s called with %d argument(s), the prototype has %d" % (line, name, n, FUNCS[name])
            seen[name] = seen.get(name, 0) + 1
    assert set(seen) == set(FUNCS), "the Go shim does not call %s" % sorted(set(FUNCS) - set(seen))
    got = shim_sigs.methods(open(shim_sigs.SHIM).read(), ("*Trainer",))
    assert got["SetAdam"] == (["AdamConf"], ["error"]) and got["Adam"] == ([], ["AdamConf", "uint64", "error"])
    assert got["Moments"] == (["int", "[]float32", "[]float32"], ["error"])
    assert got["SetMoments"] == (["int", "[]float32", "[]float32"], ["error"])


def test_calls_on_a_null_trainer_return_an_error_code():
    lib = capi.lib()
    ac = capi.AdamConf(0.9, 0.999, 1e-8, 1)
    step = C.c_uint64(0)
    m, v = (C.c_float * 4)(), (C.c_float * 4)()
    for rc in (lib.agz_trainer_set_adam(None, C.byref(ac)), lib.agz_trainer_get_adam(None, C.byref(ac), C.byref(step)),
               lib.agz_trainer_get_moments(None, 0, m, v, 4), lib.agz_trainer_set_moments(None, 0, m, v, 4)):
        assert rc == -1                              # AGZ_E_INVALID, and no crash
        assert b"NULL" in lib.agz_last_error()


def test_the_float32_restatement_follows_a_float64_adam():
    """50 steps of random gradients (fixed mean + noise, so that the moments neither vanish nor cancel), with L2 and a clamp that bites:
    the float32 restatement stays within 1e-5 relative of textbook Adam carried in float64 (the same float32 settings promoted)."""
    rng = np.random.default_rng(0)
    n, lr, l2, clip, b1, b2, eps = 4096, 0.01, 1e-4, 1.5, 0.9, 0.999, 1e-8
    mean = rng.normal(0, 1, n)
    w32 = rng.normal(0, 1, n).astype(np.float32)
    m32, v32 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    w64, m64, v64 = w32.astype(np.float64), np.zeros(n), np.zeros(n)
    f = lambda x: float(np.float32(x))
    clamped = 0
    for t in range(1, 51):
        g = (mean + rng.normal(0, 0.3, n)).astype(np.float32)
        w32, m32, v32, g3, _ = adam_step(w32, m32, v32, g, lr, 1.0, l2, clip, b1, b2, eps, t)
        clamped += int((np.abs(g3) == np.float32(clip)).sum())
        g64 = np.clip(g.astype(np.float64) + f(l2) * w64, -f(clip), f(clip))
        m64 = f(b1) * m64 + (1 - f(b1)) * g64
        v64 = f(b2) * v64 + (1 - f(b2)) * g64 * g64
        w64 = w64 - f(lr) * (m64 / (1 - f(b1) ** t)) / (np.sqrt(v64 / (1 - f(b2) ** t)) + f(eps))
    assert clamped > 0
    for a32, a64 in ((w32, w64), (m32, m64), (v32, v64)):
        rel = float(np.abs(a32 - a64).max() / np.abs(a64).max())
        assert rel <= 1e-5, rel
