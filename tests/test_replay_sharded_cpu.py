"""CPU: the ABI of the sharded replay route and the window digest (agogo_amd/csrc/replay.hpp; DESIGN §2 `replay-sharded`).

The five calls — agz_replay_sample_slice_dev, agz_replay_sample_slice, agz_replay_digest, agz_replay_digest_host, agz_train_replay_sharded —
are declared in include/agz.h with the documented parameters, exported by libagz.so and bound in agogo_amd/capi.py.  The digest has one
host/device definition in replay.hpp, which includes nothing from HIP: tests/cpp/replay_digest_check.cpp runs it under g++ -Wall -Werror
and prints the digest of fixed row sets, recomputed here with Python integers from the declared definition

    mix64(z)       the SplitMix64 finaliser
    rowlen         F * cells + PolicyLen + 1; bits(j, e) the 32-bit pattern of element e (planes, policy, value) of logical row j
    digest       = n + sum over j < n, e < rowlen of mix64(mix64(j * rowlen + e) ^ bits(j, e))          (mod 2^64)

and agz_replay_digest_host (no context) must equal it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
INVALID = -1
NS, XS, AS = (0, 1, 5), (1, 18, 25), (1, 10)
NEG_ZERO, NAN_PATTERN = 0x80000000, 0x7FC00123

# name -> the parameter list include/agz.h documents
PROTOS = {
    "agz_replay_sample_slice_dev": "agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric, "
                                   "float* X_dev, float* Pi_dev, float* V_dev",
    "agz_replay_sample_slice": "agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric, "
                               "float* X, float* Pi, float* V",
    "agz_replay_digest": "agz_replay* rp, uint64_t* digest",
    "agz_replay_digest_host": "const float* planes, const float* policy, const float* value, int64_t n, int Features, int cells, "
                              "int PolicyLen, uint64_t* digest",
    "agz_train_replay_sharded": "agz_trainer* t, agz_replay* rp, int steps, uint64_t seed, int symmetric, int verify, float* last_cost",
}


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest_py(planes, policy, value):
    """the declared definition over uint32 arrays planes [n, xs], policy [n, A1], value [n], in Python integers"""
    n, xs, A1 = len(value), planes.shape[1], policy.shape[1]
    rowlen = xs + A1 + 1
    d = n
    for j in range(n):
        row = [int(b) for b in planes[j]] + [int(b) for b in policy[j]] + [int(value[j])]
        for e, bits in enumerate(row):
            d = (d + mix64(mix64((j * rowlen + e) & M64) ^ bits)) & M64
    return d


def pattern(i):
    """tests/cpp/replay_digest_check.cpp's pattern(i)"""
    if i % 7 == 3:
        return NEG_ZERO
    if i % 11 == 5:
        return NAN_PATTERN
    return (i * 2654435761 + 12345) & 0xFFFFFFFF


def fixed_rows(n, xs, A1):
    p = np.array([[pattern(j * xs + e) for e in range(xs)] for j in range(n)], np.uint32).reshape(n, xs)
    q = np.array([[pattern(1000 + j * A1 + e) for e in range(A1)] for j in range(n)], np.uint32).reshape(n, A1)
    v = np.array([pattern(2000 + j) for j in range(n)], np.uint32)
    return p, q, v


def digest_lib(p, q, v, F, cells):
    """agz_replay_digest_host over the patterns taken as float32 (a view: a NaN keeps its payload)"""
    return capi.replay_digest_host(p.view(np.float32), q.view(np.float32), v.view(np.float32), F, cells, q.shape[1])


def test_the_new_calls_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    L = capi.lib()
    for name, params in PROTOS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "include/agz.h does not declare %s" % name
        assert " ".join(m.group(1).split()) == params, name
        fn = getattr(L, name)                                           # AttributeError: libagz.so does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1, "agogo_amd/capi.py binds %s with %r" % (name, fn.argtypes)
    for attr in ("sample_slice", "sample_slice_dev", "digest"):
        assert callable(getattr(capi.Replay, attr))
    assert callable(capi.replay_digest_host) and callable(capi.Trainer.train_replay_sharded)


def test_mix64_is_the_finaliser_of_the_draw():
    from test_replay_cpu import out_py
    for seed, i in ((0, 0), (7, 3), (2024, 2 ** 40)):
        assert mix64((seed + (i + 1) * 0x9E3779B97F4A7C15) & M64) == out_py(seed, i)


def test_the_header_under_plain_gxx_against_python(tmp_path):
    exe = str(tmp_path / "replay_digest_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "replay_digest_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "DIGEST OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    got = {tuple(int(x) for x in line.split()[1:4]): int(line.split()[4]) for line in out.stdout.splitlines() if line.startswith("digest ")}
    assert set(got) == {(n, xs, A1) for n in NS for xs in XS for A1 in AS}
    seen = set()
    for (n, xs, A1), d in got.items():
        p, q, v = fixed_rows(n, xs, A1)
        assert d == digest_py(p, q, v), (n, xs, A1)
        assert d == digest_lib(p, q, v, 1, xs), (n, xs, A1)
        if xs == 18:
            assert d == digest_lib(p, q, v, 2, 9)                     # only F * cells enters
        seen |= set(np.concatenate([p.ravel(), q.ravel(), v]).tolist())
    assert {NEG_ZERO, NAN_PATTERN} <= seen                              # -0.0 and a NaN pattern were among the values
    assert [got[(0, xs, A1)] for xs in XS for A1 in AS] == [0] * 6      # an empty set: digest = n = 0


def test_the_digest_sees_row_order_and_the_sign_of_zero():
    p, q, v = fixed_rows(5, 18, 10)
    base = digest_py(p, q, v)
    assert base == digest_lib(p, q, v, 2, 9)
    order = [0, 3, 2, 1, 4]                                             # rows 1 and 3 swapped
    swapped = digest_py(p[order], q[order], v[order])
    assert swapped != base and swapped == digest_lib(p[order], q[order], v[order], 2, 9)
    z = p.copy()
    z[2, 4] = 0                                                         # +0.0 ...
    plus = digest_py(z, q, v)
    z[2, 4] = NEG_ZERO                                                  # ... to -0.0 in one cell
    minus = digest_py(z, q, v)
    assert plus != minus
    assert digest_lib(z, q, v, 2, 9) == minus
    z[2, 4] = 0
    assert digest_lib(z, q, v, 2, 9) == plus
    # one row fewer, and the same rows under another row length, are other digests too
    assert digest_py(p[:4], q[:4], v[:4]) != base
    assert digest_py(p.reshape(10, 9), np.concatenate([q, q]), np.concatenate([v, v])) != base


def test_argument_checks_without_a_device():
    L = capi.lib()
    f = (C.c_float * 64)()
    d = C.c_uint64(0)
    assert L.agz_replay_sample_slice_dev(None, 8, 0, 8, 1, 0, 0, None, None, None) == INVALID
    assert b"NULL" in L.agz_last_error()
    assert L.agz_replay_sample_slice(None, 8, 0, 8, 1, 0, 0, f, f, f) == INVALID
    assert L.agz_replay_digest(None, C.byref(d)) == INVALID
    assert L.agz_train_replay_sharded(None, None, 1, 0, 0, 1, None) == INVALID
    assert b"agz_train_replay_sharded" in L.agz_last_error()
    assert L.agz_replay_digest_host(f, f, f, 1, 2, 9, 10, None) == INVALID
    assert L.agz_replay_digest_host(f, f, f, -1, 2, 9, 10, C.byref(d)) == INVALID
    assert L.agz_replay_digest_host(None, f, f, 1, 2, 9, 10, C.byref(d)) == INVALID
    assert L.agz_replay_digest_host(f, f, f, 1, 0, 9, 10, C.byref(d)) == INVALID
    assert L.agz_replay_digest_host(None, None, None, 0, 2, 9, 10, C.byref(d)) == 0 and d.value == 0
    with pytest.raises(capi.AgzError):                                  # PolicyLen < 1, through the binding
        capi.replay_digest_host(np.zeros((1, 18), np.float32), np.zeros((1, 0), np.float32), np.zeros(1, np.float32), 2, 9, 0)
