"""No GPU: playout cap randomization (agz_arena_set_playout_cap, DESIGN.md §2 playout-cap), the host side.

The definition declared in include/agz.h is restated here in Python integers; agz_playout_cap_of (csrc/cap.hpp, the copy the device
kernel k_cap_decide compiles too) must equal it bit for bit.  The restatement is itself checked to be a fair coin at p = 0.25."""
import ctypes as C
import os
import re

import numpy as np

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
E_INVALID = -1
FULL, FAST = capi.CAP_FULL, capi.CAP_FAST

SYMBOLS = ("agz_arena_set_playout_cap", "agz_arena_get_playout_cap", "agz_arena_playout_cap", "agz_arena_playout_cap_counts", "agz_playout_cap_of")
DEBUG_SYMBOLS = ("agz_arena_set_cap_compact", "agz_arena_last_cap_batch")


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def threshold(p):
    """(uint32)(p_full * 16777216.0f): the float product is exact (a power of two), so float64 arithmetic on the float32 value gives it"""
    return int(float(np.float32(p)) * 16777216.0)


def kind_of(seed, key, ply, p):
    z = mix64(seed ^ mix64((key + 0x9E3779B97F4A7C15 * (ply + 1)) & M64))
    return FULL if (z >> 40) < threshold(p) else FAST


def test_abi_symbols_and_struct():
    L = capi.lib()
    with open(os.path.join(ROOT, "include", "agz.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "agz_debug.h")) as f:
        debug = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name).argtypes is not None, name
    for name in DEBUG_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, debug), name
        assert getattr(L, name).argtypes is not None, name
    assert "#define AGZ_CAP_FULL 0" in header and "#define AGZ_CAP_FAST 1" in header
    assert (FULL, FAST) == (0, 1)
    assert C.sizeof(capi.PlayoutCapConf) == 24
    assert [n for n, _ in capi.PlayoutCapConf._fields_] == ["p_full", "fast_budget", "on", "reserved", "seed"]
    assert capi.PlayoutCapConf.seed.offset == 16 and capi.PlayoutCapConf.on.offset == 8


P_VALUES = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.25, 0.5, 0.1, 0.9)


def test_host_function_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(20240611)
    n = 0
    for p in P_VALUES:
        seeds = [0, 1, M64] + [int(x) * 2 + 1 for x in rng.integers(0, 1 << 63, size=5, dtype=np.uint64)]
        for seed in seeds:
            keys = [0, M64, 0x9E3779B97F4A7C15] + [int(x) * 2 + (i & 1) for i, x in enumerate(rng.integers(0, 1 << 63, size=17, dtype=np.uint64))]
            for key in keys:
                for ply in [0, 1, 2, 721, 2 ** 31 - 2, 2 ** 31 - 1] + [int(x) for x in rng.integers(0, 800, size=2)]:
                    assert capi.playout_cap_of(seed, key, ply, p) == kind_of(seed, key, ply, p), (seed, key, ply, p)
                    n += 1
    assert n >= 10000, n


def test_the_two_ends_are_certain():
    rng = np.random.default_rng(7)
    for _ in range(2000):
        seed, key = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + 1, int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2
        ply = int(rng.integers(0, 722))
        assert capi.playout_cap_of(seed, key, ply, 1.0) == FULL == kind_of(seed, key, ply, 1.0)
        assert capi.playout_cap_of(seed, key, ply, 0.0) == FAST == kind_of(seed, key, ply, 0.0)
    assert threshold(1.0) == 1 << 24 and threshold(0.0) == 0 and threshold(2.0 ** -24) == 1 and threshold(1.0 - 2.0 ** -24) == (1 << 24) - 1


def test_a_quarter_of_the_plies_of_one_key_is_full():
    """2^16 consecutive plies of one key at p = 0.25: sigma of the share = sqrt(0.25 * 0.75 / 65536) = 0.0017, so 0.25 +- 0.01 is beyond
    5 sigma.  The restatement alone is held to the band, and the host function to the restatement."""
    n = 1 << 16
    for seed, key in ((0, 7), (0xC0FFEE, 0x123456789ABCDEF)):
        mine = np.array([kind_of(seed, key, ply, 0.25) for ply in range(n)])
        share = float((mine == FULL).mean())
        print("seed %#x key %#x: share of FULL %.5f" % (seed, key, share))
        assert abs(share - 0.25) <= 0.01, share
        theirs = np.array([capi.playout_cap_of(seed, key, ply, 0.25) for ply in range(0, n, 16)])
        np.testing.assert_array_equal(theirs, mine[::16])


def test_refusals_of_the_host_function():
    L = capi.lib()
    kind = C.c_int32(77)
    nan, inf = float("nan"), float("inf")
    for ply, p in ((-1, 0.25), (-2 ** 31, 0.25), (0, -0.5), (0, 1.0 + 2.0 ** -20), (0, 2.0), (0, nan), (0, inf), (0, -inf)):
        assert L.agz_playout_cap_of(1, 2, ply, p, C.byref(kind)) == E_INVALID, (ply, p)
        assert b"agz_playout_cap_of" in L.agz_last_error()
        assert kind.value == 77
    assert L.agz_playout_cap_of(1, 2, 0, 0.25, None) == E_INVALID
    assert L.agz_playout_cap_of(1, 2, 0, 0.25, C.byref(kind)) == 0 and kind.value in (FULL, FAST)
    assert L.agz_playout_cap_of(1, 2, 0, -0.0, C.byref(kind)) == 0 and kind.value == FAST      # -0.0 is 0
