"""CPU: the replay window's draw and ring arithmetic (agogo_amd/csrc/replay.hpp), on the code the sampler kernel compiles.

replay.hpp is the one definition host and device share: k_replay_sample (replay.hip) and agz_replay_draw.  It includes nothing from HIP,
so tests/cpp/replay_check.cpp runs it under g++ -Wall -Werror and prints every draw and slot it computes; here they are recomputed with
Python integers from the declared definition:

    out(seed, i) = finaliser(seed + (i + 1) * 0x9E3779B97F4A7C15)        the i-th output of SplitMix64 seeded with `seed`
    q = step * rows + r;  z0 = out(seed, 2q);  z1 = out(seed, 2q + 1);  j = (z0 * n) >> 64;  k = z1 >> 61 (0 when not symmetric)
    slot(j) = (total - min(total, cap) + j) mod cap;  an append writes slot total mod cap

and the same through libagz (agz_replay_draw needs no context)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
SEEDS = (1, 7, 2024)
STEPS = (0, 1, 2 ** 33)
ROWS = (1, 3, 64)
NS = (1, 5, 7, 2 ** 31 + 3)


def out_py(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_py(seed, step, rows, n, symmetric=True):
    """[(j, k)] of the `rows` rows of minibatch `step` over n live rows"""
    res = []
    for r in range(rows):
        q = (step * rows + r) & M64
        z0, z1 = out_py(seed, (2 * q) & M64), out_py(seed, (2 * q + 1) & M64)
        res.append(((z0 * n) >> 64, (z1 >> 61) if symmetric else 0))
    return res


def slot_py(cap, total, j):
    return (total - min(total, cap) + j) % cap


def test_the_known_first_output():
    assert out_py(0, 0) == 0xE220A8397B1DCDAF


def test_the_header_under_plain_gxx_against_python(tmp_path):
    exe = str(tmp_path / "replay_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "replay_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "REPLAY OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    draws = [tuple(int(x) for x in line.split()[1:]) for line in out.stdout.splitlines() if line.startswith("draw ")]
    assert len(draws) == len(SEEDS) * len(STEPS) * len(NS) * 2 * sum(ROWS)
    want = {}
    seen = set()
    for seed, step, rows, n, symmetric, r, j, k in draws:
        key = (seed, step, rows, n, symmetric)
        if key not in want:
            want[key] = draw_py(seed, step, rows, n, bool(symmetric))
        assert want[key][r] == (j, k), (key, r, j, k)
        seen.add(key)
    assert seen == {(s, t, r, n, y) for s in SEEDS for t in STEPS for r in ROWS for n in NS for y in (0, 1)}
    slots = [tuple(int(x) for x in line.split()[1:]) for line in out.stdout.splitlines() if line.startswith("slot ")]
    states = set()
    for cap, total, j, s, head in slots:
        assert s == slot_py(cap, total, j) and head == total % cap, (cap, total, j, s, head)
        states.add((cap, "before" if total < cap else "at" if total == cap else "after"))
    assert states >= {(c, w) for c in (5, 7) for w in ("before", "at", "after")}      # ring states before, at and after the wrap


@pytest.mark.parametrize("seed", SEEDS)
def test_replay_draw_through_the_library_equals_the_restatement(seed):
    for step in STEPS:
        for rows in ROWS:
            for n in NS:
                want = draw_py(seed, step, rows, n, True)
                j, k = capi.replay_draw(seed, step, rows, n, symmetric=True)
                assert [int(x) for x in j] == [w[0] for w in want], (seed, step, rows, n)
                assert [int(x) for x in k] == [w[1] for w in want], (seed, step, rows, n)
                j0, k0 = capi.replay_draw(seed, step, rows, n, symmetric=False)
                assert not k0.any()                                   # symmetric off: every k is 0 ...
                np.testing.assert_array_equal(j0, j)                  # ... and the rows drawn are unchanged


def test_a_run_is_one_sequential_stream_whatever_the_minibatch_size():
    """draw q depends on step * rows + r alone: 2 steps of 6 rows are 4 steps of 3 rows"""
    a = [d for step in range(2) for d in draw_py(7, step, 6, 5)]
    b = [d for step in range(4) for d in draw_py(7, step, 3, 5)]
    assert a == b
    ja = np.concatenate([capi.replay_draw(7, step, 6, 5)[0] for step in range(2)])
    jb = np.concatenate([capi.replay_draw(7, step, 3, 5)[0] for step in range(4)])
    np.testing.assert_array_equal(ja, jb)
    assert [int(x) for x in ja] == [d[0] for d in a]


def test_sanity_of_the_definition():
    """guards on the declared definition itself (computed from it, not from the library): 64 draws at n = 5 reach all five rows and all
    eight symmetries under each seed; 8 steps x 512 rows at n = 7 under seed 2024 give every row 585 +- 90 draws (expected 4096 / 7)"""
    for seed in SEEDS:
        d = draw_py(seed, 0, 64, 5)
        assert {x[0] for x in d} == set(range(5)), seed
        assert {x[1] for x in d} == set(range(8)), seed
        j, k = capi.replay_draw(seed, 0, 64, 5)
        assert set(j.tolist()) == set(range(5)) and set(k.tolist()) == set(range(8))
    counts_py, counts_lib = np.zeros(7, int), np.zeros(7, int)
    for step in range(8):
        for j, _ in draw_py(2024, step, 512, 7):
            counts_py[j] += 1
        np.add.at(counts_lib, capi.replay_draw(2024, step, 512, 7)[0], 1)
    assert (np.abs(counts_py - 585) <= 90).all(), counts_py
    np.testing.assert_array_equal(counts_lib, counts_py)


def test_argument_checks_without_a_device():
    L = capi.lib()
    INVALID = -1
    j, k = (C.c_int64 * 4)(), (C.c_int32 * 4)()
    assert L.agz_replay_draw(1, 0, 0, 5, 1, j, k) == INVALID           # rows < 1
    assert L.agz_replay_draw(1, 0, 4, 0, 1, j, k) == INVALID           # n < 1
    assert L.agz_replay_draw(1, 0, 4, 5, 1, None, None) == INVALID
    assert L.agz_replay_draw(1, 0, 4, 5, 1, j, None) == 0 and L.agz_replay_draw(1, 0, 4, 5, 1, None, k) == 0
    with pytest.raises(capi.AgzError):
        capi.replay_draw(1, 0, 0, 5)
    # NULL handles
    out = C.c_void_p()
    assert L.agz_replay_create(None, 2, 3, 3, 10, 5, C.byref(out)) == INVALID
    assert b"NULL" in L.agz_last_error()
    live = C.c_int64(0)
    assert L.agz_replay_count(None, C.byref(live), None, None) == INVALID
    assert L.agz_replay_clear(None) == INVALID
    assert L.agz_replay_append_examples(None, None) == INVALID
    assert L.agz_replay_append_dev(None, None, None, None, 0) == INVALID
    assert L.agz_replay_append_host(None, None, None, None, 0) == INVALID
    assert L.agz_replay_get(None, 0, 0, None, None, None) == INVALID
    assert L.agz_replay_sample_dev(None, 1, 0, 0, 0, None, None, None) == INVALID
    assert L.agz_replay_sample(None, 1, 0, 0, 0, None, None, None) == INVALID
    assert L.agz_train_replay(None, None, 1, 0, 0, None) == INVALID
    L.agz_replay_destroy(None)                                          # a no-op
