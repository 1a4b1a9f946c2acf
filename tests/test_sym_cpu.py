"""CPU: the eight board symmetries and the leaf-symmetry key (agogo_amd/csrc/sym.hpp), on the code the kernels compile.

sym.hpp is the one definition host and device share: k_select / k_expand (leaf symmetry), k_augment_rot (rotation and dihedral
augmenter) and the host helpers of agz.h.  It includes nothing from HIP, so tests/cpp/sym_check.cpp runs it under g++: bijections,
dst o src = id, inv, the group (distinct, closed), S_0..S_3 = the rotation augmenter's rot_src, S_k = R^(k&3) o T^(k>>2) generator by
generator, for m = 4, 5, 19.  Here the same maps come through libagz (agz_symmetry_map / _inverse / agz_leaf_symmetry_of, which need
no context) and are compared with a numpy restatement whose orientation is fixed by the definition (R x)[i][j] = x[j][m-1-i], and
with a Python restatement of mix32."""
import os
import subprocess

import numpy as np
import pytest

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4, 5, 19)


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def leaf_symmetry_py(seed, board, to_move):
    """AGZ_SYM_RANDOM's k, restated: ph = sum mix32(4 i + board[i] + 1) + mix32(0xABCD0000 + to_move); k = mix32(ph ^ lo ^ hi) >> 29"""
    with np.errstate(over="ignore"):
        b = np.asarray(board, np.uint32).reshape(-1)
        ph = mix32(np.arange(b.size, dtype=np.uint32) * np.uint32(4) + b + np.uint32(1)).sum(dtype=np.uint32)
        ph = np.uint32(ph + mix32(np.uint32(0xABCD0000) + np.uint32(to_move)))
        fold = np.uint32(seed & 0xFFFFFFFF) ^ np.uint32((seed >> 32) & 0xFFFFFFFF)
        return int(mix32(ph ^ fold) >> np.uint32(29))


def R(x):
    """(R x)[i][j] = x[j][m-1-i]: column m-1-i of x read downwards is row i — np.rot90's own (counter-clockwise) quarter turn"""
    m = x.shape[0]
    y = np.rot90(x, 1)
    assert all(y[i, j] == x[j, m - 1 - i] for i in range(m) for j in range(m))       # the orientation, from the definition
    return y


def S(x, k):
    """S_k = R^(k&3) o T^(k>>2)"""
    y = x.T if k >> 2 else x
    for _ in range(k & 3):
        y = R(y)
    return np.ascontiguousarray(y)


def test_the_header_under_plain_gxx_and_its_keys_against_python(tmp_path):
    exe = str(tmp_path / "sym_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sym_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "SYM OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    keys = [line.split() for line in out.stdout.splitlines() if line.startswith("key ")]
    assert len(keys) == 64
    for w in keys:
        seed, to_move, k = int(w[1]), int(w[2]), int(w[3])
        assert leaf_symmetry_py(seed, np.array(w[4:], np.int32), to_move) == k


@pytest.mark.parametrize("m", SIZES)
def test_symmetry_map_equals_numpy_on_a_board_without_symmetry(m):
    x = np.arange(m * m, dtype=np.int64).reshape(m, m)            # every cell its own value: no symmetry of its own
    seen = set()
    for k in range(8):
        src = capi.symmetry_map(m, k)
        assert sorted(src.tolist()) == list(range(m * m))          # a bijection
        np.testing.assert_array_equal(x.reshape(-1)[src].reshape(m, m), S(x, k), err_msg="m %d k %d" % (m, k))
        inv = capi.symmetry_inverse(k)
        dst = capi.symmetry_map(m, inv)
        np.testing.assert_array_equal(dst[src], np.arange(m * m))  # dst_k o src_k = id
        np.testing.assert_array_equal(src[dst], np.arange(m * m))
        seen.add(tuple(src.tolist()))
    assert len(seen) == 8
    for a in range(8):                                              # closed under composition
        for b in range(8):
            assert tuple(capi.symmetry_map(m, a)[capi.symmetry_map(m, b)].tolist()) in seen
    np.testing.assert_array_equal(capi.symmetry_map(m, 0), np.arange(m * m))


def test_helper_argument_checks():
    for bad in (-1, 8):
        with pytest.raises(capi.AgzError):
            capi.symmetry_map(5, bad)
        with pytest.raises(capi.AgzError):
            capi.symmetry_inverse(bad)
    with pytest.raises(capi.AgzError):
        capi.symmetry_map(20, 0)
    assert [capi.symmetry_inverse(k) for k in range(8)] == [0, 3, 2, 1, 4, 5, 6, 7]


def test_leaf_symmetry_of_equals_the_restatement_and_reaches_all_eight():
    rng = np.random.default_rng(2024)
    counts_py, counts_lib = np.zeros(8, int), np.zeros(8, int)
    for t in range(1000):
        m = SIZES[t % 3]
        board = rng.integers(0, 3, size=m * m).astype(np.int32)
        to_move = int(rng.integers(1, 3))
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) if t % 4 else t      # 64-bit seeds, and small ones
        kp = leaf_symmetry_py(seed, board, to_move)
        kl = capi.leaf_symmetry_of(seed, board, to_move)
        assert kp == kl, (t, seed, to_move)
        counts_py[kp] += 1
        counts_lib[kl] += 1
    # condition, not measurement: 1000 draws over eight values, 125 expected each; the restatement alone first
    assert (counts_py > 0).all(), counts_py
    assert (counts_lib > 0).all(), counts_lib
    # the seed matters, and so does the mover
    b = rng.integers(0, 3, size=81).astype(np.int32)
    assert len({capi.leaf_symmetry_of(s, b, 1) for s in range(64)}) > 1
    assert len({(capi.leaf_symmetry_of(s, b, 1), capi.leaf_symmetry_of(s, b, 2)) for s in range(64)}) > 1
    assert capi.leaf_symmetry_of(1 << 32, b, 1) == capi.leaf_symmetry_of(1, b, 1)                # the documented fold: lo ^ hi
