"""GPU: the dihedral augmenter (agz_examples_augment_dihedral) and agz_symmetry_boards, against numpy.

S_k = R^(k&3) o T^(k>>2) with (R x)[i][j] = x[j][m-1-i] — np.rot90's own quarter turn — and T the transpose.  The kernel
is the rotation augmenter's, its source index generalised to the eight maps (k_augment_rot, sym.hpp): agz_examples_augment_rotate and
agz_rotate_boards must keep their results bit for bit, and S_0..S_3 are their images."""
import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi

pytestmark = pytest.mark.gpu


def S_apply(x, k):
    y = np.swapaxes(x, -1, -2) if k >> 2 else x
    return np.ascontiguousarray(np.rot90(y, k & 3, axes=(-2, -1)))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("m", [4, 5, 19])
def test_symmetry_boards_equals_numpy_and_the_rotations(ctx, m):
    rng = np.random.default_rng(m)
    boards = rng.standard_normal((3, m, m)).astype(np.float32)      # no symmetry of their own
    images = []
    for k in range(8):
        got = capi.symmetry_boards(ctx, boards, m, k).reshape(3, m, m)
        np.testing.assert_array_equal(bits(got), bits(S_apply(boards, k)), err_msg="m %d k %d" % (m, k))
        images.append(got.tobytes())
    assert len(set(images)) == 8
    rot = boards
    for k in range(4):                                               # k < 4: RotateBoard applied k times
        np.testing.assert_array_equal(bits(capi.symmetry_boards(ctx, boards, m, k).reshape(3, m, m)), bits(rot), err_msg="m %d k %d" % (m, k))
        rot = capi.rotate_boards(ctx, rot, m, m).reshape(3, m, m)
    np.testing.assert_array_equal(bits(rot), bits(boards))          # four quarter turns
    for bad in (-1, 8):
        with pytest.raises(A.AgzError, match="agz_symmetry_boards"):
            capi.symmetry_boards(ctx, boards, m, bad)


def filled(ctx, F, S, n, seed, tail=1):
    rng = np.random.default_rng(seed)
    planes = rng.standard_normal((n, F, S, S)).astype(np.float32)
    policy = rng.random((n, S * S + tail)).astype(np.float32)
    value = rng.standard_normal(n).astype(np.float32)
    ex = A.Examples(ctx, F, S, S, S * S + tail)
    ex.append_host(planes, policy, value)
    return ex, planes, policy, value


@pytest.mark.parametrize("F,S,n", [(2, 5, 7), (18, 9, 3)], ids=["f2-5x5", "f18-9x9"])
def test_augment_dihedral_rows_against_numpy_and_the_rotation_augmenter(ctx, F, S, n):
    ex, planes, policy, value = filled(ctx, F, S, n, seed=F + S)
    ex.augment_dihedral()
    assert len(ex) == 8 * n
    p, q, v = ex.get()
    p, cells = p.reshape(8 * n, F, S, S), S * S
    for e in range(n):
        for k in range(8):
            r = 8 * e + k                                            # every example e becomes [S_0 e .. S_7 e] in place of e
            np.testing.assert_array_equal(bits(p[r]), bits(S_apply(planes[e], k)), err_msg="planes of example %d, k %d" % (e, k))
            np.testing.assert_array_equal(bits(q[r, :cells].reshape(S, S)), bits(S_apply(policy[e, :cells].reshape(S, S), k)),
                                          err_msg="policy of example %d, k %d" % (e, k))
            assert bits(q[r, cells:]).tolist() == bits(policy[e, cells:]).tolist()          # the pass entry, copied
            assert bits(v[r:r + 1])[0] == bits(value[e:e + 1])[0]                             # the value, copied
    ex.close()
    # rows 0..3 of each group are the rotation augmenter's, bit for bit, on the same store
    rot, _, _, _ = filled(ctx, F, S, n, seed=F + S)
    rot.augment_rotate()
    assert len(rot) == 4 * n
    rp, rq, rv = rot.get()
    keep = (np.arange(8 * n) % 8) < 4
    np.testing.assert_array_equal(bits(p.reshape(8 * n, -1)[keep]), bits(rp))
    np.testing.assert_array_equal(bits(q[keep]), bits(rq))
    np.testing.assert_array_equal(bits(v[keep]), bits(rv))
    rot.close()


def test_augment_dihedral_preconditions(ctx):
    rect = A.Examples(ctx, 2, 3, 4, 13)
    with pytest.raises(A.AgzError, match="square boards"):
        rect.augment_dihedral()
    rect.close()
    short = A.Examples(ctx, 2, 4, 4, 10)
    with pytest.raises(A.AgzError, match="agz_examples_augment_dihedral"):
        short.augment_dihedral()
    short.close()
    empty = A.Examples(ctx, 2, 4, 4, 17)
    empty.augment_dihedral()                                         # nothing to do
    assert len(empty) == 0
    empty.close()
