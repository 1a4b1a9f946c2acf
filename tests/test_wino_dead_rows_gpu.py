"""GPU: the chained Winograd tower with its short positions (agogo_amd/csrc/gemm_maps.hpp: the transform rows that only feed
off-board outputs are neither stored, multiplied nor read) against the same tower keeping every row — agz_net_set_wino_h2_gemm + 128,
the parent layout.  No term that reaches an on-board pixel changes or is reordered, so policy and value must be BIT-IDENTICAL; a
repeated call gives the same bits; and the first boards stay inside the suite's network tolerance of the oracle."""
import numpy as np
import pytest

import agogo_amd as A
from test_net_gpu import make_pair, rand_planes, POL_ATOL, POL_RTOL, VAL_ATOL

pytestmark = pytest.mark.gpu

KEEP_ALL = 128
LIVE = {19: 96, 9: 64, 7: 64}          # live rows per 128-row slot at the short positions (tests/cpp/wino_rows_check.cpp)


@pytest.mark.parametrize("K,S,B,L", [
    (128, 19, 9, 3),      # F(5x5,3x3), 96 live rows; ragged last 128-row slot
    (256, 19, 33, 2),     # the headline's K
    (128, 9, 37, 3),      # four boards per 16-tile group, 64 live rows
    (128, 7, 21, 3),      # F(4x4,3x3)
    (128, 19, 70, 2),     # one queue and two queues
])
def test_short_positions_are_bit_identical_to_every_row_kept(ctx, K, S, B, L):
    F = 18
    onet, gnet = make_pair(ctx, K, L, 32, S, S, F, S * S + 1, 2, seed=K + S)
    assert A.capi.wino_h2_chained(S, S, K) == 1
    x = rand_planes(B, F, S, S, seed=B)
    gnet.set_compute_mode(A.capi.COMPUTE_WINO_H2 | A.capi.COMPUTE_FORCE)
    for queues in ((1, 2) if B >= 64 else (0,)):
        gnet.set_tower_queues(queues)
        gnet.set_wino_h2_gemm(0)
        p, v = gnet.infer(x)
        assert gnet.wino_h2_last_rows() == (LIVE[S], LIVE[S])      # the short positions really are on
        p2, v2 = gnet.infer(x)
        gnet.set_wino_h2_gemm(1 + KEEP_ALL)
        pk, vk = gnet.infer(x)
        assert gnet.wino_h2_last_rows() == (0, 0)                  # ... and off in the run they are compared with
        gnet.set_wino_h2_gemm(0)
        assert np.all(np.isfinite(p)) and np.all(np.isfinite(v))
        np.testing.assert_array_equal(p, pk)
        np.testing.assert_array_equal(v, vk)
        np.testing.assert_array_equal(p, p2)
        np.testing.assert_array_equal(v, v2)
    gnet.set_tower_queues(0)
    nb = min(B, 4)
    po, vo = onet.infer(x[:nb])
    np.testing.assert_allclose(p[:nb], po, atol=POL_ATOL, rtol=POL_RTOL)
    np.testing.assert_allclose(v[:nb], vo, atol=VAL_ATOL)
    gnet.close()


def test_one_ragged_edge_only(ctx):
    """4 x 7 board, F(4x4,3x3): only the columns hang over the edge — class C alone, the (AL-1, AL-1) corner keeps every row"""
    K, L, F, W, H, B = 256, 2, 1, 7, 4, 9
    onet, gnet = make_pair(ctx, K, L, 2, W, H, F, 29, 0, seed=25)
    assert A.capi.wino_h2_chained(H, W, K) == 1
    x = rand_planes(B, F, H, W, seed=14)
    gnet.set_compute_mode(A.capi.COMPUTE_WINO_H2 | A.capi.COMPUTE_FORCE)
    gnet.set_latency_mode(False)
    p, v = gnet.infer(x)
    assert gnet.wino_h2_last_rows() == (0, 64)
    gnet.set_wino_h2_gemm(1 + KEEP_ALL)
    pk, vk = gnet.infer(x)
    assert gnet.wino_h2_last_rows() == (0, 0)
    np.testing.assert_array_equal(p, pk)
    np.testing.assert_array_equal(v, vk)
    po, vo = onet.infer(x[:4])
    np.testing.assert_allclose(p[:4], po, atol=POL_ATOL, rtol=POL_RTOL)
    np.testing.assert_allclose(v[:4], vo, atol=VAL_ATOL)
    gnet.close()
