"""GPU: the chained Winograd tower with its short positions' live rows PACKED into whole 128-row slots (agogo_amd/csrc/gemm_maps.hpp,
"packed short positions": the DMA GEMM launches no workgroup for the slots a packing group leaves empty) against the same tower keeping
every row — agz_net_set_wino_h2_gemm + 128.  Rows are independent and no accumulator's MFMA sequence changes, so policy and value must be
BIT-IDENTICAL.  K = 128 is the smallest width the chained form takes; two blocks run block 0's input transform, one pipelined out->in
kernel and the last block's kernel.  The board counts sit on the map's edges: one partly filled slot; a board whose rows straddle two
slots (board 10 of a 19x19 group); a second group with a one-board tail; two chunks on two queues, each with a tail of its own."""
import numpy as np
import pytest

import agogo_amd as A
from test_net_gpu import make_pair, rand_planes, POL_ATOL, POL_RTOL, VAL_ATOL

pytestmark = pytest.mark.gpu

KEEP_ALL = 128
LIVE = {19: 96, 9: 64, 7: 64}          # live rows per 128-row slot at the short positions (tests/test_wino_dead_rows_gpu.py)
K, L, F = 128, 2, 18

_pairs = {}


@pytest.fixture(scope="module")
def pair(ctx):
    def get(S):
        if S not in _pairs:
            _pairs[S] = make_pair(ctx, K, L, 32, S, S, F, S * S + 1, 2, seed=K + S)
            _pairs[S][1].set_compute_mode(A.capi.COMPUTE_WINO_H2 | A.capi.COMPUTE_FORCE)
        return _pairs[S]
    yield get
    for onet, gnet in _pairs.values():
        gnet.close()
    _pairs.clear()


@pytest.mark.parametrize("S,B,queues,oracle", [
    (19, 4, 0, True),       # one partly filled slot
    (19, 11, 0, False),     # board 10's rows straddle two slots
    (19, 33, 0, False),     # a second packing group with a one-board tail
    (19, 72, 2, False),     # two chunks of 36 boards on two queues, each with its own tail
    (9, 68, 0, False),      # 64 live rows: groups of 2 slots / 64 boards, tail
    (7, 36, 0, False),      # F(4x4,3x3)
])
def test_packed_rows_are_bit_identical_to_every_row_kept(pair, S, B, queues, oracle):
    onet, gnet = pair(S)
    assert A.capi.wino_h2_chained(S, S, K) == 1
    x = rand_planes(B, F, S, S, seed=B)
    gnet.set_tower_queues(queues)
    gnet.set_wino_h2_gemm(0)
    p, v = gnet.infer(x)
    assert gnet.wino_h2_last_rows() == (LIVE[S], LIVE[S])      # the short map (packed: there is no other) is on
    gnet.set_wino_h2_gemm(1 + KEEP_ALL)
    pk, vk = gnet.infer(x)
    assert gnet.wino_h2_last_rows() == (0, 0)                  # ... and off in the run it is compared with
    gnet.set_wino_h2_gemm(0)
    gnet.set_tower_queues(0)
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(v))
    np.testing.assert_array_equal(p, pk)
    np.testing.assert_array_equal(v, vk)
    if oracle:
        po, vo = onet.infer(x[:4])
        np.testing.assert_allclose(p[:4], po, atol=POL_ATOL, rtol=POL_RTOL)
        np.testing.assert_allclose(v[:4], vo, atol=VAL_ATOL)
