"""GPU: the small-batch form of the AGZ_COMPUTE_BF16_ACT block (agz_net_set_bf16_small_batch, conv_bf16s.hpp) — one board split over
32-row x 64-column wave tiles, K never split, so every bit is that mode's.

  equal      tower output, policy and value under AGZ_BF16_SMALL_ALWAYS are those under AGZ_BF16_SMALL_OFF on the same net and planes,
             bit for bit, with 1, 2 and 4 row blocks per workgroup, at every (K, board, blocks) that takes another path through the kernel.
  float64    the rule of test_bf16_act_gpu.py::test_whole_tower_against_float64 on the small form's output.
  auto       AGZ_BF16_SMALL_AUTO takes the small form below a workgroup per CU and the whole-board kernel above, the same bits both times.
  inert      under AGZ_COMPUTE_BF16 and on a one-block net the setting changes nothing.
"""
import numpy as np
import pytest
import torch

from agogo_amd import capi
from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
from test_bf16_act_gpu import conv_r
from test_tower_f64_gpu import C, build_net, draw_planes

pytestmark = pytest.mark.gpu
OFF, AUTO, ALWAYS = capi.BF16_SMALL_OFF, capi.BF16_SMALL_AUTO, capi.BF16_SMALL_ALWAYS
P15, P16, P17 = capi.NPATH_BLK_BF16, capi.NPATH_BLK_BF16_ACT, capi.NPATH_BLK_BF16_ACT_SMALL

# The stage holds 256 haloed pixels.  The widest slice of a run of rb = 4 row blocks (128 rows): 7x6 the whole board, 8 lines x 9 = 72;
# 9x9 the whole board, 11 x 11 = 121; 19x19 8 lines + 2, 10 x 21 = 210; 21x20 8 lines + 2, 10 x 23 = 230.  Every rb fits every case:
# AGZ_BF16_SMALL_ALWAYS always takes path 17.
#        K, W, H, F, L, B
CASES = [(64, 7, 6, 2, 2, 1),        # one chunk, 42 rows: a live block of 32 and a ragged one of 10, two column tiles, <f32, bf16> and <bf16, f32>
         (128, 9, 9, 18, 3, 2),      # two chunks, 81 rows: the third row block ragged, <bf16, bf16> in the middle, odd width, uneven runs at rb = 2
         (128, 19, 19, 18, 4, 1),    # 12 row blocks, runs that start mid-line with line0 > 0, both stages reused, the 9-row tail
         (192, 19, 19, 18, 3, 3),    # three chunks, six column tiles: pieces j = 0, 1 of three 16 KB weight images
         (64, 21, 20, 2, 3, 2)]      # 420 rows: the whole-board kernel itself runs two runs per board; the widest slice per run
_runs = {}


def forward(net, x, policy, rb=0):
    net.set_bf16_small_batch(policy)
    net.debug_set_bf16_small_rb(rb)
    pol, val = net.infer(x)
    return net.tower_out(len(x)), pol, val, net.last_paths()[1]


def same(a, b):
    return a[0].any() and all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))


def run(ctx, case):
    """one net per case, the same planes (boards scaled over 4^+-2; of several boards the last all zero) with the policy off and with
    every rb: kept for the float64 test"""
    if case not in _runs:
        K, W, H, F, L, B = case
        c = C("small", capi.COMPUTE_BF16_ACT, 0, K, W, H, L, B, None, F=F)
        net, P, conf, _ = build_net(ctx, c, 6100 + K + W + L)
        try:
            x = draw_planes(B, c, 6200 + K + W + L)
            if B > 1:
                x[B - 1] = 0
            out = {0: forward(net, x, OFF)}
            for rb in (1, 2, 4):
                out[rb] = forward(net, x, ALWAYS, rb)
        finally:
            net.close()
        _runs[case] = (c, P, conf, x, out)
    return _runs[case]


@pytest.mark.parametrize("rb", [1, 2, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "K%d-%dx%d-F%d-L%d-B%d" % s)
def test_equal_to_bf16_act_bit_for_bit(ctx, case, rb):
    out = run(ctx, case)[4]
    assert out[0][3] == P16 and out[rb][3] == P17
    assert same(out[0], out[rb])


@pytest.mark.parametrize("case", [CASES[2], CASES[0]], ids=lambda s: "K%d-%dx%d-L%d" % (s[0], s[1], s[2], s[4]))
def test_whole_tower_against_float64(ctx, case):
    c, P, conf, x, out = run(ctx, case)
    dev, pol, val, _ = out[1]
    f64t = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64 = f64t.tower(x).numpy()
    mod = Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_SMALL_TOWER | K %d %dx%d L %d B %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (case[0], case[1], case[2], case[4], case[5], loc_m, loc_d, 2 * loc_m, dif_m, dif_d, 2 * dif_m))
    assert loc_d <= 2 * loc_m and dif_d <= 2 * dif_m
    p64, v64 = f64t.heads(dev)                 # the heads: fp32-grade kernels on the device's own tower output
    assert np.all(np.abs(pol - p64) <= 2e-5 + 1e-4 * np.abs(p64)) and np.all(np.abs(val - v64) <= 1e-4)


def test_auto_takes_the_small_form_below_a_workgroup_per_cu(ctx):
    c = C("auto", capi.COMPUTE_BF16_ACT, 0, 64, 7, 6, 2, 512, None)      # the whole-board grid is B workgroups
    net, _, _, _ = build_net(ctx, c, 6300)
    try:
        x = draw_planes(512, c, 6301)
        for B, want in ((1, P17), (512, P16)):
            off, auto = forward(net, x[:B], OFF), forward(net, x[:B], AUTO)
            assert off[3] == P16 and auto[3] == want and same(off, auto)
        assert net.get_bf16_small_batch() == AUTO
    finally:
        net.close()


@pytest.mark.parametrize("mode,L", [(capi.COMPUTE_BF16, 2), (capi.COMPUTE_BF16_ACT, 1)])
def test_inert_outside_the_bf16_act_tower(ctx, mode, L):
    c = C("inert", mode, 0, 64, 7, 6, L, 3, None)
    net, _, _, _ = build_net(ctx, c, 6400 + L)
    try:
        x = draw_planes(3, c, 6401)
        off, on = forward(net, x, OFF), forward(net, x, ALWAYS)
        assert off[3] == P15 and on[3] == P15 and same(off, on)
    finally:
        net.close()
