"""GPU: the few-boards form of the 16-bit block (AGZ_BF16_SMALL_FEW_*, conv_bf16f.hpp) — one 32 x 32 accumulator tile per wave, the run's
slice resident in LDS, the weight tiles through a six-stage ring with counted waits; K never split, so every bit is the whole-board kernel's.

  equal      tower output, policy and value under FEW_ALWAYS are those under OFF on the same net and planes, bit for bit, with 1, 2 and
             4 row blocks per workgroup (where the asked rb does not fit the slice, the launcher's own choice runs), bf16 and fp16.
  float64    the rule of test_bf16_small_gpu.py::test_whole_tower_against_float64 on the few-boards form's output.
  policy     FEW_AUTO, the getter, unknown values, and the modes and nets where the setting is inert.
  fallback   a net whose RB = 1 slice does not fit: FEW_ALWAYS runs the small form.
"""
import numpy as np
import pytest
import torch

import agogo_amd as A
from agogo_amd import capi
from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
from test_bf16_act_gpu import conv_r
from test_bf16_small_gpu import forward, same
from test_tower_f64_gpu import C, build_net, draw_planes

pytestmark = pytest.mark.gpu
OFF, FEW_AUTO, FEW = capi.BF16_SMALL_OFF, capi.BF16_SMALL_FEW_AUTO, capi.BF16_SMALL_FEW_ALWAYS
ACT, FP16 = capi.COMPUTE_BF16_ACT, capi.COMPUTE_FP16
PATHS = {ACT: (capi.NPATH_BLK_BF16_ACT, capi.NPATH_BLK_BF16_ACT_FEW), FP16: (capi.NPATH_BLK_FP16_ACT, capi.NPATH_BLK_FP16_ACT_FEW)}

#        K, W, H, F, L, B
CASES = [(64, 7, 6, 2, 2, 3),        # nine steps: less than two laps of the ring; 42 rows, a ragged second row block; <f32, 16> and <16, f32>
         (128, 9, 9, 18, 3, 2),      # 18 steps, <16, 16> in the middle, odd width, ragged third row block
         (128, 19, 19, 18, 3, 1),    # one board: 12 row blocks, runs that start mid-line, the 9-row tail
         (192, 19, 19, 18, 3, 3),    # 27 steps, not a multiple of the ring; six column tiles: both 4 KB pieces
         (64, 21, 20, 2, 3, 2)]      # the widest slice
_runs = {}


def run(ctx, mode, case):
    """one net per (mode, case), the same planes (boards scaled over 4^+-2; of several boards the last all zero) off and with every rb"""
    if (mode, case) not in _runs:
        K, W, H, F, L, B = case
        c = C("few", mode, 0, K, W, H, L, B, None, F=F)
        net, P, conf, _ = build_net(ctx, c, 9100 + K + W + L)
        try:
            x = draw_planes(B, c, 9200 + K + W + L)
            if B > 1:
                x[B - 1] = 0
            out = {0: forward(net, x, OFF)}
            for rb in (1, 2, 4):
                out[rb] = forward(net, x, FEW, rb)
        finally:
            net.close()
        _runs[mode, case] = (c, P, conf, x, out)
    return _runs[mode, case]


@pytest.mark.parametrize("rb", [1, 2, 4])
@pytest.mark.parametrize("mode,case", [(ACT, s) for s in CASES] + [(FP16, CASES[0]), (FP16, CASES[2])],
                         ids=lambda s: "K%d-%dx%d-F%d-L%d-B%d" % s if isinstance(s, tuple) else "fp16" if s == FP16 else "bf16")
def test_equal_to_the_whole_board_kernel_bit_for_bit(ctx, mode, case, rb):
    out = run(ctx, mode, case)[4]
    assert (out[0][3], out[rb][3]) == PATHS[mode]
    assert same(out[0], out[rb])


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=lambda s: "K%d-%dx%d-L%d" % (s[0], s[1], s[2], s[4]))
def test_whole_tower_against_float64(ctx, case):
    c, P, conf, x, out = run(ctx, ACT, case)
    dev, pol, val, _ = out[1]
    f64t = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64 = f64t.tower(x).numpy()
    mod = Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_FEW_TOWER | K %d %dx%d L %d B %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (case[0], case[1], case[2], case[4], case[5], loc_m, loc_d, 2 * loc_m, dif_m, dif_d, 2 * dif_m))
    assert loc_d <= 2 * loc_m and dif_d <= 2 * dif_m
    p64, v64 = f64t.heads(dev)                 # the heads: fp32-grade kernels on the device's own tower output
    assert np.all(np.abs(pol - p64) <= 2e-5 + 1e-4 * np.abs(p64)) and np.all(np.abs(val - v64) <= 1e-4)


def test_few_auto_the_getter_and_unknown_values(ctx):
    c = C("auto", ACT, 0, 64, 7, 6, 2, 512, None)      # the whole-board grid is B workgroups
    net, _, _, _ = build_net(ctx, c, 9300)
    try:
        x = draw_planes(512, c, 9301)
        for B, want in ((1, PATHS[ACT][1]), (512, PATHS[ACT][0])):
            off, auto = forward(net, x[:B], OFF), forward(net, x[:B], FEW_AUTO)
            assert off[3] == PATHS[ACT][0] and auto[3] == want and same(off, auto)
        assert net.get_bf16_small_batch() == FEW_AUTO
        for bad in (5, -1):
            with pytest.raises(A.AgzError, match=r"\(-1\)"):       # AGZ_E_INVALID
                net.set_bf16_small_batch(bad)
            assert net.get_bf16_small_batch() == FEW_AUTO
    finally:
        net.close()


@pytest.mark.parametrize("mode,L", [(capi.COMPUTE_BF16, 2), (ACT, 1)])
def test_inert_outside_the_16_bit_activation_tower(ctx, mode, L):
    c = C("inert", mode, 0, 64, 7, 6, L, 3, None)
    net, _, _, _ = build_net(ctx, c, 9400 + L)
    try:
        x = draw_planes(3, c, 9401)
        off, on = forward(net, x, OFF), forward(net, x, FEW)
        assert off[3] == capi.NPATH_BLK_BF16 and on[3] == capi.NPATH_BLK_BF16 and same(off, on)
    finally:
        net.close()


# K = 576 at 19x19: a 32-row run spans up to 5 haloed lines of 21 pixels x 9 chunks = 945 > BF16F_SPC_MAX = 864, the smallest K refused at 19x19
@pytest.mark.parametrize("case", [(576, 19, 19, 18, 2, 1)], ids=lambda s: "K%d-%dx%d" % s[:3])
def test_a_slice_that_does_not_fit_runs_the_small_form(ctx, case):
    K, W, H, F, L, B = case
    c = C("fall", ACT, 0, K, W, H, L, B, None, F=F)
    net, _, _, _ = build_net(ctx, c, 9500)
    try:
        x = draw_planes(B, c, 9501)
        off, few = forward(net, x, OFF), forward(net, x, FEW)
        assert off[3] == capi.NPATH_BLK_BF16_ACT and few[3] == capi.NPATH_BLK_BF16_ACT_SMALL and same(off, few)
    finally:
        net.close()
