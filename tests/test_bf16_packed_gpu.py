"""GPU: the packed-boards form of the AGZ_COMPUTE_BF16_ACT block (agz_net_set_bf16_packed_boards, conv_bf16p.hpp) — several small boards
per workgroup, K never split, so every bit is that mode's.

  equal      tower output, policy and value under AGZ_BF16_PACKED_ALWAYS are those under AGZ_BF16_PACKED_OFF on the same net and planes,
             bit for bit, with the launcher's G and with 2 and 3 boards per workgroup, at every board that takes another path.
  float64    the rule of test_bf16_act_gpu.py::test_whole_tower_against_float64 on the packed form's output.
  auto       AGZ_BF16_PACKED_AUTO takes the packed form where the whole-board grid exceeds the CU count, the same bits both sides.
  inert      under AGZ_COMPUTE_BF16, on a one-block net and at 19x19 the setting changes nothing; the small-batch form goes first.
"""
import numpy as np
import pytest
import torch

import agogo_amd as A
from agogo_amd import capi
from f64_tower import Tower, conv_direct, diffuse_metric, local_metric
from test_bf16_act_gpu import conv_r
from test_tower_f64_gpu import C, build_net, draw_planes

pytestmark = pytest.mark.gpu
OFF, AUTO, ALWAYS = capi.BF16_PACKED_OFF, capi.BF16_PACKED_AUTO, capi.BF16_PACKED_ALWAYS
P15, P16, P17, P18 = capi.NPATH_BLK_BF16, capi.NPATH_BLK_BF16_ACT, capi.NPATH_BLK_BF16_ACT_SMALL, capi.NPATH_BLK_BF16_ACT_PACKED

#        K, W, H, F, L, B
CASES = [(64, 7, 6, 2, 2, 7),        # G = 6: a full group of 252 rows (third wave ragged, fourth dead) and a tail of one; <f32, bf16>, <bf16, f32>
         (128, 9, 9, 18, 3, 5),      # G = 4: 324 rows, 484 staged pixels (last DMA round partial), two chunks, <bf16, bf16>, odd width
         (64, 3, 3, 2, 2, 20),       # G = 19: a 16-lane read crosses a board boundary at every tap; tail of one
         (192, 13, 13, 18, 3, 3)]    # G = 2: 338 rows, 450 pixels, three chunks, three n-tiles; tail of one
GS = [(case, g) for case in CASES for g in (0, 2, 3) if g <= capi.lib().agz_bf16_packed_boards_of(case[2], case[1])]
_runs = {}


def forward(net, x, policy, g=0):
    net.set_bf16_packed_boards(policy)
    net.debug_set_bf16_packed_g(g)
    pol, val = net.infer(x)
    return net.tower_out(len(x)), pol, val, net.last_paths()[1]


def same(a, b):
    return a[0].any() and all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))


def run(ctx, case):
    """one net per case, the same planes (boards scaled over 4^+-2, the last all zero) with the policy off and with every G: kept for
    the float64 test"""
    if case not in _runs:
        K, W, H, F, L, B = case
        c = C("packed", capi.COMPUTE_BF16_ACT, 0, K, W, H, L, B, None, F=F)
        net, P, conf, _ = build_net(ctx, c, 7100 + K + W + L)
        try:
            x = draw_planes(B, c, 7200 + K + W + L)
            x[B - 1] = 0
            out = {"off": forward(net, x, OFF)}
            for g in (g for cs, g in GS if cs == case):
                out[g] = forward(net, x, ALWAYS, g)
        finally:
            net.close()
        _runs[case] = (c, P, conf, x, out)
    return _runs[case]


@pytest.mark.parametrize("case,g", GS, ids=lambda v: "K%d-%dx%d-F%d-L%d-B%d" % v if isinstance(v, tuple) else "G%d" % v)
def test_equal_to_bf16_act_bit_for_bit(ctx, case, g):
    out = run(ctx, case)[4]
    assert out["off"][3] == P16 and out[g][3] == P18
    assert same(out["off"], out[g])


@pytest.mark.parametrize("case", [CASES[1], CASES[0]], ids=lambda s: "K%d-%dx%d-L%d" % (s[0], s[1], s[2], s[4]))
def test_whole_tower_against_float64(ctx, case):
    c, P, conf, x, out = run(ctx, case)
    dev, pol, val, _ = out[0]
    f64t = Tower(P, conf, c.bn, None, torch.float64, conv_direct)
    f64 = f64t.tower(x).numpy()
    mod = Tower(P, conf, c.bn, None, torch.float32, conv_r).tower(x).numpy()
    loc_m, loc_d = local_metric(mod, f64)[0], local_metric(dev, f64)[0]
    dif_m, dif_d = diffuse_metric(mod, f64), diffuse_metric(dev, f64)
    print("\nBF16_PACKED_TOWER | K %d %dx%d L %d B %d | local: model %.3e device %.3e bar %.3e | diffuse: model %.3e device %.3e bar %.3e"
          % (case[0], case[1], case[2], case[4], case[5], loc_m, loc_d, 2 * loc_m, dif_m, dif_d, 2 * dif_m))
    assert loc_d <= 2 * loc_m and dif_d <= 2 * dif_m
    p64, v64 = f64t.heads(dev)                 # the heads: fp32-grade kernels on the device's own tower output
    assert np.all(np.abs(pol - p64) <= 2e-5 + 1e-4 * np.abs(p64)) and np.all(np.abs(val - v64) <= 1e-4)


def test_auto_takes_the_packed_form_above_a_workgroup_per_cu(ctx):
    c = C("auto", capi.COMPUTE_BF16_ACT, 0, 64, 7, 6, 2, 512, None)      # the whole-board grid is B workgroups
    net, _, _, _ = build_net(ctx, c, 7300)
    try:
        x = draw_planes(512, c, 7301)
        for B, want in ((512, P18), (2, P16)):
            off, auto = forward(net, x[:B], OFF), forward(net, x[:B], AUTO)
            assert off[3] == P16 and auto[3] == want and same(off, auto)
        assert net.get_bf16_packed_boards() == AUTO
    finally:
        net.close()


@pytest.mark.parametrize("mode,W,H,L,path", [(capi.COMPUTE_BF16, 7, 6, 2, P15), (capi.COMPUTE_BF16_ACT, 7, 6, 1, P15),
                                             (capi.COMPUTE_BF16_ACT, 19, 19, 2, P16)])
def test_inert_where_the_form_does_not_exist(ctx, mode, W, H, L, path):
    c = C("inert", mode, 0, 64, W, H, L, 3, None)
    net, _, _, _ = build_net(ctx, c, 7400 + L + W)
    try:
        x = draw_planes(3, c, 7401)
        off, on = forward(net, x, OFF), forward(net, x, ALWAYS)
        assert off[3] == path and on[3] == path and same(off, on)
    finally:
        net.close()


def test_small_batch_form_goes_first_and_debug_g_is_checked(ctx):
    c = C("prec", capi.COMPUTE_BF16_ACT, 0, 64, 7, 6, 2, 2, None)
    net, _, _, _ = build_net(ctx, c, 7500)
    try:
        x = draw_planes(2, c, 7501)
        off = forward(net, x, OFF)
        net.set_bf16_small_batch(capi.BF16_SMALL_ALWAYS)
        both = forward(net, x, ALWAYS)
        assert both[3] == P17 and same(off, both)
        for g in (1, -1):
            with pytest.raises(A.AgzError, match=r"\(-1\)"):       # AGZ_E_INVALID
                net.debug_set_bf16_packed_g(g)
    finally:
        net.close()
