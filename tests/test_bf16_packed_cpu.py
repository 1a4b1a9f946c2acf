"""CPU: agz_bf16_packed_boards_of, the host-only definition of the boards per workgroup of the packed-boards bf16 block (conv_bf16p.hpp):
as many as fit the workgroup's 384 GEMM rows and its LDS stage."""
import pytest

from agogo_amd import capi

ROWS = 384      # four waves x 96 GEMM rows
# gfx950 has 160 KB of LDS per workgroup: two 16 KB weight stages leave (160 - 32) KB / 2 / 128 B = 512 pixels per activation stage at
# the most; the kernel takes 496 (a whole number of 16-pixel half rounds that holds four 9x9 boards, 484)
STAGE = 496


@pytest.mark.parametrize("W,H,G", [(3, 3, 19), (7, 6, 6), (9, 9, 4), (13, 13, 2)])
def test_documented_values(W, H, G):
    assert capi.lib().agz_bf16_packed_boards_of(H, W) == G


@pytest.mark.parametrize("W,H", [(19, 19), (21, 20)])
def test_large_boards_have_no_form(W, H):
    assert capi.lib().agz_bf16_packed_boards_of(H, W) < 2


def test_is_the_largest_that_fits_rows_and_stage():
    of = capi.lib().agz_bf16_packed_boards_of
    assert STAGE * 128 * 2 + 2 * 16384 <= 160 * 1024
    for H in range(1, 22):
        for W in range(1, 22):
            G = of(H, W)
            assert G >= 0 and G * H * W <= ROWS and G * (H + 2) * (W + 2) <= STAGE, (H, W, G)
            assert (G + 1) * H * W > ROWS or (G + 1) * (H + 2) * (W + 2) > STAGE, (H, W, G)
