"""CPU: the licence and the row map of the chained Winograd tower's short positions (agogo_amd/csrc/gemm_maps.hpp).

Where the tiles hang over the board's edge (19 = 4 x 5 - 1) the last output row / column of the last tile row / column is discarded,
and in the compiled tables the last transform point (the "infinity" point, index AL - 1) feeds ONLY that output.  So the product at
position (xi, nu) of a last-row tile with xi == AL - 1 — and of a last-column tile with nu == AL - 1 — reaches no kept pixel: the
kernels neither store, multiply nor read those rows.  Checked here without a GPU: the zero structure of the compiled At; in exact
rational arithmetic that zeroing every dead product leaves every on-board pixel of a ragged tiled convolution unchanged; and, on the
header the kernels include (tests/cpp/wino_rows_check.cpp under g++), that the row map gives every live (board, tile) of a 128-row
slot its own row below the live count, dead tiles none, a wave contiguous rows, 96 / 64 / 64 live rows and 732 rows per 19x19 board."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_wino_h2_tables_cpu import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tm", [4, 5])
def test_the_last_transform_point_feeds_the_last_output_only(tm):
    al, vshift, BT, AT, G = tables(tm)
    assert al == tm + 2 and len(AT) == tm
    for l in range(tm - 1):
        assert AT[l][al - 1] == 0, (l, AT[l][al - 1])
    assert AT[tm - 1][al - 1] != 0


def _matmul(A, B):
    return [[sum(a * b for a, b in zip(row, col)) for col in zip(*B)] for row in A]


def _T(A):
    return [list(r) for r in zip(*A)]


@pytest.mark.parametrize("tm,H,W", [(5, 19, 19), (5, 9, 9), (4, 7, 7), (4, 6, 7)])
def test_zeroing_the_dead_products_keeps_every_on_board_pixel_exactly(tm, H, W):
    al, vshift, BT, AT, G = tables(tm)
    rng = np.random.default_rng(100 * H + W)
    x = [[Fraction(int(v)) for v in row] for row in rng.integers(-4, 5, (H, W))]
    g = [[Fraction(int(v)) for v in row] for row in rng.integers(-4, 5, (3, 3))]
    nty, ntx = -(-H // tm), -(-W // tm)
    dead_y, dead_x = tm * nty > H, tm * ntx > W
    assert dead_y and dead_x
    xp = [[Fraction(0)] * (ntx * tm + 2) for _ in range(nty * tm + 2)]
    for i in range(H):
        for j in range(W):
            xp[i + 1][j + 1] = x[i][j]
    U = _matmul(_matmul(G, g), _T(G))
    y = [[None] * (ntx * tm) for _ in range(nty * tm)]
    n_dead = 0
    for ty in range(nty):
        for tx in range(ntx):
            d = [row[tx * tm:tx * tm + al] for row in xp[ty * tm:ty * tm + al]]
            V = _matmul(_matmul(BT, d), _T(BT))
            M = [[U[xi][nu] * V[xi][nu] for nu in range(al)] for xi in range(al)]
            for xi in range(al):
                for nu in range(al):
                    if (dead_y and xi == al - 1 and ty == nty - 1) or (dead_x and nu == al - 1 and tx == ntx - 1):
                        M[xi][nu] = Fraction(0)          # never stored, multiplied or read: the kernels see zeros (or nothing)
                        n_dead += 1
            Y = _matmul(_matmul(AT, M), _T(AT))
            for k in range(tm):
                for l in range(tm):
                    y[ty * tm + k][tx * tm + l] = Y[k][l]
    assert n_dead == al * ntx + al * nty - 1             # every dead product (the map drops all but nty - 1 of them, gemm_maps.hpp); the corner tile's corner counted once
    for i in range(H):
        for j in range(W):
            ref = sum(xp[i + a][j + b] * g[a][b] for a in range(3) for b in range(3))
            assert y[i][j] == ref, (i, j)                # exact: Fractions


def test_row_map_properties(tmp_path):
    exe = str(tmp_path / "wino_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "wino_rows_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "WINO_ROWS OK" in out.stdout, out.stdout[-3000:]


def test_the_kernels_take_the_row_map_from_the_header():
    h2c = open(os.path.join(ROOT, "agogo_amd", "csrc", "conv_wino_h2c.hpp")).read()
    h2 = open(os.path.join(ROOT, "agogo_amd", "csrc", "conv_wino_h2.hpp")).read()
    for fn in ("maps::rows_pos_live", "maps::rows_row", "maps::rows_class", "maps::rows_per_board", "maps::rows_short_ok", "maps::rows_slot_live"):
        assert fn in h2c, fn
    assert "maps::rows_row" in h2 and "maps::rows_class" in h2
