"""CPU: the packed map of the chained Winograd tower's short positions (agogo_amd/csrc/gemm_maps.hpp, "packed short positions").

Where the short map is on, the live rows of S = 128 / gcd(128, live) consecutive 128-row slots are packed into the first S * live / 128
slots of the group and the DMA GEMM launches no workgroup for the others.  tests/cpp/wino_pack_check.cpp includes the header the kernels
include under g++ and checks, for 19x19 / F(5), 9x9 / F(5), 7x7 / F(4) and 4x7 / F(4) at 1, bpt, S bpt - 1, S bpt, S bpt + 1 and a
multi-group number of boards: (board, live tile) -> (slot, row) is injective, dense, inside the group's first slots and inside the
allocation, and dead exactly where rows_local says; the per-group form the out->in kernels compute (uniform first row + per-thread
offset + the recomputed slot step) is that same address, and a dead lane stays out of range; the GEMM's tile decode enumerates every
used (position, slot, column tile) exactly once, position-major, and nothing else; full positions — and the whole grid with the map
off — are the old map."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_map_properties(tmp_path):
    exe = str(tmp_path / "wino_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "wino_pack_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "WINO_PACK OK" in out.stdout, out.stdout[-3000:]


def _body(src, name):
    i = src.index("void %s(" % name)
    j = src.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[j:k + 1]
        k += 1


def test_the_kernels_take_the_packed_map_from_the_header():
    h2c = open(os.path.join(ROOT, "agogo_amd", "csrc", "conv_wino_h2c.hpp")).read()
    h2 = open(os.path.join(ROOT, "agogo_amd", "csrc", "conv_wino_h2.hpp")).read()
    gemm = _body(h2c, "wino_gemm_h2g_kernel")
    assert "maps::pack_tile" in gemm and "maps::pack_grid_tiles" in gemm
    assert "a_on" not in gemm and "k_loop" not in gemm          # every launched tile is a full one: one K loop
    oip = _body(h2c, "wino_oip_h2c_kernel")
    for fn in ("maps::pack_group_rg0", "maps::pack_group_slot0", "maps::pack_q"):
        assert fn in oip, fn
    assert "maps::pack_slot_row" in _body(h2c, "wino_oi_h2c_kernel")
    assert "maps::pack_slot_row" in _body(h2, "wino_in_h2_kernel")
    assert "maps::pack_grid(" in h2c and "maps::pack_pos_used" in h2c
