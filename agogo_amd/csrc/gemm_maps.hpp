// Address arithmetic of the chained Winograd GEMMs (conv_wino_h2c.hpp: wino_gemm_h2g_kernel, wino_gemm_h2p_kernel), as plain
// constexpr functions that BOTH the kernels and a g++-built CPU test include (tests/cpp/gemm_maps_check.cpp, run by
// tests/test_gemm_maps_cpu.py): the kernels compute every DMA source offset, LDS fragment address, M store address and work-list
// index through these functions, so changing one of them — or a kernel's use of one — is seen by a test without a GPU.
//
// Layouts (conv_wino_h2c.hpp): a K step of a 128-row tile of V2c is one 16 KB chunk, row r = 128 bytes = eight 16-byte units
// (0..3: hi fp16 of k 0..31, 4..7: lo).  `buffer_load ... lds` writes LDS lane-linearly (lane l of an instruction -> base + 16 l),
// so the bank swizzle of the LDS image goes on the SOURCE offset.
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#define AGZ_MAPS_HD __host__ __device__
#else
#define AGZ_MAPS_HD
#endif

namespace agz {
namespace maps {

// LDS image of a staged chunk: row r, 16-byte unit q at r * 128 + ((q ^ ((r >> 1) & 7)) << 4)
AGZ_MAPS_HD constexpr unsigned h2c_img(int row, int unit) { return (unsigned)(row * 128 + ((unit ^ ((row >> 1) & 7)) << 4)); }

// DMA instruction j of a wave (8 rows x 8 units = 1 KB, rows 8 j .. 8 j + 7 of the wave's part): lane's SOURCE byte offset inside
// the wave's part of the chunk, and its (lane-linear) LDS destination.  (r >> 1) & 7 of row 8 j + lane / 8 (+ the wave's first row,
// a multiple of 16) is (4 j + lane / 16) & 7.
AGZ_MAPS_HD constexpr unsigned h2c_dma_src(int lane, int j) {
  return (unsigned)(j * 1024 + (lane >> 3) * 128 + (((lane & 7) ^ ((4 * j + (lane >> 4)) & 7)) << 4));
}
AGZ_MAPS_HD constexpr unsigned h2c_dma_dst(int lane, int j) { return (unsigned)(j * 1024 + lane * 16); }
// the four waves of a workgroup split a stage of stage_rows rows evenly: wave w owns rows w * stage_rows / 4 .. (bytes, source = image)
AGZ_MAPS_HD constexpr unsigned h2c_wave_part(int wid, int stage_rows) { return (unsigned)(wid * (stage_rows / 4) * 128); }
AGZ_MAPS_HD constexpr int h2c_wave_instrs(int stage_rows) { return stage_rows / 4 / 8; }

// MFMA 32x32x16 operand fragment of image rows row0 .. row0 + 31 (row0 a multiple of 32): lane l reads row row0 + (l & 31), the 16-byte
// unit piece * 4 + 2 ks + (l >> 5) — piece 0 = hi, 1 = lo; k = 16 ks + 8 (l >> 5) .. + 7 of the 32-channel step
AGZ_MAPS_HD constexpr unsigned h2c_frag(int row0, int lane, int piece, int ks) {
  return (unsigned)((row0 + (lane & 31)) * 128 + (((piece * 4 + 2 * ks + (lane >> 5)) ^ ((lane >> 1) & 7)) << 4));
}

// Accumulator register r (0..15) of a 32x32 MFMA result holds tile row mfma_row(r) in lanes 0..31 and mfma_row(r) + 4 in lanes 32..63
AGZ_MAPS_HD constexpr int mfma_row(int r) { return (r & 3) + 8 * (r >> 2); }

// Mc[T/128][pos][Ntot/64 slices][128 rows][64 cols] fp32: float index of (m_tile, pos, slice, row, col)
AGZ_MAPS_HD constexpr size_t mc_index(int m_tile, int npos, int pos, int n_slices, int slice, int row, int col) {
  return ((((size_t)m_tile * npos + pos) * (size_t)n_slices + (size_t)slice) * 128 + (size_t)row) * 64 + (size_t)col;
}

// the four waves of a workgroup: first row of wave w's part of a stage, and of the 32-row MFMA block i of the waves wm (64 rows each)
AGZ_MAPS_HD constexpr int h2c_wave_row0(int wid, int stage_rows) { return wid * (stage_rows / 4); }
AGZ_MAPS_HD constexpr int h2c_mfma_row0(int wm, int i) { return wm * 64 + i * 32; }

// ---- short positions (tests/cpp/wino_rows_check.cpp, tests/test_wino_dead_rows_cpu.py) --------------------------------------------
// F(TM x TM, 3x3) covers H pixels with nty = ceil(H / TM) tiles; where TM * nty > H the last output row of the last tile row lies
// off the board, and the last transform point (index AL - 1, the "infinity" point) feeds that output only.  So the V2c / GEMM / Mc
// row of (position (xi, nu), tile (ty, tx)) is dead — it reaches no kept pixel — when xi == AL - 1 and ty == nty - 1, and likewise
// with nu / tx for the columns.  A short position packs its live tiles into the first rows of its 128-row slot:
//   class R (dead_y, xi == AL - 1, every nu): live ty < nty - 1, local index tt,                    lr = TPB - ntx per board
//   class C (dead_x, nu == AL - 1, xi != AL - 1): live tx < ntx - 1, local index ty * (ntx - 1) + tx, lc = TPB - nty per board
// row in the slot = (b % bpt) * l + local index, bpt = 128 / TPB boards per slot; rows bpt * l .. 127 are neither written nor read.
// (At the corner class R keeps the tx == ntx - 1 rows although they are dead too: one rule per position.)
enum { ROWS_FULL = 0, ROWS_R = 1, ROWS_C = 2 };
struct WinoRows { int TM, AL, nty, ntx, TPB, bpt; bool dead_y, dead_x; };
AGZ_MAPS_HD constexpr WinoRows wino_rows(int H, int W, int TM) {
  const int nty = (H + TM - 1) / TM, ntx = (W + TM - 1) / TM;
  return WinoRows{TM, TM + 2, nty, ntx, nty * ntx, 128 / (nty * ntx), TM * nty > H, TM * ntx > W};
}
AGZ_MAPS_HD constexpr int rows_class(bool dead_y, bool dead_x, int AL, int xi, int nu) {
  return xi == AL - 1 ? (dead_y ? ROWS_R : ROWS_FULL) : ((dead_x && nu == AL - 1) ? ROWS_C : ROWS_FULL);   // (the corner is never class C)
}
// live tiles per board at a position of class cls
AGZ_MAPS_HD constexpr int rows_per_board(int cls, int nty, int ntx) {
  return cls == ROWS_R ? nty * ntx - ntx : (cls == ROWS_C ? nty * ntx - nty : nty * ntx);
}
// local index of tile (ty, tx) among its board's live tiles; -1: dead
AGZ_MAPS_HD constexpr int rows_local(int cls, int nty, int ntx, int ty, int tx) {
  return cls == ROWS_R ? (ty < nty - 1 ? ty * ntx + tx : -1) : (cls == ROWS_C ? (tx < ntx - 1 ? ty * (ntx - 1) + tx : -1) : ty * ntx + tx);
}
// row of (board bs = b % bpt of the slot, tile (ty, tx)) inside the 128-row slot; -1: dead
AGZ_MAPS_HD constexpr int rows_row(int cls, int nty, int ntx, int bs, int ty, int tx) {
  return rows_local(cls, nty, ntx, ty, tx) < 0 ? -1 : bs * rows_per_board(cls, nty, ntx) + rows_local(cls, nty, ntx, ty, tx);
}
// live rows of a slot at a position of class cls
AGZ_MAPS_HD constexpr int rows_slot_live(const WinoRows& g, int cls) { return g.bpt * rows_per_board(cls, g.nty, g.ntx); }
// the short map is taken when a class exists and every class that does leaves whole 32-row MFMA blocks: 32, 64 or 96 live rows
AGZ_MAPS_HD constexpr bool rows_live_ok(int live) { return live == 32 || live == 64 || live == 96; }
AGZ_MAPS_HD constexpr bool rows_short_ok(const WinoRows& g) {
  return 128 % g.TPB == 0 && (g.dead_y || g.dead_x) && (!g.dead_y || rows_live_ok(rows_slot_live(g, ROWS_R))) &&
         (!g.dead_x || rows_live_ok(rows_slot_live(g, ROWS_C)));
}
// what the GEMM needs: the live rows of position pos's slots (live_r / live_c: the two classes' counts, 0 = no such class)
AGZ_MAPS_HD constexpr int rows_pos_live(int live_r, int live_c, int AL, int pos) {
  return pos / AL == AL - 1 ? (live_r ? live_r : 128) : ((live_c && pos % AL == AL - 1) ? live_c : 128);
}
// stored rows per board over all positions
AGZ_MAPS_HD constexpr int rows_stored_per_board(const WinoRows& g) {
  int n = 0;
  for (int xi = 0; xi < g.AL; xi++)
    for (int nu = 0; nu < g.AL; nu++) n += rows_per_board(rows_class(g.dead_y, g.dead_x, g.AL, xi, nu), g.nty, g.ntx);
  return n;
}

// ---- packed short positions (tests/cpp/wino_pack_check.cpp, tests/test_wino_packed_rows_cpu.py) ------------------------------------
// Where the short map is on, a class with `live` rows per slot does not leave the last 128 - live rows of every slot empty: the live
// rows of S = 128 / gcd(128, live) consecutive slots (a packing group: S * bpt boards, S * live rows; 96 -> 4 slots, 64 -> 2, 32 -> 4)
// fill the group's first S * live / 128 slots COMPLETELY, and the group's remaining slots are neither written, read nor multiplied at
// that position.  Board b, live tile of local index idx (rows_local), l = rows_per_board live tiles per board:
//   rg = (b % (S * bpt)) * l + idx        physical slot (b / (S * bpt)) * S + (rg >> 7), row rg & 127
// (a board's rows may straddle two slots).  A partly filled last group uses ceil(rows / 128) slots; its rows past the last board are
// unwritten, the GEMM may multiply them and nothing reads the result.  A full position is the same map with S = 1, l = TPB.
AGZ_MAPS_HD constexpr int pack_slots(int live) { return live == 96 || live == 32 ? 4 : (live == 64 ? 2 : 1); }
AGZ_MAPS_HD constexpr int pack_used_per_group(int live) { return live == 96 ? 3 : 1; }                 // S * live / 128 (1 for a full position)
AGZ_MAPS_HD constexpr int pack_rg(int S, int bpt, int l, int b, int idx) { return (b % (S * bpt)) * l + idx; }
// physical slot * 128 + row of (board b, local index idx)
AGZ_MAPS_HD constexpr int pack_slot_row(int S, int bpt, int l, int b, int idx) { return (b / (S * bpt)) * S * 128 + pack_rg(S, bpt, l, b, idx); }
// slots that hold rows at a position of B boards
AGZ_MAPS_HD constexpr int pack_used_slots(int S, int bpt, int l, int B) {
  return (B / (S * bpt)) * (S * bpt * l / 128) + ((B % (S * bpt)) * l + 127) / 128;
}
// The out->in kernels work on groups of 16 tile rows (16 / TPB whole boards, gr = live rows of the group at the class; 8 S groups per
// packing group).  Group g's first packed row rg0 = (g % (8 S)) * gr is uniform, and with off = (row of the tile inside its group) *
// row_bytes + (the lane's bytes inside the row) — what the unpacked map held per thread — the packed address is
//   base(slot (g / (8 S)) * S) + rg0 * row_bytes + off + q * (slot_stride - 128 * row_bytes),   q = ((rg0 + off / row_bytes) >> 7) & (S - 1)
// (q = the slot of the group the row falls into).  A dead lane's off is 2^31: q stays below S, so its offset stays past the descriptor's range.
AGZ_MAPS_HD constexpr unsigned pack_group_rg0(int S, int g, int gr) { return (unsigned)((g & (8 * S - 1)) * gr); }
AGZ_MAPS_HD constexpr int pack_log2(int S) { return S >> 1; }                                           // S is 1, 2 or 4 (no division in a kernel)
AGZ_MAPS_HD constexpr unsigned pack_group_slot0(int S, int g) { return (unsigned)((g >> (3 + pack_log2(S))) << pack_log2(S)); }
AGZ_MAPS_HD constexpr unsigned pack_q(int S, unsigned rg0, unsigned off, int row_shift) { return ((rg0 + (off >> row_shift)) >> 7) & (unsigned)(S - 1); }
// GEMM grid: one workgroup per (position, USED slot, column tile), position-major as before.  per / S = 1 and u = u_full where a class
// is absent or the short map is off.
struct PackGrid { int AL, n_nt, u_full, u_r, u_c, S_r, S_c, per_r, per_c; };
AGZ_MAPS_HD constexpr PackGrid pack_grid(int AL, int nty, int ntx, int B, int n_nt, int live_r, int live_c) {
  const int TPB = nty * ntx, bpt = 128 / TPB, u_full = pack_used_slots(1, bpt, TPB, B);
  return PackGrid{AL, n_nt, u_full,
                  live_r ? pack_used_slots(pack_slots(live_r), bpt, rows_per_board(ROWS_R, nty, ntx), B) : u_full,
                  live_c ? pack_used_slots(pack_slots(live_c), bpt, rows_per_board(ROWS_C, nty, ntx), B) : u_full,
                  pack_slots(live_r), pack_slots(live_c), pack_used_per_group(live_r), pack_used_per_group(live_c)};
}
// used slots of position pos; workgroups of the launch
AGZ_MAPS_HD constexpr int pack_pos_used(const PackGrid& g, int pos) {
  return pos / g.AL == g.AL - 1 ? g.u_r : (pos % g.AL == g.AL - 1 ? g.u_c : g.u_full);
}
AGZ_MAPS_HD constexpr int pack_grid_tiles(const PackGrid& g) {
  return ((g.AL - 1) * ((g.AL - 1) * g.u_full + g.u_c) + g.AL * g.u_r) * g.n_nt;
}
struct PackTile { int pos, slot, n_tile; };
AGZ_MAPS_HD constexpr PackTile pack_tile(const PackGrid& g, int tile) {
  const int u = tile / g.n_nt, row_u = (g.AL - 1) * g.u_full + g.u_c;
  const int xi = u / row_u < g.AL - 1 ? u / row_u : g.AL - 1, r = u - xi * row_u;
  const bool last = xi == g.AL - 1;
  const int nu = last ? r / g.u_r : (r / g.u_full < g.AL - 1 ? r / g.u_full : g.AL - 1);
  const int k = r - nu * (last ? g.u_r : g.u_full);
  const int per = last ? g.per_r : (nu == g.AL - 1 ? g.per_c : 1), S = last ? g.S_r : (nu == g.AL - 1 ? g.S_c : 1);
  return PackTile{xi * g.AL + nu, (k / per) * S + k % per, tile - u * g.n_nt};
}

// ---- persistent kernel (wino_gemm_h2p_kernel): 8 KB stages of 64 rows, ring of 16, DMA 10 stages ahead
constexpr int H2P_D = 10, H2P_R = 16, H2P_NK = 8;
// byte offset in V2c of K step 0 of half tile hm (rows 64 (hm & 1) .. of m-tile hm >> 1) of position pos
AGZ_MAPS_HD constexpr unsigned h2p_v_base(int pos, int hm, int npos) {
  return (unsigned)(((hm >> 1) * npos + pos) * (H2P_NK * 16384) + (hm & 1) * 8192);
}
// tile parity PAR (ring half), K step kk: ring slot of the step's own stage, of the next step's stage, of the stage DMA'd at this step
AGZ_MAPS_HD constexpr int h2p_slot(int par, int kk) { return (par * H2P_NK + kk) % H2P_R; }
AGZ_MAPS_HD constexpr int h2p_slot_next(int par, int kk) { return (par * H2P_NK + kk + 1) % H2P_R; }
AGZ_MAPS_HD constexpr int h2p_slot_ahead(int par, int kk) { return (par * H2P_NK + kk + H2P_D) % H2P_R; }
AGZ_MAPS_HD constexpr int h2p_kk_ahead(int kk) { return (kk + H2P_D) % H2P_NK; }
AGZ_MAPS_HD constexpr int h2p_tiles_ahead(int kk) { return (kk + H2P_D) / H2P_NK; }      // 1 or 2
// counted waits (s_waitcnt vmcnt): operations a wave issues per K step = 2 DMA + 4 M stores; "stage g + 1 has landed" when at most
// this many younger operations are outstanding — steady state: the 4 stores of the issuing step + (D - 2) whole steps; while no
// stores are in flight yet (first pair of tiles): the DMAs of D - 2 stages
AGZ_MAPS_HD constexpr int h2p_wait_steady() { return 4 + (H2P_D - 2) * 6; }
AGZ_MAPS_HD constexpr int h2p_wait_early() { return (H2P_D - 2) * 2; }
AGZ_MAPS_HD constexpr bool h2p_early(int t) { return t < 2; }                        // tiles whose waits use the early count
// work list: workgroup id -> (team, slab); team t of nteams walks units [u0, u0 + nT) of U2 = npos x n_mtiles PAIRS of half tiles
struct H2pTeam { int team, slab, nteams; bool idle; };
AGZ_MAPS_HD constexpr H2pTeam h2p_team(int block, int grid, int n_slabs) {
  const int xcd = block & 7, slot = block >> 3, tpx = (grid >> 3) / n_slabs;
  return H2pTeam{xcd * tpx + (tpx ? slot / n_slabs : 0), tpx ? slot % n_slabs : 0, 8 * tpx, slot >= tpx * n_slabs};
}
AGZ_MAPS_HD constexpr int h2p_u0(int team, int nteams, int U2) { return 2 * (int)((long)team * U2 / nteams); }

}  // namespace maps
}  // namespace agz
