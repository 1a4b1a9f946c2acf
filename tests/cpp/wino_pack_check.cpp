// CPU check of the packed short-position map of the chained Winograd tower (agogo_amd/csrc/gemm_maps.hpp "packed short positions", the
// header the kernels include): built with g++ and run by tests/test_wino_packed_rows_cpu.py.
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "../../agogo_amd/csrc/gemm_maps.hpp"

using namespace agz::maps;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

// one shape at one board count: every class's (board, live tile) -> (slot, row), the out->in kernels' per-group form of it, the GEMM grid
static void check(int H, int W, int TM, int B) {
  const WinoRows g = wino_rows(H, W, TM);
  CHECK(rows_short_ok(g), "%dx%d/%d qualifies", H, W, TM);
  const int live_r = g.dead_y ? rows_slot_live(g, ROWS_R) : 0, live_c = g.dead_x ? rows_slot_live(g, ROWS_C) : 0;
  const int n_mtiles = (B * g.TPB + 127) / 128, bpg = 16 / g.TPB, n_groups = (B * g.TPB + 15) / 16;
  std::map<int, std::set<int>> used;                       // position -> physical slots that hold a row
  for (int xi = 0; xi < g.AL; xi++)
    for (int nu = 0; nu < g.AL; nu++) {
      const int pos = xi * g.AL + nu, cls = rows_class(g.dead_y, g.dead_x, g.AL, xi, nu);
      const int live = rows_slot_live(g, cls), l = rows_per_board(cls, g.nty, g.ntx);
      const int S = cls == ROWS_FULL ? 1 : pack_slots(live), per = cls == ROWS_FULL ? 1 : pack_used_per_group(live);
      CHECK(S == 128 / gcd(128, live), "S of live %d: %d", live, S);
      CHECK(per * 128 == S * live, "live %d: %d slots of %d hold %d rows", live, per, S, S * live);
      std::set<int> seen;
      for (int b = 0; b < B; b++)
        for (int tt = 0; tt < g.TPB; tt++) {
          const int ty = tt / g.ntx, tx = tt % g.ntx, idx = rows_local(cls, g.nty, g.ntx, ty, tx);
          const bool dead = (cls == ROWS_R && ty == g.nty - 1) || (cls == ROWS_C && tx == g.ntx - 1);
          CHECK((idx < 0) == dead, "rows_local and the dead rule, (%d, %d) tile (%d, %d)", xi, nu, ty, tx);
          if (idx < 0) continue;
          const int p = pack_slot_row(S, g.bpt, l, b, idx), slot = p >> 7, grp = b / (S * g.bpt);
          CHECK(seen.insert(p).second, "(%d, %d) board %d tile %d: slot %d row %d twice", xi, nu, b, tt, slot, p & 127);
          CHECK(slot >= grp * S && slot < grp * S + per, "(%d, %d) board %d: slot %d outside the group's first %d", xi, nu, b, slot, per);
          CHECK(slot < n_mtiles, "(%d, %d) board %d: slot %d of %d allocated", xi, nu, b, slot, n_mtiles);
          if (cls == ROWS_FULL) CHECK(p == b * g.TPB + tt, "full position: board %d tile %d at %d", b, tt, p);
          used[pos].insert(slot);
          // the out->in kernels: group gi of 16 tile rows, board bl of the group; off = what the thread holds (row inside the group's
          // rows * row bytes + the lane's bytes inside the row), the rest is uniform or recomputed at the use
          const int gi = b / bpg, bl = b % bpg, gr = bpg * l, rin = rows_row(cls, g.nty, g.ntx, bl, ty, tx);
          for (int sh = 7; sh <= 8; sh++) {                  // V2c rows of 128 bytes, Mc rows of 256
            const unsigned long long rb = 1ull << sh, slot_stride = 1000003ull * 128 * rb;   // (any stride: a multiple of a slot's rows)
            for (unsigned lane_b = 0; lane_b < rb; lane_b += (unsigned)rb - 4) {
              const unsigned off = (unsigned)rin * (unsigned)rb + lane_b, rg0 = pack_group_rg0(S, gi, gr);
              const unsigned long long addr = pack_group_slot0(S, gi) * slot_stride + rg0 * rb + off + pack_q(S, rg0, off, sh) * (slot_stride - 128 * rb);
              CHECK(addr == slot * slot_stride + (unsigned long long)(p & 127) * rb + lane_b, "(%d, %d) board %d tile %d: group form", xi, nu, b, tt);
            }
          }
        }
      CHECK((int)seen.size() == B * l, "(%d, %d): %d rows of %d", xi, nu, (int)seen.size(), B * l);
      CHECK((int)used[pos].size() == pack_used_slots(S, g.bpt, l, B), "(%d, %d): %d slots used, pack_used_slots %d", xi, nu, (int)used[pos].size(),
            pack_used_slots(S, g.bpt, l, B));
      // rows are dense: every used slot but a group's last is full (only the tail's last slot may be partly filled)
      for (int s : used[pos]) {
        int n = 0;
        for (int p : seen) n += (p >> 7) == s;
        const bool tail_last = s == *used[pos].rbegin();
        CHECK(n == 128 || tail_last, "(%d, %d): slot %d holds %d rows", xi, nu, s, n);
      }
      // a dead lane (offset 2^31) stays out of range: q < S whatever the group
      for (int gi = 0; gi < n_groups; gi++) CHECK(pack_q(S, pack_group_rg0(S, gi, bpg * l), 0x80000000u, 7) < (unsigned)S && pack_q(S, pack_group_rg0(S, gi, bpg * l), 0x80000000u, 8) < (unsigned)S, "dead lane q");
    }
  // the GEMM grid: every (position, used slot, column tile) once, nothing else, position-major
  for (int n_nt = 1; n_nt <= 2; n_nt++) {
    const PackGrid pg = pack_grid(g.AL, g.nty, g.ntx, B, n_nt, live_r, live_c);
    CHECK(pg.u_full == n_mtiles, "u_full %d", pg.u_full);
    int want = 0;
    for (int pos = 0; pos < g.AL * g.AL; pos++) {
      CHECK(pack_pos_used(pg, pos) == (int)used[pos].size(), "pack_pos_used(%d) = %d, %d slots hold rows", pos, pack_pos_used(pg, pos), (int)used[pos].size());
      want += (int)used[pos].size() * n_nt;
    }
    CHECK(pack_grid_tiles(pg) == want, "B %d: %d workgroups, want %d", B, pack_grid_tiles(pg), want);
    std::set<std::tuple<int, int, int>> tiles;
    int prev_pos = 0;
    for (int t = 0; t < pack_grid_tiles(pg); t++) {
      const PackTile pt = pack_tile(pg, t);
      CHECK(pt.pos >= prev_pos && pt.pos < g.AL * g.AL && pt.n_tile >= 0 && pt.n_tile < n_nt, "tile %d: pos %d n_tile %d", t, pt.pos, pt.n_tile);
      prev_pos = pt.pos;
      CHECK(used[pt.pos].count(pt.slot) == 1, "tile %d: (pos %d, slot %d) holds no row", t, pt.pos, pt.slot);
      CHECK(tiles.insert(std::make_tuple(pt.pos, pt.slot, pt.n_tile)).second, "tile %d: (pos %d, slot %d, n_tile %d) twice", t, pt.pos, pt.slot, pt.n_tile);
    }
    CHECK((int)tiles.size() == want, "%d distinct tiles of %d", (int)tiles.size(), want);
    // the map off (every row kept): the old grid
    const PackGrid off = pack_grid(g.AL, g.nty, g.ntx, B, n_nt, 0, 0);
    CHECK(pack_grid_tiles(off) == g.AL * g.AL * n_mtiles * n_nt, "keep-all grid");
    for (int t = 0; t < pack_grid_tiles(off); t++) {
      const PackTile pt = pack_tile(off, t);
      CHECK(pt.pos == t / (n_mtiles * n_nt) && pt.slot == t / n_nt % n_mtiles && pt.n_tile == t % n_nt, "keep-all tile %d", t);
    }
  }
}

static void check_counts(int H, int W, int TM) {
  const WinoRows g = wino_rows(H, W, TM);
  const int S = pack_slots(g.dead_y ? rows_slot_live(g, ROWS_R) : rows_slot_live(g, ROWS_C)), gb = S * g.bpt;
  const int counts[] = {1, g.bpt, gb - 1, gb, gb + 1, 3 * gb + g.bpt + 1};
  for (int B : counts) check(H, W, TM, B);
}

int main() {
  check_counts(19, 19, 5);
  check_counts(9, 9, 5);
  check_counts(7, 7, 4);
  check_counts(4, 7, 4);                                     // class C alone
  {   // 19x19: 96 live rows, groups of 4 slots / 32 boards; boards 10 and 21 of a group straddle two slots; 512 boards: 416 of 6272 workgroups go
    const WinoRows g = wino_rows(19, 19, 5);
    CHECK(pack_slots(96) == 4 && pack_slots(64) == 2 && pack_slots(32) == 4 && pack_slots(0) == 1 && pack_slots(128) == 1, "pack_slots");
    for (int b = 0; b < 32; b++) {
      const int first = pack_slot_row(4, g.bpt, 12, 32 + b, 0) >> 7, last = pack_slot_row(4, g.bpt, 12, 32 + b, 11) >> 7;
      CHECK((first != last) == (b == 10 || b == 21), "board %d of a group: slots %d .. %d", b, first, last);
    }
    const PackGrid pg = pack_grid(7, 4, 4, 512, 2, 96, 96), off = pack_grid(7, 4, 4, 512, 2, 0, 0);
    CHECK(pack_grid_tiles(off) == 6272 && pack_grid_tiles(off) - pack_grid_tiles(pg) == 416, "512 boards: %d of %d", pack_grid_tiles(pg), pack_grid_tiles(off));
  }
  if (fails) { printf("WINO_PACK FAILED (%d)\n", fails); return 1; }
  printf("WINO_PACK OK\n");
  return 0;
}
