// CPU check of the short-position row map of the chained Winograd tower (agogo_amd/csrc/gemm_maps.hpp, the header the kernels
// include): built with g++ and run by tests/test_wino_dead_rows_cpu.py.
#include <cstdio>
#include <set>
#include <vector>

#include "../../agogo_amd/csrc/gemm_maps.hpp"

using namespace agz::maps;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_shape(int H, int W, int TM, int want_live, int want_stored) {
  const WinoRows g = wino_rows(H, W, TM);
  CHECK(g.AL == TM + 2 && g.TPB == g.nty * g.ntx && g.bpt * g.TPB == 128, "%dx%d/%d geometry", H, W, TM);
  CHECK(g.dead_y == (TM * g.nty > H) && g.dead_x == (TM * g.ntx > W), "%dx%d/%d dead flags", H, W, TM);
  CHECK(g.dead_y && g.dead_x, "%dx%d/%d: both edges ragged in this test", H, W, TM);
  CHECK(rows_short_ok(g), "%dx%d/%d qualifies", H, W, TM);
  CHECK(rows_slot_live(g, ROWS_R) == want_live && rows_slot_live(g, ROWS_C) == want_live, "%dx%d/%d live %d %d", H, W, TM,
        rows_slot_live(g, ROWS_R), rows_slot_live(g, ROWS_C));
  CHECK(rows_stored_per_board(g) == want_stored, "%dx%d/%d stored rows per board %d", H, W, TM, rows_stored_per_board(g));
  const int bpg = 16 / g.TPB;   // boards per 16-tile group of the out->in kernels
  int stored = 0;
  for (int xi = 0; xi < g.AL; xi++)
    for (int nu = 0; nu < g.AL; nu++) {
      const int cls = rows_class(g.dead_y, g.dead_x, g.AL, xi, nu);
      CHECK(cls == (xi == g.AL - 1 ? ROWS_R : (nu == g.AL - 1 ? ROWS_C : ROWS_FULL)), "class of (%d, %d)", xi, nu);
      const int live = rows_slot_live(g, cls), per = rows_per_board(cls, g.nty, g.ntx);
      CHECK(rows_pos_live(rows_slot_live(g, ROWS_R), rows_slot_live(g, ROWS_C), g.AL, xi * g.AL + nu) == live, "rows_pos_live (%d, %d)", xi, nu);
      CHECK(live == (cls == ROWS_FULL ? 128 : want_live), "live rows of (%d, %d): %d", xi, nu, live);
      stored += per;
      std::set<int> seen;
      for (int t = 0; t < 128; t++) {   // tile t of the slot: board t / TPB, tile (ty, tx)
        const int bs = t / g.TPB, tt = t % g.TPB, ty = tt / g.ntx, tx = tt % g.ntx;
        const bool dead = (cls == ROWS_R && ty == g.nty - 1) || (cls == ROWS_C && tx == g.ntx - 1);
        const int r = rows_row(cls, g.nty, g.ntx, bs, ty, tx);
        if (dead) { CHECK(r == -1, "dead tile got row %d", r); continue; }
        CHECK(r >= 0 && r < live, "(%d, %d) tile %d: row %d of %d", xi, nu, t, r, live);
        CHECK(seen.insert(r).second, "(%d, %d) tile %d: row %d twice", xi, nu, t, r);
        if (cls == ROWS_FULL) CHECK(r == t, "full position: row %d of tile %d", r, t);
        // the out->in kernels split the slot's board into (group of 16 tiles, board of the group): the same row
        const int grp = t / 16, bl = (t % 16) / g.TPB;
        CHECK(grp * bpg * per + rows_row(cls, g.nty, g.ntx, bl, ty, tx) == r, "group split of tile %d", t);
      }
      CHECK((int)seen.size() == live, "(%d, %d): %d rows used of %d", xi, nu, (int)seen.size(), live);
      // a wave of the pipelined out->in kernel = four consecutive tiles: its live rows are consecutive (class C: one run per wave;
      // store 0 = tiles 0, 1 of the wave, store 1 = tiles 2, 3)
      for (int w = 0; w < 32; w++) {
        int prev = -1;
        for (int k = 0; k < 4; k++) {
          const int t = 4 * w + k, bs = t / g.TPB, tt = t % g.TPB;
          const int r = rows_row(cls, g.nty, g.ntx, bs, tt / g.ntx, tt % g.ntx);
          if (r < 0) continue;
          CHECK(prev < 0 || r == prev + 1, "(%d, %d) wave %d: rows %d, %d not consecutive", xi, nu, w, prev, r);
          prev = r;
        }
      }
      // the GEMM: every live row lies in a 32-row block that is fetched (wave w's part) and multiplied (block (wm, i)); none past it is
      for (int r = 0; r < 128; r++) {
        const int w = r / 32, wm = r / 64, i = (r % 64) / 32;
        CHECK((h2c_wave_row0(w, 128) < live) == (r < live), "DMA block of row %d at live %d", r, live);
        CHECK((h2c_mfma_row0(wm, i) < live) == (r < live), "MFMA block of row %d at live %d", r, live);
      }
      // ... and these block origins are the ones the DMA and the fragment reads address: wave w's part of a stage starts at the image
      // bytes of row h2c_wave_row0 (its instructions cover the 32 rows from there), block (wm, i)'s fragment reads stay inside rows
      // h2c_mfma_row0 .. + 31 of the image
      for (int w = 0; w < 4; w++) {
        CHECK(h2c_wave_part(w, 128) == (unsigned)h2c_wave_row0(w, 128) * 128u, "wave %d part", w);
        for (int j = 0; j < h2c_wave_instrs(128); j++)
          for (int l = 0; l < 64; l++) {
            const unsigned src = h2c_wave_part(w, 128) + h2c_dma_src(l, j), dst = h2c_wave_part(w, 128) + h2c_dma_dst(l, j);
            CHECK((int)(src / 128) >= h2c_wave_row0(w, 128) && (int)(src / 128) < h2c_wave_row0(w, 128) + 32, "wave %d DMA source row %u", w, src / 128);
            CHECK((int)(dst / 128) >= h2c_wave_row0(w, 128) && (int)(dst / 128) < h2c_wave_row0(w, 128) + 32, "wave %d DMA image row %u", w, dst / 128);
          }
      }
      for (int wm = 0; wm < 2; wm++)
        for (int i = 0; i < 2; i++)
          for (int l = 0; l < 64; l++)
            for (int piece = 0; piece < 2; piece++)
              for (int ks = 0; ks < 2; ks++) {
                const int row = (int)(h2c_frag(h2c_mfma_row0(wm, i), l, piece, ks) / 128);
                CHECK(row == h2c_mfma_row0(wm, i) + (l & 31), "fragment row %d of block (%d, %d) lane %d", row, wm, i, l);
              }
    }
  CHECK(stored == want_stored, "stored rows per board %d", stored);
}

int main() {
  check_shape(19, 19, 5, 96, 732);
  check_shape(9, 9, 5, 64, 36 * 4 + 13 * 2);
  check_shape(7, 7, 4, 64, 25 * 4 + 11 * 2);
  check_shape(6, 7, 4, 64, 25 * 4 + 11 * 2);
  // shapes that keep every row: nothing hangs over the edge; a board that does not divide the 128-row slot; live counts off the 32-row grid
  CHECK(!rows_short_ok(wino_rows(5, 5, 5)), "5x5/5");
  CHECK(!rows_short_ok(wino_rows(13, 13, 5)), "13x13/5");
  CHECK(!rows_short_ok(wino_rows(3, 4, 5)), "3x4/5 (one tile per board: no live row left)");
  {   // one ragged edge only (4x7 / F(4x4): the columns): class C at nu == AL - 1 except the corner, which keeps every row
    const WinoRows g = wino_rows(4, 7, 4);
    CHECK(!g.dead_y && g.dead_x && rows_short_ok(g) && rows_slot_live(g, ROWS_C) == 64, "4x7/4");
    for (int xi = 0; xi < g.AL; xi++)
      for (int nu = 0; nu < g.AL; nu++) {
        const int cls = rows_class(g.dead_y, g.dead_x, g.AL, xi, nu), want = (nu == g.AL - 1 && xi != g.AL - 1) ? ROWS_C : ROWS_FULL;
        CHECK(cls == want, "4x7/4 class of (%d, %d): %d", xi, nu, cls);
        CHECK(rows_pos_live(0, 64, g.AL, xi * g.AL + nu) == (want == ROWS_C ? 64 : 128), "4x7/4 live rows of (%d, %d)", xi, nu);
        // what the out->in kernels compile in (both classes assumed, the absent one mapped to the full layout) is the same class
        const int cc = rows_class(true, true, g.AL, xi, nu);
        CHECK((cc == ROWS_R ? ROWS_FULL : cc) == want, "4x7/4 compiled class of (%d, %d)", xi, nu);
      }
    CHECK(rows_stored_per_board(g) == 31 * 2 + 5 * 1, "4x7/4 stored rows %d", rows_stored_per_board(g));
  }
  CHECK(rows_live_ok(32) && rows_live_ok(64) && rows_live_ok(96) && !rows_live_ok(0) && !rows_live_ok(128) && !rows_live_ok(48), "live counts");
  CHECK(rows_pos_live(0, 0, 7, 48) == 128 && rows_pos_live(96, 0, 7, 6) == 128 && rows_pos_live(0, 64, 7, 48) == 128 && rows_pos_live(96, 96, 7, 6) == 96 && rows_pos_live(96, 64, 7, 48) == 96, "rows_pos_live");
  if (fails) { printf("WINO_ROWS FAILED (%d)\n", fails); return 1; }
  printf("WINO_ROWS OK\n");
  return 0;
}
