// CPU check of agogo_amd/csrc/conv_maps.hpp — the address arithmetic of the trainer's nine-tap DMA forward convolution (train.hip:
// k_conv_h2dma3).  Built with g++ and run by tests/test_conv_maps_cpu.py.  The kernel's data movement is replayed with the header's
// functions on tagged planes (every 16-byte unit of the activation tensor carries its own (padded pixel, unit) tag): the x image is
// landed instruction by instruction as the kernel issues it, then every MFMA A-fragment read of every output pixel, tap and k half must
// fetch exactly the unit the convolution's definition names — y[m] += w[ky][kx] . x[pixel(m) + (ky - 1) Wp + (kx - 1)] — for whole tiles,
// a tile crossing a board, and the partial last tile; the image must fit CD3_IMG rows where the launcher says it does; and the
// fragment reads' bank spread is reported per lane group.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../../agogo_amd/csrc/conv_maps.hpp"

using namespace agz::cmaps;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL %s:%d: %s — ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } fails++; } } while (0)

// lane groups a ds_read_b128 is served in (MI355X_MICROARCH.md, LDS section)
static const int GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                  {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

struct Geo { int B, H, W, HW, Hp, Wp, M; };
static Geo geo(int B, int H, int W) { return Geo{B, H, W, H * W, H + 2, W + 2, B * H * W}; }

static int max_rows(const Geo& g) {
  int mx = 0;
  for (int m0 = 0; m0 < g.M; m0 += 256)
    mx = std::max(mx, cd3_rows(pix(m0, g.HW, g.W, g.Hp, g.Wp), pix(std::min(m0 + 255, g.M - 1), g.HW, g.W, g.Hp, g.Wp), g.Wp));
  return mx;
}

static long worst_conflict = 1, reads_checked = 0;

static void check_tile(const Geo& g, int m_tile) {
  const int m0 = m_tile * 256;
  const size_t pix0 = pix(m0, g.HW, g.W, g.Hp, g.Wp);
  const int pb = cd3_base(pix0, g.Wp);
  const long n_pix = (long)g.B * g.Hp * g.Wp;
  CHECK(pb >= 0, "tile %d: image row 0 before the tensor", m_tile);
  // land the image of one chunk: lds[byte / 16] = (padded pixel, unit of the chunk); the kernel: instruction j of wave j % 4, lanes off where row >= CD3_IMG
  std::map<unsigned, std::pair<long, int>> lds;
  for (int j = 0; j < CD3_INSTR; j++)
    for (int lane = 0; lane < 64; lane++) {
      const int row = dma_row(lane, j);
      if (row >= CD3_IMG) continue;
      const unsigned dst = dma_dst(lane, j);            // (the hardware adds 16 * lane to the instruction's base dma_dst(0, j))
      CHECK(dst == dma_dst(0, j) + 16u * lane, "lane-linear landing");
      CHECK(dst / 64 == (unsigned)row, "instruction %d lane %d lands in row %u, not %d", j, lane, dst / 64, row);
      CHECK(!lds.count(dst / 16), "LDS unit %u written twice", dst / 16);
      const long p = pb + row;                          // source: plane byte (pb + row) * Cin * 2 + chunk * 64 + dma_src_unit(lane)
      lds[dst / 16] = {p < n_pix ? p : -1, (int)(dma_src_unit(lane) >> 4)};
      CHECK(dma_src_unit(lane) % 16 == 0 && dma_src_unit(lane) < 64, "source unit");
    }
  CHECK((int)lds.size() == CD3_IMG * 4, "%zu units landed", lds.size());
  for (auto& kv : lds) {
    const int row = (int)(kv.first * 16 / 64);
    CHECK(kv.first * 16 == lds_off(row, kv.second.second), "unit %d of row %d is at byte %u", kv.second.second, row, kv.first * 16);
  }
  int max_row_read = -1;
  // every fragment read: 4 waves = (wm, wn); wave's row blocks i = 0..3 -> output pixels m0 + (wm * 4 + i) * 32 + (lane & 31)
  for (int wm = 0; wm < 2; wm++)
    for (int i = 0; i < 4; i++)
      for (int tap = 0; tap < 9; tap++) {
        const int ky = tap / 3, kx = tap % 3;
        for (int ks = 0; ks < 2; ks++) {
          unsigned addr[64];
          bool real[64];
          for (int lane = 0; lane < 64; lane++) {
            int m = m0 + (wm * 4 + i) * 32 + (lane & 31);
            real[lane] = m < g.M;
            if (m >= g.M) m = g.M - 1;                   // (the kernel clamps; such rows are not stored)
            const size_t pm = pix(m, g.HW, g.W, g.Hp, g.Wp);
            const int row = cd3_row0(pm, pix0) + cd3_tap(ky, kx, g.Wp);
            CHECK(row >= 0 && row < CD3_IMG, "tile %d pixel %d tap %d: image row %d", m_tile, m, tap, row);
            max_row_read = std::max(max_row_read, row);
            const int kh = lane >> 5;
            addr[lane] = lds_off(row, 2 * ks + kh);
            CHECK(lds.count(addr[lane] / 16), "fragment address %u not landed", addr[lane]);
            auto pu = lds[addr[lane] / 16];
            const long want = (long)pm + (long)(ky - 1) * g.Wp + (kx - 1);
            CHECK(pu.first == want, "tile %d pixel %d tap (%d,%d): read padded pixel %ld, the convolution needs %ld", m_tile, m, ky, kx, pu.first, want);
            CHECK(pu.second == 2 * ks + kh, "tile %d lane %d ks %d: unit %d", m_tile, lane, ks, pu.second);
            // the neighbour is a pixel of the SAME board (interior or halo): never another board's interior
            const long b_of = want / ((long)g.Hp * g.Wp), b_m = (long)pm / ((long)g.Hp * g.Wp);
            CHECK(b_of == b_m, "tile %d pixel %d tap %d leaves its board", m_tile, m, tap);
          }
          for (int gq = 0; gq < 4; gq++) {              // bank spread of the lanes served together (16 bytes = four banks; 64 banks)
            std::map<unsigned, int> slot;
            for (int q = 0; q < 16; q++) { const int lane = GROUPS[gq][q]; if (real[lane]) slot[(addr[lane] / 16) % 16]++; }
            for (auto& kv : slot) worst_conflict = std::max<long>(worst_conflict, kv.second);
            reads_checked++;
          }
        }
      }
  // the launcher's fit rule counts exactly the rows the tile reads
  const int rows = cd3_rows(pix0, pix(std::min(m0 + 255, g.M - 1), g.HW, g.W, g.Hp, g.Wp), g.Wp);
  CHECK(max_row_read + 1 == rows, "tile %d reads rows 0..%d, cd3_rows says %d", m_tile, max_row_read, rows);
}

int main() {
  // the geometries the trainer runs the kernel on (19x19) and the launcher's fit rule
  const Geo g19 = geo(3, 19, 19), gbig = geo(256, 19, 19);
  CHECK(max_rows(g19) <= CD3_IMG && max_rows(gbig) <= CD3_IMG, "19x19 needs %d / %d rows", max_rows(g19), max_rows(gbig));
  CHECK(max_rows(gbig) >= CD3_IMG - 16, "CD3_IMG %d is far above what 19x19 needs (%d): LDS wasted", CD3_IMG, max_rows(gbig));
  CHECK(max_rows(geo(5, 25, 25)) > CD3_IMG, "25x25 should not fit");
  for (int t = 0; t * 256 < g19.M; t++) check_tile(g19, t);              // 1083 rows: whole tiles, board crossings, a partial tile
  for (int t : {0, 1, 180, 359, 360}) check_tile(gbig, t);
  const Geo g1617 = geo(4, 16, 17);                                       // another board >= 16 wide that fits
  if (max_rows(g1617) <= CD3_IMG) for (int t = 0; t * 256 < g1617.M; t++) check_tile(g1617, t);
  // the wide boards tests/test_train_wide_gpu.py runs the kernel on, every tile (geo(B, H, W): boards, height, width):
  // 16x16 (HW = 256: every tile is one board) at B = 1 and 3; 16 wide x 17 high and its transpose; 20 wide x 16 high at B = 2, whose image needs
  // exactly the limit; 21 wide x 16 high at B = 1 (one board: no crossing, fits); 16 wide x 9 high at B = 3 (two board crossings inside one tile)
  const Geo wide[] = {geo(1, 16, 16), geo(3, 16, 16), geo(2, 17, 16), geo(2, 16, 17), geo(2, 16, 20), geo(1, 16, 21), geo(3, 9, 16)};
  for (const Geo& g : wide) {
    CHECK(max_rows(g) <= CD3_IMG, "%d boards of %d wide x %d high need %d rows", g.B, g.W, g.H, max_rows(g));
    for (int t = 0; t * 256 < g.M; t++) check_tile(g, t);
  }
  CHECK(max_rows(geo(2, 16, 20)) == CD3_IMG, "20 wide x 16 high, B = 2 needs %d rows, not exactly the limit", max_rows(geo(2, 16, 20)));
  CHECK(max_rows(geo(3, 9, 16)) == 360, "16 wide x 9 high, B = 3 needs %d rows", max_rows(geo(3, 9, 16)));
  // ... and the ones the launcher must keep on k_conv_h2dma: the same 21-wide board at B = 2, the short boards at B = 5
  CHECK(max_rows(geo(2, 16, 21)) > CD3_IMG, "21 wide x 16 high, B = 2 fits (%d rows)", max_rows(geo(2, 16, 21)));
  CHECK(max_rows(geo(5, 9, 16)) > CD3_IMG, "16 wide x 9 high, B = 5 fits (%d rows)", max_rows(geo(5, 9, 16)));
  CHECK(max_rows(geo(5, 3, 16)) > CD3_IMG, "16 wide x 3 high, B = 5 fits (%d rows)", max_rows(geo(5, 3, 16)));
  // k_conv_h2dma's stage images use the same row / unit / swizzle functions: 16 distinct bank slots for 16 consecutive rows, any alignment
  for (int r0 = 0; r0 < 8; r0++)
    for (int u = 0; u < 4; u++) {
      std::set<unsigned> s;
      for (int r = r0; r < r0 + 16; r++) s.insert((lds_off(r, u) / 16) % 16);
      CHECK(s.size() == 16, "rows %d..: %zu slots", r0, s.size());
    }
  printf("fragment read groups checked: %ld, worst same-slot count inside a lane group: %ld\n", reads_checked, worst_conflict);
  CHECK(worst_conflict <= 2, "a lane group reads one bank slot %ld times", worst_conflict);
  if (fails) { printf("%d failures\n", fails); return 1; }
  printf("CONV_MAPS OK\n");
  return 0;
}
