// Plain g++ check of agogo_amd/csrc/sym.hpp (no HIP): the eight board symmetries and the leaf-symmetry key, on the code the kernels
// compile.  Driven by tests/test_sym_cpu.py.  For m = 4, 5, 19:
//   every src_k is a bijection; dst_k o src_k = id; inv is right; the eight maps are distinct and closed under composition;
//   S_0..S_3 equal the rotation augmenter's rot_src (restated below from RotateBoard, encoding_helper.go:92-103);
//   S_k = R^(k&3) o T^(k>>2), applied to a board generator by generator.
// Then it prints `key <seed> <to_move> <k>` for boards it draws from a fixed LCG, which the Python test recomputes.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../agogo_amd/csrc/sym.hpp"

using namespace agz;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the rotation augmenter's source index as it stood before sym.hpp (RotateBoard composed q times)
static int rot_src(int i, int j, int m, int q) {
  switch (q & 3) {
    case 0: return i * m + j;
    case 1: return j * m + (m - 1 - i);
    case 2: return (m - 1 - i) * m + (m - 1 - j);
    default: return (m - 1 - j) * m + i;
  }
}

using Board = std::vector<int>;
static Board apply_R(const Board& x, int m) {   // (R x)[i][j] = x[j][m-1-i]
  Board y(x.size());
  for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) y[i * m + j] = x[j * m + (m - 1 - i)];
  return y;
}
static Board apply_T(const Board& x, int m) {   // (T x)[i][j] = x[j][i]
  Board y(x.size());
  for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) y[i * m + j] = x[j * m + i];
  return y;
}
static Board apply_S(const Board& x, int m, int k) {   // through the index map under test
  Board y(x.size());
  for (int c = 0; c < m * m; c++) y[c] = x[sym::src(m, k, c)];
  return y;
}

static void check_m(int m) {
  const int mm = m * m;
  Board x(mm);
  for (int c = 0; c < mm; c++) x[c] = c;   // a board with no symmetry of its own: S_k x IS the map src_k
  std::set<Board> images;
  for (int k = 0; k < 8; k++) {
    std::vector<int> hit(mm, 0);
    for (int c = 0; c < mm; c++) {
      const int s = sym::src(m, k, c);
      CHECK(s >= 0 && s < mm, "m %d k %d: src(%d) = %d out of range", m, k, c, s);
      if (s >= 0 && s < mm) hit[s]++;
      CHECK(sym::src(m, k, c) == sym::src_ij(m, k, c / m, c % m), "m %d k %d: src and src_ij differ at %d", m, k, c);
      CHECK(sym::dst(m, k, sym::src(m, k, c)) == c, "m %d k %d: dst(src(%d)) != %d", m, k, c, c);
      CHECK(sym::src(m, k, sym::dst(m, k, c)) == c, "m %d k %d: src(dst(%d)) != %d", m, k, c, c);
      if (k < 4) CHECK(s == rot_src(c / m, c % m, m, k), "m %d k %d: not the rotation augmenter's image at %d", m, k, c);
    }
    for (int c = 0; c < mm; c++) CHECK(hit[c] == 1, "m %d k %d: cell %d is the source of %d cells", m, k, c, hit[c]);
    // the definition, generator by generator: T first when k >= 4, then R (k&3) times
    Board want = x;
    if (k >> 2) want = apply_T(want, m);
    for (int r = 0; r < (k & 3); r++) want = apply_R(want, m);
    CHECK(apply_S(x, m, k) == want, "m %d k %d: S_k is not R^%d o T^%d", m, k, k & 3, k >> 2);
    // inv
    const int ik = sym::inv(k);
    CHECK(ik >= 0 && ik < 8, "inv(%d) = %d", k, ik);
    CHECK(apply_S(apply_S(x, m, k), m, ik) == x, "m %d: S_inv(%d) o S_%d is not the identity", m, k, k);
    CHECK(sym::inv(ik) == k, "inv(inv(%d)) = %d", k, sym::inv(ik));
    images.insert(apply_S(x, m, k));
  }
  CHECK(images.size() == 8, "m %d: only %zu distinct maps", m, images.size());
  for (int a = 0; a < 8; a++)
    for (int b = 0; b < 8; b++) CHECK(images.count(apply_S(apply_S(x, m, a), m, b)) == 1, "m %d: S_%d o S_%d is none of the eight", m, b, a);
}

int main() {
  for (int m : {4, 5, 19}) check_m(m);
  // mix32 is the finaliser the position hash has always used (a known value pins the constants)
  CHECK(mix32(0u) == 0u && mix32(1u) == 0x514E28B7u, "mix32(1) = %08x", mix32(1u));
  // keys of LCG-drawn 5x5 boards: printed for the Python restatement
  uint64_t lcg = 12345;
  auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 33); };
  for (int t = 0; t < 64; t++) {
    int32_t board[25];
    for (int c = 0; c < 25; c++) board[c] = (int32_t)(next() % 3u);
    const int to_move = 1 + (int)(next() % 2u);
    const uint64_t seed = ((uint64_t)next() << 32) | next();
    const uint32_t ph = sym::position_key(board, 25, to_move);
    int8_t small[25];
    for (int c = 0; c < 25; c++) small[c] = (int8_t)board[c];
    CHECK(sym::position_key(small, 25, to_move) == ph, "the key depends on the cell type");
    printf("key %llu %d %d", (unsigned long long)seed, to_move, sym::of_key(ph, sym::fold_seed(seed)));
    for (int c = 0; c < 25; c++) printf(" %d", board[c]);
    printf("\n");
  }
  if (fails) { printf("SYM CHECK FAILED (%d)\n", fails); return 1; }
  printf("SYM OK\n");
  return 0;
}
