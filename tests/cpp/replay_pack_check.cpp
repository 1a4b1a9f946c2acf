// Plain g++ check of agogo_amd/csrc/replay_pack.hpp (no HIP): the packed plane layout of a replay window, on the code the pack and sampler
// kernels compile.  Driven by tests/test_replay_pack_cpu.py.
//   palettes are compared as bit patterns (+0.0 and -0.0 differ, a NaN pattern is an entry), a pattern outside has no code, duplicate
//   entries and sizes outside 1..4 are refused, every plane starts a word, unused high bits are zero, unpack(pack(row)) is the row.
// Then it prints `geom <mm> <wpp>`, `cell <mm> <f> <c> <word> <shift>` and, for fixed rows, `row <id> <F> <mm> <n> <palette...>`,
// `codes <id> <code...>` and `words <id> <word...>` lines, which the Python test recomputes with Python integers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../agogo_amd/csrc/replay_pack.hpp"

using namespace agz;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  static_assert(replay_pack::CODE_BITS == 2 && replay_pack::CODES_PER_WORD == 16 && replay_pack::MAX_PALETTE == 4, "the declared constants");
  const uint32_t PZ = 0x00000000u, NZ = 0x80000000u, ONE = 0x3F800000u, MONE = 0xBF800000u, MILLI = 0x3A83126Fu, NAN1 = 0x7FC00001u;
  // palettes
  {
    const uint32_t wq[4] = {PZ, NZ, ONE, MONE};
    CHECK(replay_pack::palette_ok(wq, 4) && replay_pack::palette_ok(wq, 1) && replay_pack::palette_ok(wq, 3), "a good palette refused");
    CHECK(!replay_pack::palette_ok(wq, 0) && !replay_pack::palette_ok(wq, 5) && !replay_pack::palette_ok(wq, -1), "a size outside 1..4 admitted");
    const uint32_t dup[4] = {PZ, ONE, PZ, MONE};
    CHECK(!replay_pack::palette_ok(dup, 4) && !replay_pack::palette_ok(dup, 3) && replay_pack::palette_ok(dup, 2), "duplicates");
    const replay_pack::Palette p = replay_pack::make_palette(wq, 4);
    for (int i = 0; i < 4; i++) {
      CHECK(replay_pack::code_of(p, wq[i]) == i, "code_of entry %d", i);
      CHECK(replay_pack::decode(p, (uint32_t)i) == wq[i], "decode %d", i);
    }
    CHECK(replay_pack::code_of(p, MILLI) == -1 && replay_pack::code_of(p, NAN1) == -1, "a pattern outside the palette has a code");
    const uint32_t pz[1] = {PZ};
    const replay_pack::Palette p1 = replay_pack::make_palette(pz, 1);
    CHECK(replay_pack::code_of(p1, PZ) == 0 && replay_pack::code_of(p1, NZ) == -1, "-0.0 is in a palette that holds only +0.0");
    const uint32_t nn[2] = {NZ, NAN1};
    const replay_pack::Palette pn = replay_pack::make_palette(nn, 2);
    CHECK(replay_pack::code_of(pn, NAN1) == 1 && replay_pack::code_of(pn, NZ) == 0 && replay_pack::code_of(pn, PZ) == -1 &&
              replay_pack::code_of(pn, 0x7FC00000u) == -1, "the NaN entry is compared as bits");
    CHECK(replay_pack::decode(pn, 1) == NAN1, "the NaN entry is decoded with its payload");
    // an unused entry never matches: a 3-entry palette does not admit what sits in its padding
    const uint32_t three[3] = {MILLI, ONE, MONE};
    const replay_pack::Palette p3 = replay_pack::make_palette(three, 3);
    CHECK(replay_pack::code_of(p3, MILLI) == 0 && replay_pack::code_of(p3, MONE) == 2 && replay_pack::code_of(p3, PZ) == -1, "3-entry palette");
  }
  // geometry
  const int mms[] = {1, 9, 15, 16, 17, 25, 42, 361};
  for (int mm : mms) {
    printf("geom %d %d\n", mm, replay_pack::wpp(mm));
    for (int f : {0, 1, 17})
      for (int c = 0; c < mm; c++) {
        const int w = replay_pack::word_of(mm, f, c), sh = replay_pack::shift_of(c);
        CHECK(w >= f * replay_pack::wpp(mm) && w < (f + 1) * replay_pack::wpp(mm), "cell %d of plane %d leaves its plane's words", c, f);
        CHECK(sh >= 0 && sh <= 30 && sh % 2 == 0, "shift %d", sh);
        printf("cell %d %d %d %d %d\n", mm, f, c, w, sh);
      }
  }
  // fixed rows: codes from a small generator, packed, printed, unpacked
  const uint32_t pals[][4] = {{PZ, NZ, ONE, MONE}, {MILLI, PZ, ONE, MONE}, {ONE, 0, 0, 0}, {MILLI, ONE, MONE, 0}, {NZ, NAN1, 0, 0}};
  const int pal_n[] = {4, 4, 1, 3, 2};
  int id = 0;
  for (int pi = 0; pi < 5; pi++) {
    const replay_pack::Palette p = replay_pack::make_palette(pals[pi], pal_n[pi]);
    for (int mm : mms) {
      const int F = mm == 361 ? 18 : 3, w = replay_pack::wpp(mm);
      std::vector<uint32_t> bits((size_t)F * mm), words((size_t)F * w, 0xFFFFFFFFu), back((size_t)F * mm);
      std::vector<int> codes((size_t)F * mm);
      uint32_t x = 12345u + 977u * (uint32_t)id;
      for (size_t i = 0; i < bits.size(); i++) {
        x = x * 1103515245u + 12345u;
        codes[i] = (int)((x >> 16) % (uint32_t)p.n);
        bits[i] = p.e[codes[i]];
      }
      CHECK(replay_pack::pack_row(p, bits.data(), F, mm, nullptr) == -1, "a row of palette entries refused");
      CHECK(replay_pack::pack_row(p, bits.data(), F, mm, words.data()) == -1, "a row of palette entries refused");
      replay_pack::unpack_row(p, words.data(), F, mm, back.data());
      CHECK(back == bits, "unpack(pack(row)) != row (palette %d, mm %d)", pi, mm);
      for (int f = 0; f < F; f++) {
        for (int c = 0; c < mm; c++) CHECK((int)replay_pack::cell_code(words.data(), mm, f, c) == codes[(size_t)f * mm + c], "cell_code");
        if (mm % 16) CHECK((words[(size_t)f * w + w - 1] >> (2 * (mm % 16))) == 0, "unused high bits are not zero");
      }
      // the first bad element is the smallest one
      if (mm >= 9) {
        std::vector<uint32_t> bad = bits;
        bad[(size_t)2 * mm + 5] = 0x12345678u;
        bad[(size_t)1 * mm + 7] = 0x12345678u;
        CHECK(replay_pack::pack_row(p, bad.data(), F, mm, nullptr) == (int64_t)mm + 7, "first bad element");
      }
      printf("row %d %d %d %d", id, F, mm, p.n);
      for (int i = 0; i < p.n; i++) printf(" %u", p.e[i]);
      printf("\ncodes %d", id);
      for (int cd : codes) printf(" %d", cd);
      printf("\nwords %d", id);
      for (uint32_t wd : words) printf(" %u", wd);
      printf("\n");
      id++;
    }
  }
  if (fails) { printf("REPLAY PACK CHECK FAILED (%d)\n", fails); return 1; }
  printf("REPLAY PACK OK\n");
  return 0;
}
