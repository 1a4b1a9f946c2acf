// The packed plane layout of a replay window made by agz_replay_create_packed (DESIGN.md §2 replay-packed).  ONE definition for host and
// device: k_replay_pack_check / k_replay_pack / k_replay_sample_packed (replay.hip), the host functions agz_replay_pack_host and
// agz_replay_get, and a plain g++ check (tests/cpp/replay_pack_check.cpp).  Integer arithmetic only, and nothing of HIP is included.
//
//   palette        1 to 4 pairwise distinct 32-bit patterns, compared as uint32 and never as floats: +0.0 and -0.0 are different entries,
//                  a NaN pattern is a legal one
//   code           the index of a cell's bit pattern in the palette; a pattern that is not in it has no code (code_of gives -1)
//   word           CODE_BITS = 2 bits a cell, 16 cells in a uint32; wpp(mm) = (mm + 15) / 16 words hold a plane of mm cells and EVERY PLANE
//                  STARTS A WORD, so a symmetry gather never leaves its plane's words
//   cell c of plane f of a row     word f * wpp + (c >> 4), bits [2 * (c & 15), 2 * (c & 15) + 2)
//   the unused high bits of a plane's last word are zero; a packed row is F * wpp words
// Decoding gives back the palette entry's bits exactly.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGZ_PACK_HD __host__ __device__ inline __attribute__((always_inline))   // (no macro of hip_runtime.h: includable before it)
#else
#define AGZ_PACK_HD inline
#endif

namespace agz {
namespace replay_pack {

constexpr int CODE_BITS = 2;
constexpr int CODES_PER_WORD = 32 / CODE_BITS;   // 16
constexpr int MAX_PALETTE = 1 << CODE_BITS;      // 4

// entries [n, 4) repeat entry 0: no code selects them, and four kernel arguments are always defined
struct Palette {
  uint32_t e[MAX_PALETTE];
  int n;
};

AGZ_PACK_HD int wpp(int mm) { return (mm + CODES_PER_WORD - 1) / CODES_PER_WORD; }
AGZ_PACK_HD int word_of(int mm, int f, int c) { return f * wpp(mm) + (c >> 4); }
AGZ_PACK_HD int shift_of(int c) { return CODE_BITS * (c & (CODES_PER_WORD - 1)); }

// 1 <= n <= 4 and no two entries equal as bit patterns
AGZ_PACK_HD bool palette_ok(const uint32_t* bits, int n) {
  if (n < 1 || n > MAX_PALETTE) return false;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++)
      if (bits[i] == bits[j]) return false;
  return true;
}
AGZ_PACK_HD Palette make_palette(const uint32_t* bits, int n) {
  Palette p;
  p.n = n;
  for (int i = 0; i < MAX_PALETTE; i++) p.e[i] = bits[i < n ? i : 0];
  return p;
}

AGZ_PACK_HD int code_of(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, int n, uint32_t bits) {
  int code = -1;
  if (n > 3 && bits == p3) code = 3;
  if (n > 2 && bits == p2) code = 2;
  if (n > 1 && bits == p1) code = 1;
  if (bits == p0) code = 0;
  return code;
}
AGZ_PACK_HD int code_of(const Palette& p, uint32_t bits) { return code_of(p.e[0], p.e[1], p.e[2], p.e[3], p.n, bits); }

// selects on the two code bits: no table
AGZ_PACK_HD uint32_t decode(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t code) {
  const uint32_t lo = (code & 2u) ? p2 : p0, hi = (code & 2u) ? p3 : p1;
  return (code & 1u) ? hi : lo;
}
AGZ_PACK_HD uint32_t decode(const Palette& p, uint32_t code) { return decode(p.e[0], p.e[1], p.e[2], p.e[3], code); }

AGZ_PACK_HD uint32_t cell_code(const uint32_t* row_words, int mm, int f, int c) {
  return (row_words[word_of(mm, f, c)] >> shift_of(c)) & (uint32_t)(MAX_PALETTE - 1);
}

// One row of F planes of mm cells (bit patterns) into F * wpp(mm) words.  Returns the first element f * mm + c of the row that is not in
// the palette, or -1; `words` may be NULL (validate only) and is written whole, unused bits zero, only up to a bad cell's word.
inline int64_t pack_row(const Palette& p, const uint32_t* bits, int F, int mm, uint32_t* words) {
  const int w = wpp(mm);
  for (int f = 0; f < F; f++) {
    for (int wi = 0; wi < w; wi++) {
      uint32_t word = 0;
      const int c1 = (wi + 1) * CODES_PER_WORD < mm ? (wi + 1) * CODES_PER_WORD : mm;
      for (int c = wi * CODES_PER_WORD; c < c1; c++) {
        const int code = code_of(p, bits[(int64_t)f * mm + c]);
        if (code < 0) return (int64_t)f * mm + c;
        word |= (uint32_t)code << shift_of(c);
      }
      if (words) words[(int64_t)f * w + wi] = word;
    }
  }
  return -1;
}
inline void unpack_row(const Palette& p, const uint32_t* words, int F, int mm, uint32_t* bits) {
  for (int f = 0; f < F; f++)
    for (int c = 0; c < mm; c++) bits[(int64_t)f * mm + c] = decode(p, cell_code(words, mm, f, c));
}

}  // namespace replay_pack
}  // namespace agz
