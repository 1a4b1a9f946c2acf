// The replay window's checkpoint file (agz_replay_save / agz_replay_load): its byte layout, the validation of its header and lengths,
// and the chunks its rows are streamed in (row_chunks), and nothing else.  Host-only: include/agz.h, replay.hpp, replay_pack.hpp and the
// standard library, so tests/cpp/replay_ckpt_check.cpp checks this very code under g++ (tests/test_replay_ckpt_cpu.py).  replay.hip
// describes a window as a Header and hands the three arrays over as ranges of rows; it knows nothing of the bytes.
//
// All words are little-endian, nothing is padded, every count is 64 bits wide.  F, H, W = the planes' shape, A1 = PolicyLen, mm = H * W,
// wpp = (mm + 15) / 16 (replay_pack.hpp).  A file is
//
//     "AGZRPW01"
//     shape     uint32 Features, Height, Width, PolicyLen
//     form      uint32 form (0 = fp32 planes, 1 = packed), uint32 n_palette (0 for form 0, 1 to 4 for form 1), uint32 palette[4] as bit
//               patterns (entries [n_palette, 4) are 0)
//     counts    uint64 total, uint64 live, uint64 capacity of the saving window (capacity is informational, except that
//               live == min(total, capacity); a window that holds fewer rows than that — after a load into a larger window, until
//               appends have filled it — writes live here)
//     digest    uint64 = agz_replay_digest of the window at save time (replay.hpp: of the LOGICAL content, the same for both forms)
//     planes    form 0: float32 [live][F * mm]        form 1: uint32 [live][F * wpp]   (replay_pack.hpp's layout, unchanged)
//     policy    float32 [live][A1]
//     value     float32 [live]
//     end       "AGZRPWZZ", uint64 the file's total length
//
// Rows are stored in LOGICAL order, the oldest live row first: the file does not depend on where the ring sat or how large it was.  An
// empty window (live 0) is a valid file of 96 bytes.
//
// read_head() validates the header, the counts and the length of the WHOLE file against them before the caller reads a row.  What lies
// inside the rows — a packed file's codes and unused bits, an fp32 file's cells against a packed window's palette, the digest — is
// checked on the device as the chunks stream by (k_replay_ckpt_scan, replay.hip).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "agz.h"
#include "replay.hpp"
#include "replay_pack.hpp"

namespace agz {
namespace replay_ckpt {

constexpr uint64_t HEAD_BYTES = 8 + 16 + 24 + 24 + 8;   // magic, shape, form, counts, digest
constexpr uint64_t END_BYTES = 16;
enum { PLANES = 0, POLICY = 1, VALUE = 2, ARRAYS = 3 };

struct Header {
  uint32_t F, H, W, A1;
  uint32_t form, n_palette, palette[replay_pack::MAX_PALETTE];
  uint64_t total, live, capacity, digest;
  uint64_t mm() const { return (uint64_t)H * W; }
  uint64_t xs() const { return (uint64_t)F * mm(); }
  uint64_t row_words() const { return (uint64_t)F * (uint64_t)replay_pack::wpp((int)mm()); }
  uint64_t rowlen() const { return xs() + A1 + 1; }   // of the digest: elements of a logical row
};

// where the three arrays lie, from the header alone
struct Layout {
  uint64_t row_bytes[ARRAYS] = {}, off[ARRAYS] = {}, end_off = 0, total = 0;
};
inline Layout layout(const Header& h) {
  Layout l;
  l.row_bytes[PLANES] = 4 * (h.form ? h.row_words() : h.xs());
  l.row_bytes[POLICY] = 4ull * h.A1;
  l.row_bytes[VALUE] = 4;
  uint64_t o = HEAD_BYTES;
  for (int k = 0; k < ARRAYS; k++) { l.off[k] = o; o += h.live * l.row_bytes[k]; }
  l.end_off = o;
  l.total = o + END_BYTES;
  return l;
}

// ---- the steps the arrays are streamed in (replay.hip, through ckpt_stream.hpp's pump) -------------------------------------------------
constexpr uint64_t CKPT_MAX_ROWS = 1u << 30;   // of one chunk: the kernels count a chunk's rows in an int

struct Chunk { int k; uint64_t j0, cnt; };     // rows [j0, j0 + cnt) of array k, in the file's logical order

// rows [from, to) of the three arrays in file order, each cut into chunks of as many whole rows as `staging` bytes hold (at least one):
// emit(Chunk) for each.  Returns the bytes of the largest chunk, and at least 64.
template <class Fn>
inline uint64_t row_chunks(const Layout& l, uint64_t from, uint64_t to, uint64_t staging, Fn emit) {
  uint64_t bytes = 64;
  for (int k = 0; k < ARRAYS; k++) {
    uint64_t rows = staging / l.row_bytes[k];
    if (rows < 1) rows = 1;
    if (rows > CKPT_MAX_ROWS) rows = CKPT_MAX_ROWS;
    for (uint64_t j = from; j < to; j += rows) {
      const uint64_t cnt = rows < to - j ? rows : to - j;
      emit(Chunk{k, j, cnt});
      if (cnt * l.row_bytes[k] > bytes) bytes = cnt * l.row_bytes[k];
    }
  }
  return bytes;
}

// ---- writer -----------------------------------------------------------------------------------------------------------------------------
inline bool seek_to(FILE* f, uint64_t off) { return fseeko(f, (off_t)off, SEEK_SET) == 0; }

inline bool write_head(FILE* f, const Header& h) {
  const uint32_t shape[4] = {h.F, h.H, h.W, h.A1}, form[2] = {h.form, h.n_palette};
  const uint64_t counts[4] = {h.total, h.live, h.capacity, h.digest};
  return fwrite("AGZRPW01", 1, 8, f) == 8 && fwrite(shape, 4, 4, f) == 4 && fwrite(form, 4, 2, f) == 2 && fwrite(h.palette, 4, 4, f) == 4 &&
         fwrite(counts, 8, 4, f) == 4;
}
// rows [first, first + count) of array k, in logical order
inline bool write_rows(FILE* f, const Layout& l, int k, uint64_t first, uint64_t count, const void* bytes) {
  return count == 0 || (seek_to(f, l.off[k] + first * l.row_bytes[k]) && fwrite(bytes, (size_t)l.row_bytes[k], (size_t)count, f) == count);
}
inline bool write_end(FILE* f, const Layout& l) {
  return seek_to(f, l.end_off) && fwrite("AGZRPWZZ", 1, 8, f) == 8 && fwrite(&l.total, 8, 1, f) == 1;
}

// ---- reader ---------------------------------------------------------------------------------------------------------------------------
enum Status {
  OK = 0,
  NOT_WINDOW,   // no window checkpoint
  MISMATCH,     // rows of another shape (why names the field)
  BROKEN        // truncated, too long, or inconsistent
};

inline bool read_rows(FILE* f, const Layout& l, int k, uint64_t first, uint64_t count, void* bytes) {
  return count == 0 || (seek_to(f, l.off[k] + first * l.row_bytes[k]) && fread(bytes, (size_t)l.row_bytes[k], (size_t)count, f) == count);
}

// `want`: the loading window's F, H, W, A1 (nothing else of it is read).  The header, the counts, the file's length and its end mark are
// checked; *why says what was wrong.
inline Status read_head(FILE* f, const Header& want, Header* out, Layout* lay, std::string* why) {
  char buf[200];
  auto fail = [&](Status st, const std::string& w) { *why = w; return st; };
  if (fseeko(f, 0, SEEK_END) != 0) return fail(NOT_WINDOW, "cannot seek");
  const int64_t len = (int64_t)ftello(f);
  char magic[8];
  if (len < 0 || !seek_to(f, 0) || fread(magic, 1, 8, f) != 8 || memcmp(magic, "AGZRPW01", 8) != 0) return fail(NOT_WINDOW, "not a replay window checkpoint (magic)");
  Header h{};
  uint32_t shape[4], form[2];
  uint64_t counts[4];
  if (fread(shape, 4, 4, f) != 4 || fread(form, 4, 2, f) != 2 || fread(h.palette, 4, 4, f) != 4 || fread(counts, 8, 4, f) != 4) return fail(BROKEN, "truncated inside the header");
  h.F = shape[0]; h.H = shape[1]; h.W = shape[2]; h.A1 = shape[3]; h.form = form[0]; h.n_palette = form[1];
  h.total = counts[0]; h.live = counts[1]; h.capacity = counts[2]; h.digest = counts[3];
#define AGZ_RPW_SAME(field, name)                                                                                         \
  if (h.field != want.field) {                                                                                            \
    snprintf(buf, sizeof(buf), "%s differs: the file has %u, this window %u", name, (unsigned)h.field, (unsigned)want.field); \
    return fail(MISMATCH, buf);                                                                                           \
  }
  AGZ_RPW_SAME(F, "Features") AGZ_RPW_SAME(H, "Height") AGZ_RPW_SAME(W, "Width") AGZ_RPW_SAME(A1, "PolicyLen")
#undef AGZ_RPW_SAME
  if (h.F < 1 || h.H < 1 || h.W < 1 || h.A1 < 1 || h.xs() + h.A1 + 1 > (1ull << 30)) return fail(BROKEN, "bad shape");
  if (h.form > 1) { snprintf(buf, sizeof(buf), "form %u (0 = fp32 planes, 1 = packed)", h.form); return fail(BROKEN, buf); }
  if (h.form == 0) {
    if (h.n_palette != 0 || h.palette[0] || h.palette[1] || h.palette[2] || h.palette[3]) return fail(BROKEN, "palette words in a file of fp32 planes");
  } else {
    if (!replay_pack::palette_ok(h.palette, (int)h.n_palette)) { snprintf(buf, sizeof(buf), "palette of %u entries (1 to 4, pairwise distinct)", h.n_palette); return fail(BROKEN, buf); }
    for (uint32_t i = h.n_palette; i < (uint32_t)replay_pack::MAX_PALETTE; i++)
      if (h.palette[i]) return fail(BROKEN, "palette: an unused entry is not 0");
  }
  if (h.live > h.total) { snprintf(buf, sizeof(buf), "live %llu > total %llu", (unsigned long long)h.live, (unsigned long long)h.total); return fail(BROKEN, buf); }
  if (h.capacity < 1 || h.live != replay::live(h.total, h.capacity)) {
    snprintf(buf, sizeof(buf), "live %llu is not min(total %llu, capacity %llu)", (unsigned long long)h.live, (unsigned long long)h.total, (unsigned long long)h.capacity);
    return fail(BROKEN, buf);
  }
  if (h.live > (1ull << 40)) return fail(BROKEN, "live out of range");   // (rows of at most 4 GiB: no offset below overflows)
  const Layout l = layout(h);
  if ((uint64_t)len != l.total) { snprintf(buf, sizeof(buf), "truncated or overlong: the file is %lld bytes long, its counts say %llu", (long long)len, (unsigned long long)l.total); return fail(BROKEN, buf); }
  char endm[8];
  uint64_t total = 0;
  if (!seek_to(f, l.end_off) || fread(endm, 1, 8, f) != 8 || fread(&total, 8, 1, f) != 1 || memcmp(endm, "AGZRPWZZ", 8) != 0 || total != l.total) return fail(BROKEN, "bad end marker");
  *out = h;
  *lay = l;
  return OK;
}

}  // namespace replay_ckpt
}  // namespace agz
