// CPU check of the replay window's checkpoint codec (agogo_amd/csrc/replay_ckpt.hpp), on the code replay.hip runs.
// Usage: replay_ckpt_check DIR
// A toy window — F = 2 planes of a 5x5 board (25 cells: wpp = 2, fourteen unused bits in every plane's second word), PolicyLen 26, total 10,
// live 7, capacity 7 — is written into DIR/toy_fp32.bin and DIR/toy_packed.bin through the codec in chunks of 3 rows
// (tests/test_replay_ckpt_cpu.py compares both files with bytes it builds itself from the documented format).  Then, for both forms:
// read_head returns what was written, the rows read back in chunks of 3 are equal, EVERY truncation and a trailing byte are refused, and
// every single-word corruption of the header that read_head() must catch is refused with its reason named.  Last, row_chunks, the planner
// replay.hip streams the arrays by, is held to its contract at a staging below one row, of three plane rows and of 1 MB.  Prints the digest of the rows
// ("digest N") and "REPLAY CKPT OK".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../agogo_amd/csrc/replay_ckpt.hpp"

using namespace agz::replay_ckpt;
namespace rpack = agz::replay_pack;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const uint32_t F = 2, H = 5, W = 5, A1 = 26, MM = 25, XS = 50, WPP = 2, RW = 4;
static const uint64_t TOTAL = 10, LIVE = 7, CAP = 7;
static const uint32_t PAL[4] = {0x00000000u, 0x80000000u, 0x3F800000u, 0x7FC00001u};   // +0.0, -0.0, 1.0 and a NaN pattern

struct Toy { Header h; std::vector<uint32_t> planes, policy, value; };   // planes: [LIVE][XS] patterns or [LIVE][RW] words

static Toy toy(bool packed) {
  Toy y;
  std::vector<uint32_t> bits(LIVE * XS);
  for (uint64_t j = 0; j < LIVE; j++) {
    for (uint32_t f = 0; f < F; f++)
      for (uint32_t c = 0; c < MM; c++) bits[j * XS + f * MM + c] = PAL[(j * 7 + f * 3 + c * 5 + (c >> 2)) & 3];
    for (uint32_t e = 0; e < A1; e++) y.policy.push_back(0x3C000000u + (uint32_t)j * 1000u + e);
    y.value.push_back(0xBF000000u + (uint32_t)j);
  }
  y.h = Header{F, H, W, A1, packed ? 1u : 0u, packed ? 4u : 0u, {0, 0, 0, 0}, TOTAL, LIVE, CAP, 0};
  y.h.digest = agz::replay::digest_rows(bits.data(), y.policy.data(), y.value.data(), LIVE, XS, A1);
  if (packed) {
    memcpy(y.h.palette, PAL, sizeof(PAL));
    const rpack::Palette p = rpack::make_palette(PAL, 4);
    y.planes.assign(LIVE * RW, 0xFFFFFFFFu);
    for (uint64_t j = 0; j < LIVE; j++) CHECK(rpack::pack_row(p, &bits[j * XS], (int)F, (int)MM, &y.planes[j * RW]) == -1, "pack row %d", (int)j);
  } else {
    y.planes = bits;
  }
  return y;
}

static bool write_file(const std::string& path, const Toy& y) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const Layout l = layout(y.h);
  bool ok = write_head(f, y.h);
  const uint32_t* base[ARRAYS] = {y.planes.data(), y.policy.data(), y.value.data()};
  for (int k = 0; k < ARRAYS; k++)
    for (uint64_t j = 0; ok && j < y.h.live; j += 3)   // chunks of 3 rows
      ok = write_rows(f, l, k, j, std::min<uint64_t>(3, y.h.live - j), base[k] + j * (l.row_bytes[k] / 4));
  ok = ok && write_end(f, l);
  return fclose(f) == 0 && ok;
}

static std::vector<unsigned char> slurp(const std::string& path) {
  std::vector<unsigned char> b;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return b;
  fseek(f, 0, SEEK_END); b.resize((size_t)ftell(f)); fseek(f, 0, SEEK_SET);
  if (!b.empty() && fread(b.data(), 1, b.size(), f) != b.size()) b.clear();
  fclose(f);
  return b;
}
static bool spit(const std::string& path, const unsigned char* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}
static Status head_of(const std::string& path, const Header& want, Header* h, Layout* l, std::string* why) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { *why = "cannot open"; return NOT_WINDOW; }
  const Status st = read_head(f, want, h, l, why);
  fclose(f);
  return st;
}

// row_chunks over rows [from, to): array by array the chunks tile the range, each holds max(1, staging / row_bytes) rows (an array's last
// chunk what is left), and the result is the largest chunk's bytes, or 64 where none is as large
static void check_row_plan(const Layout& l, uint64_t from, uint64_t to, uint64_t staging) {
  int k_at = 0, n = 0;
  uint64_t at = from, most = 0;
  const uint64_t bytes = row_chunks(l, from, to, staging, [&](const Chunk& c) {
    const int k = c.k;
    const uint64_t j0 = c.j0, cnt = c.cnt;
    if (cnt == 0 || ++n > 3 * (int)(to - from)) {   // (a planner that does not advance would never return)
      printf("FAIL row_chunks(%llu, %llu, %llu bytes): chunk %d holds %llu rows\n", (unsigned long long)from, (unsigned long long)to, (unsigned long long)staging, n, (unsigned long long)cnt);
      exit(1);
    }
    if (k != k_at) {
      CHECK(k == k_at + 1 && at == to, "%llu bytes: array %d ends at row %llu of %llu", (unsigned long long)staging, k_at, (unsigned long long)at, (unsigned long long)to);
      k_at = k; at = from;
    }
    const uint64_t rows = std::max<uint64_t>(1, staging / l.row_bytes[k]);
    CHECK(j0 == at && cnt == std::min(rows, to - at), "%llu bytes, array %d: chunk [%llu, +%llu) at row %llu, %llu rows a chunk", (unsigned long long)staging, k,
          (unsigned long long)j0, (unsigned long long)cnt, (unsigned long long)at, (unsigned long long)rows);
    at = j0 + cnt;
    most = std::max(most, cnt * l.row_bytes[k]);
  });
  if (from == to) CHECK(n == 0, "%llu bytes: %d chunks of no rows", (unsigned long long)staging, n);
  else CHECK(k_at == ARRAYS - 1 && at == to, "%llu bytes: the chunks end in array %d at row %llu of %llu", (unsigned long long)staging, k_at, (unsigned long long)at, (unsigned long long)to);
  CHECK(bytes == std::max<uint64_t>(64, most) && bytes >= 64, "%llu bytes: the largest chunk is %llu bytes, reported %llu", (unsigned long long)staging, (unsigned long long)most, (unsigned long long)bytes);
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: replay_ckpt_check DIR\n"); return 2; }
  const std::string dir = argv[1], bad = dir + "/bad.bin";
  int cases = 0;
  for (int packed = 0; packed < 2; packed++) {
    const std::string good = dir + (packed ? "/toy_packed.bin" : "/toy_fp32.bin");
    const Toy y = toy(packed != 0);
    const Layout l = layout(y.h);
    CHECK(l.row_bytes[PLANES] == (packed ? 16u : 200u) && l.off[PLANES] == HEAD_BYTES && l.off[VALUE] == l.off[POLICY] + LIVE * 104, "layout");
    CHECK(write_file(good, y), "write");
    const std::vector<unsigned char> bytes = slurp(good);
    CHECK(bytes.size() == l.total && l.total == 80 + LIVE * (l.row_bytes[PLANES] + 104 + 4) + 16, "file %zu bytes, layout %llu", bytes.size(), (unsigned long long)l.total);
    if (!packed) printf("digest %llu\n", (unsigned long long)y.h.digest);
    for (uint64_t staging : {(uint64_t)4, 3 * l.row_bytes[PLANES], (uint64_t)1 << 20}) {   // below one row of any array; three plane rows; everything at once
      check_row_plan(l, 0, LIVE, staging);
      check_row_plan(l, 2, LIVE, staging);   // (a load into a smaller window skips the oldest rows)
      check_row_plan(l, 5, 5, staging);
    }

    {  // ---- round trip, read back in chunks of 3 rows
      Header h;
      Layout got;
      std::string why;
      const Status st = head_of(good, y.h, &h, &got, &why);
      CHECK(st == OK, "%s", why.c_str());
      if (st == OK) {
        CHECK(memcmp(&h, &y.h, sizeof(Header)) == 0, "header");
        CHECK(got.total == l.total && got.end_off == l.end_off && memcmp(got.off, l.off, sizeof(l.off)) == 0, "layout");
        FILE* f = fopen(good.c_str(), "rb");
        const std::vector<uint32_t>* src[ARRAYS] = {&y.planes, &y.policy, &y.value};
        for (int k = 0; k < ARRAYS && f; k++) {
          std::vector<uint32_t> back(src[k]->size(), 0xDEADBEEFu);
          bool ok = true;
          for (uint64_t j = 0; ok && j < LIVE; j += 3) ok = read_rows(f, got, k, j, std::min<uint64_t>(3, LIVE - j), back.data() + j * (got.row_bytes[k] / 4));
          CHECK(ok && back == *src[k], "array %d", k);
        }
        if (f) fclose(f);
      }
    }
    {  // ---- every truncation, and a trailing byte
      Header h;
      Layout got;
      std::string why;
      for (size_t n = 0; n < bytes.size(); n++) {
        CHECK(spit(bad, bytes.data(), n), "spit");
        CHECK(head_of(bad, y.h, &h, &got, &why) != OK, "a file cut to %zu of %zu bytes is accepted", n, bytes.size());
      }
      std::vector<unsigned char> more = bytes;
      more.push_back(0);
      CHECK(spit(bad, more.data(), more.size()), "spit");
      CHECK(head_of(bad, y.h, &h, &got, &why) != OK && why.find("bytes long") != std::string::npos, "a trailing byte is accepted (%s)", why.c_str());
    }
    // ---- one corruption per rule of read_head: words of the good file are patched and the file must be refused, naming `token`
    auto refuse = [&](const char* name, const char* token, Status expect, const std::function<void(std::vector<unsigned char>&, Header&)>& mutate) {
      std::vector<unsigned char> b = bytes;
      Header want = y.h;
      mutate(b, want);
      Header h;
      Layout got;
      std::string why;
      CHECK(spit(bad, b.data(), b.size()), "spit %s", name);
      const Status st = head_of(bad, want, &h, &got, &why);
      CHECK(st == expect, "%s: status %d, expected %d (%s)", name, (int)st, (int)expect, why.c_str());
      CHECK(why.find(token) != std::string::npos, "%s: the refusal \"%s\" does not name %s", name, why.c_str(), token);
      cases++;
    };
    auto put32 = [](std::vector<unsigned char>& b, size_t at, uint32_t v) { memcpy(&b[at], &v, 4); };
    auto put64 = [](std::vector<unsigned char>& b, size_t at, uint64_t v) { memcpy(&b[at], &v, 8); };
    refuse("magic", "magic", NOT_WINDOW, [](std::vector<unsigned char>& b, Header&) { b[7] = '2'; });
    refuse("Features", "Features", MISMATCH, [](std::vector<unsigned char>&, Header& w) { w.F = 3; });
    refuse("Height", "Height", MISMATCH, [](std::vector<unsigned char>&, Header& w) { w.H = 4; });
    refuse("Width", "Width", MISMATCH, [](std::vector<unsigned char>&, Header& w) { w.W = 6; });
    refuse("PolicyLen", "PolicyLen", MISMATCH, [](std::vector<unsigned char>&, Header& w) { w.A1 = 25; });
    refuse("form", "form 2", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 24, 2); });
    refuse("live > total", "> total", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put64(b, 48, 6); });
    refuse("live not min(total, capacity)", "is not min", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put64(b, 64, 8); });
    refuse("capacity 0", "is not min", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put64(b, 64, 0); });
    refuse("live not the rows", "bytes long", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put64(b, 56, 6); put64(b, 64, 6); });
    refuse("live enormous", "out of range", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put64(b, 48, ~0ull); put64(b, 56, ~0ull); put64(b, 64, ~0ull); });
    refuse("end mark", "end marker", BROKEN, [&](std::vector<unsigned char>& b, Header&) { b[b.size() - 16] = 'X'; });
    refuse("length word", "end marker", BROKEN, [&](std::vector<unsigned char>& b, Header&) { b[b.size() - 8] ^= 1; });
    if (packed) {
      refuse("n_palette 0", "palette of 0", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 28, 0); });
      refuse("n_palette 5", "palette of 5", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 28, 5); });
      refuse("two equal palette entries", "pairwise distinct", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 32 + 8, PAL[0]); });
      refuse("an unused palette entry", "unused entry", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 28, 3); });
    } else {
      refuse("n_palette in an fp32 file", "palette words", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 28, 1); });
      refuse("a palette word in an fp32 file", "palette words", BROKEN, [&](std::vector<unsigned char>& b, Header&) { put32(b, 32 + 12, 1); });
    }
    {  // the capacity is informational beyond the rule above, and the digest is the caller's to compare: both load as they are
      std::vector<unsigned char> b = bytes;
      put64(b, 72, 12345);
      Header h;
      Layout got;
      std::string why;
      CHECK(spit(bad, b.data(), b.size()) && head_of(bad, y.h, &h, &got, &why) == OK && h.digest == 12345, "digest word: %s", why.c_str());
    }
  }
  {  // an empty window is a valid file of 96 bytes
    Toy y = toy(false);
    y.h.total = y.h.live = 0; y.h.digest = 0;
    y.planes.clear(); y.policy.clear(); y.value.clear();
    Header h;
    Layout got;
    std::string why;
    CHECK(write_file(bad, y) && slurp(bad).size() == 96 && head_of(bad, y.h, &h, &got, &why) == OK && h.live == 0, "empty: %s", why.c_str());
  }
  remove(bad.c_str());
  printf("%d corruptions refused\n", cases);
  if (fails) { printf("%d check(s) failed\n", fails); return 1; }
  printf("REPLAY CKPT OK\n");
  return 0;
}
