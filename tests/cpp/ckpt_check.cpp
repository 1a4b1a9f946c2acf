// CPU check of the trainer's checkpoint codec (agogo_amd/csrc/ckpt.hpp), on the code train.hip runs.  Usage: ckpt_check DIR
// Writes the 12 forms of a toy layout into DIR (tests/test_ckpt_cpu.py compares them with bytes it builds itself from the documented
// format), then checks on each: scan returns what was written and where; for three ranks, every rank's rows; every truncation and two
// extensions are refused; every inconsistent file of the right length is refused.  A refusal reports no offsets.  Prints "CKPT OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../agogo_amd/csrc/ckpt.hpp"

using namespace agz::ckpt;
typedef std::vector<unsigned char> Bytes;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const uint64_t COUNT[5] = {1, 2, 3, 7, 4};
static const bool BATCH[5] = {false, true, false, true, false};
static const uint64_t BN_C[3] = {3, 2, 1};
static float value(int g, size_t i, uint64_t e) { return 1000.f * g + 100.f * i + (float)e + 0.5f; }

static Layout layout(bool tied, int nr) {
  Layout l{{3, 1, 8, 2 * nr, 3, 3, 2, 10, 0, 0.5f}, tied, {}, {BN_C, BN_C + 3}};
  for (int i = 0; i < 5; i++) l.tensors.push_back({COUNT[i] * (BATCH[i] ? nr : 1), BATCH[i]});
  return l;
}
static Options options(State s) { return {{s == VELOCITY ? 0.5f : 0.f, 0.25f, 2.f, 0}, {0.75f, 0.875f, 0.0078125f, 1}, 0x0102030405ull}; }
static BnBlock bn_block() {
  BnBlock b{0.75f, 1u, {}, {}, {}};
  for (int i = 0; i < 3; i++) {
    b.n.push_back(2.5 + i); b.sm.emplace_back(); b.sv.emplace_back();
    for (uint64_t c = 0; c < BN_C[i]; c++) { b.sm[i].push_back(10.0 * i + c + 0.25); b.sv[i].push_back(100.0 + 10.0 * i + c + 0.125); }
  }
  return b;
}
static std::string DIR;
static std::string name(Form m) { return DIR + "/form_" + (m.tied ? "t" : "p") + std::to_string((int)m.state) + (m.bn ? "b" : "n") + ".bin"; }

static bool write_file(const std::string& path, const Layout& lay, Form m) {
  std::vector<float> v;
  FILE* f = fopen(path.c_str(), "wb");
  bool ok = write(f, lay, m, options(m.state), bn_block(), [&](int g, size_t i) {
    v.resize(lay.tensors[i].count);
    for (uint64_t e = 0; e < v.size(); e++) v[e] = value(g, i, e);
    return std::make_pair((const float*)v.data(), (uint64_t)v.size());
  });
  return f && fclose(f) == 0 && ok;
}
static Bytes slurp(const std::string& path) {
  Bytes b;
  FILE* f = fopen(path.c_str(), "rb");
  for (int c; f && (c = fgetc(f)) != EOF;) b.push_back((unsigned char)c);
  if (f) fclose(f);
  return b;
}
static Status scan_bytes(const Bytes& b, const Layout& lay, Scan* s) {
  const std::string path = DIR + "/scratch.bin";
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (!b.empty() && fwrite(b.data(), 1, b.size(), f) != b.size()) || fclose(f) != 0 || !(f = fopen(path.c_str(), "rb"))) { printf("cannot write %s\n", path.c_str()); exit(2); }
  const Status st = scan(f, lay, s);
  fclose(f);
  return st;
}
static void refused(Bytes b, const Layout& lay, const char* what, Form m) {
  Scan s;
  s.off[0].push_back(1);   // (a refusal also clears what the caller passed in)
  const Status st = scan_bytes(b, lay, &s);
  CHECK(st != OK && s.off[0].empty() && s.off[1].empty() && s.off[2].empty(), "%s accepted (tied %d state %d bn %d)", what, m.tied, m.state, m.bn);
}
template <typename T> static Bytes with(Bytes b, size_t at, T v) { memcpy(&b.at(at), &v, sizeof(T)); return b; }

static void check_form(Form m) {
  const Layout lay = layout(m.tied, 1);
  const Bytes good = slurp(name(m));
  Scan s;
  CHECK(scan_bytes(good, lay, &s) == OK, "the file is refused (tied %d state %d bn %d)", m.tied, m.state, m.bn);
  if (s.off[0].empty()) return;
  // ---- round trip
  const Options want = options(m.state);
  CHECK(s.form.tied == m.tied && s.form.state == m.state && s.form.bn == m.bn, "form");
  if (m.state != NONE) CHECK(memcmp(&s.opt.solver, &want.solver, 16) == 0, "solver options");
  if (m.state == ADAM) CHECK(memcmp(&s.opt.adam, &want.adam, 16) == 0 && s.opt.step == want.step, "Adam options");
  if (m.bn) { const BnBlock b = bn_block(); CHECK(s.bn.lam == b.lam && s.bn.on == b.on && s.bn.n == b.n && s.bn.sm == b.sm && s.bn.sv == b.sv, "BatchNorm block"); }
  for (int g = 0; g < 3; g++) {
    CHECK(s.off[g].size() == (g < groups(m.state) ? 5u : 0u), "group %d has %zu offsets", g, s.off[g].size());
    for (size_t i = 0; i < s.off[g].size(); i++) {
      const std::pair<long, uint64_t> r = rows(lay.tensors[i], s.off[g][i], 0, 1);
      CHECK(r.second == COUNT[i] && r.first == s.off[g][i], "rows of one rank");
      for (uint64_t e = 0; e < r.second; e++) { float x; memcpy(&x, &good.at(r.first + 4 * e), 4); CHECK(x == value(g, i, e), "group %d tensor %zu element %d", g, i, (int)e); }
    }
  }
  // ---- three ranks: the file of the global batch, every rank's rows
  const Layout lay3 = layout(m.tied, 3);
  const std::string p3 = DIR + "/ranks3.bin";
  CHECK(write_file(p3, lay3, m), "writing the three-rank file");
  const Bytes g3 = slurp(p3);
  Scan s3;
  CHECK(scan_bytes(g3, lay3, &s3) == OK, "the three-rank file is refused");
  refused(g3, lay, "the three-rank file under the one-rank layout", m);
  for (int g = 0; g < groups(m.state) && !s3.off[0].empty(); g++)
    for (size_t i = 0; i < 5; i++)
      for (int r = 0; r < 3; r++) {
        const std::pair<long, uint64_t> w = rows(lay3.tensors[i], s3.off[g][i], r, 3);
        CHECK(w.second == COUNT[i], "rank %d tensor %zu: %d rows' floats", r, i, (int)w.second);
        for (uint64_t e = 0; e < w.second; e++) {
          float x; memcpy(&x, &g3.at(w.first + 4 * e), 4);
          CHECK(x == value(g, i, (BATCH[i] ? r * COUNT[i] : 0) + e), "rank %d group %d tensor %zu element %d", r, g, i, (int)e);
        }
      }
  // ---- every truncation, two extensions
  for (size_t n = 0; n < good.size(); n++) refused(Bytes(good.begin(), good.begin() + n), lay, "a truncated file", m);
  for (int extra : {1, 4}) { Bytes b = good; b.resize(b.size() + extra, 0); refused(b, lay, "an extended file", m); }
  // ---- inconsistent files of the right length
  const size_t head = (m.tied ? 16 : 8) + (m.bn ? 4 : 0), last = groups(m.state) - 1;
  for (int g = 0; g <= (int)last; g++)
    for (size_t i = 0; i < 5; i++)
      for (uint64_t d : {COUNT[i] - 1, COUNT[i] + 1}) refused(with(good, s.off[g][i] - 8, d), lay, "a count word off by one", m);
  for (int g = 0; g <= (int)last; g++)   // two count words wrong, the length right: tensor 1 one float longer, tensor 2 one shorter
    refused(with(with(good, s.off[g][1] - 8, COUNT[1] + 1), s.off[g][1] + 4 * (COUNT[1] + 1), COUNT[2] - 1), lay, "two count words that cancel", m);
  for (uint64_t nt : {4, 6}) refused(with(good, head + 40, nt), lay, "a tensor count off by one", m);
  for (int k = 0; k < 10; k++) { Bytes b = good; b[head + 4 * k] ^= 1; refused(b, lay, "a changed configuration field", m); }
  refused(with(good, 7, '6'), lay, "magic AGZTRN06", m);
  refused(with(good, 7, '0'), lay, "magic AGZTRN00", m);
  if (m.tied) {
    for (uint32_t v : {0, 2}) refused(with(good, 12, v), lay, "05 with flags 0 / 2", m);
    for (uint32_t v : {0, 5}) refused(with(good, 8, v), lay, "05 with inner form 0 / 5", m);
  }
  if (m.bn) for (uint32_t v : {0, 4}) refused(with(good, head - 4, v), lay, "03 with inner form 0 / 4", m);
  refused(good, layout(!m.tied, 1), "a file of the other kind", m);
  { Scan k; CHECK(scan_bytes(good, layout(!m.tied, 1), &k) == KIND && k.form.tied == m.tied, "the other kind is not reported as such"); }
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const size_t opt = s.off[0][4] + 4 * COUNT[4];   // the options follow group 0
  if (m.state == VELOCITY) refused(with(good, opt, 0.f), lay, "02 with momentum 0", m);
  if (m.state == ADAM) {
    refused(with(good, opt, 0.5f), lay, "an Adam form with momentum != 0", m);
    for (int32_t on : {0, 2}) refused(with(good, opt + 28, on), lay, "Adam on = 0 / 2", m);
    refused(with(good, opt + 16, 1.f), lay, "beta1 = 1", m);
    refused(with(good, opt + 24, 0.f), lay, "eps = 0", m);
  }
  for (int k = 0; m.state != NONE && k < (m.state == ADAM ? 7 : 3); k++) if (k != 3) refused(with(good, opt + 4 * k, nan), lay, "a NaN option", m);
  if (m.state != NONE) refused(with(good, opt + 12, (int32_t)1), lay, "reserved = 1", m);
  if (m.bn) {
    const size_t bn = s.off[last][4] + 4 * COUNT[4];   // the block follows the last group
    refused(with(good, bn, 1.f), lay, "BatchNorm momentum 1", m);
    refused(with(good, bn + 4, (uint32_t)2), lay, "BatchNorm on = 2", m);
    for (uint32_t n : {2, 4}) refused(with(good, bn + 8, n), lay, "an op count off by one", m);
    size_t at = bn + 12;
    for (int i = 0; i < 3; i++) {
      for (uint64_t c : {BN_C[i] - 1, BN_C[i] + 1}) refused(with(good, at, c), lay, "a changed C", m);
      refused(with(good, at + 8, 0.0), lay, "N = 0", m);
      refused(with(good, at + 8, -1.0), lay, "N < 0", m);
      refused(with(good, at + 8, (double)INFINITY), lay, "N = inf", m);
      for (uint64_t c = 0; c < 2 * BN_C[i]; c++) refused(with(good, at + 16 + 8 * c, (double)NAN), lay, "a NaN sum", m);
      at += 16 + 16 * BN_C[i];
    }
    CHECK(at == good.size(), "the BatchNorm block ends at %zu, the file at %zu", at, good.size());
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: ckpt_check DIR\n"); return 2; }
  DIR = argv[1];
  std::vector<Form> forms;
  for (bool tied : {false, true}) for (State s : {NONE, VELOCITY, ADAM}) for (bool bn : {false, true}) forms.push_back({tied, s, bn});
  for (Form m : forms) CHECK(write_file(name(m), layout(m.tied, 1), m), "writing %s", name(m).c_str());
  for (Form m : forms) check_form(m);
  // the writer keeps asking for tensors without a file (a rank that holds none) and after a failure, and reports both
  for (int pass = 0; pass < 2; pass++) {
    int calls = 0;
    const Layout lay = layout(false, 1);
    FILE* f = pass ? fopen((DIR + "/scratch.bin").c_str(), "wb") : nullptr;
    const bool ok = write(f, lay, {false, ADAM, true}, options(ADAM), bn_block(), [&](int, size_t) { calls++; return std::make_pair((const float*)nullptr, (uint64_t)0); });
    if (f) fclose(f);
    CHECK(!ok && calls == 15, "ok %d after %d calls", ok, calls);
  }
  if (fails) { printf("CKPT FAILED: %d checks\n", fails); return 1; }
  printf("CKPT OK\n");
  return 0;
}
