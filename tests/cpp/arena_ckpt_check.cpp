// CPU check of the arena checkpoint codec (agogo_amd/csrc/arena_ckpt.hpp), on the code engine.hip runs.  Usage: arena_ckpt_check DIR
// A toy arena — 3 games of a 2x3 board, 6 trees with 1, 0, 5, 9, 2, 4 live nodes (trees 2 and 4 in pool 1), a 2-deep ring, 4 example rows
// chained across games 0 and 2 — is written into DIR/toy.bin through the codec in chunks of 4 nodes (so trees are cut) and 5 bytes of
// examples (tests/test_arena_ckpt_cpu.py compares the file with bytes it builds itself from the documented format).  Then: scan returns
// what was written, the nodes and examples read back equal, EVERY truncation and a trailing byte are refused, and every single-field
// corruption scan() must catch is refused with the field named.  Last, the planners engine.hip streams the two large sections by
// (node_chunks, example_chunks, staging_bytes) are held to their contract on tree counts that cut trees, skip empty ones and fill a
// launch's grid.  Prints "ARENA CKPT OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../../agogo_amd/csrc/arena_ckpt.hpp"

using namespace agz::arena_ckpt;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const int G = 3, T = 6, P = 8, R = 2, S = 10, CELLS = 6, A = 6, F = 2, E = 4;
static const int N_NODES[T] = {1, 0, 5, 9, 2, 4};
static const int CUR_POOL[T] = {0, 0, 1, 0, 1, 0};

struct Nodes { std::vector<float> prior, bsum; std::vector<uint32_t> visits; std::vector<int32_t> kids_off; std::vector<int16_t> kids_n, nmove; };
struct Examples { std::vector<float> planes, policy, value; std::vector<int32_t> game, prev; std::vector<uint8_t> labelled; };
struct Toy { Shape h; Host host; Small s; Nodes n; Examples e; };

static Toy toy() {
  Toy y;
  y.h = Shape{{AGZ_GAME_MNK, 2, 3, 2, 0.5f, 6, AGZ_ENC_TWOPLANE}, {1.0f, 2, 3, 0, 4, 0, 0.0f, 1, 0.0f, AGZ_DONT_PREFER_PASS}, (uint32_t)G, 1u, (uint32_t)P, (uint32_t)R, (uint32_t)S};
  y.host = Host{0x1111222233334444ull, 0x5555666677778888ull, 7, 5, 0};
  Small& s = y.s;
  s.board.assign(G * P, 0); s.ring.assign(G * R * P, 0); s.moves.assign(G * S, 0); s.amoves.assign(G * S, 0);
  for (int g = 0; g < G; g++) {
    for (int i = 0; i < CELLS; i++) { s.board[g * P + i] = (int8_t)((g + i) % 3); for (int r = 0; r < R; r++) s.ring[(g * R + r) * P + i] = (int8_t)((g + r + i) % 3); }
    s.to_move.push_back(1 + g % 2); s.ply.push_back(g + 2); s.passes.push_back(g); s.pass_count.push_back(g % 2); s.ended.push_back(g == 1);
    s.winner.push_back(g == 1 ? 2 : 0); s.a_is_black.push_back(g != 2); s.last_move.push_back(g - 1); s.cap_b.push_back(0.5f * g); s.cap_w.push_back(1.5f * g);
    s.zhash.push_back(0xABCD0000u + g); s.n_amoves.push_back(g + 3); s.hist_from.push_back(g % 2);
    for (int j = 0; j < S; j++) { s.moves[g * S + j] = (int16_t)((g + j) % A); s.amoves[g * S + j] = (int16_t)((g + 2 * j) % A - 1); }
    s.rng_game.push_back(0x0102030405060708ull * (g + 1)); s.best_out.push_back(g - 2);
  }
  s.ex_last = {2, -1, 3};
  s.prev_board.assign(T * P, 0); s.pc_hash.assign(T * S, 0); s.pc_move.assign(T * S, 0);
  for (int t = 0; t < T; t++) {
    s.n_nodes.push_back(N_NODES[t]); s.cur_pool.push_back(CUR_POOL[t]); s.has_root.push_back(N_NODES[t] > 0); s.has_prev.push_back(t % 2 == 0);
    s.prev_ply.push_back(t % 3); s.stalled.push_back(t == 3); s.overflow.push_back(t == 4); s.pc_n.push_back(t % 4);
    for (int i = 0; i < CELLS; i++) s.prev_board[t * P + i] = (int8_t)((t + 2 * i) % 3);
    s.rng.push_back(0x1000000000000001ull * (t + 1));
    for (int q = 0; q < S; q++) { s.pc_hash[t * S + q] = 0x9000u + 16 * t + q; s.pc_move[t * S + q] = (int16_t)((t + q) % (A + 1) - 1); }
  }
  for (int k = 0; k < N_COUNTERS; k++) s.counters[k] = 1000ull * k + 7;
  s.ex_count = E;
  // the trees: (kids_off, kids_n) per node; children lie behind their parent, blocks are disjoint
  static const int LINKS[T][9][2] = {
      {{-1, 0}}, {}, {{1, 4}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}},
      {{1, 3}, {-1, 0}, {4, 5}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}}, {{1, 1}, {-1, 0}}, {{1, 2}, {3, 1}, {-1, 0}, {-1, 0}}};
  for (int t = 0; t < T; t++)
    for (int i = 0; i < N_NODES[t]; i++) {
      y.n.prior.push_back(0.25f * i + t); y.n.visits.push_back(10 * t + i + 1); y.n.bsum.push_back(-0.5f * i - t);
      y.n.kids_off.push_back(LINKS[t][i][0]); y.n.kids_n.push_back((int16_t)LINKS[t][i][1]); y.n.nmove.push_back((int16_t)(i == 0 ? -1 : (i + t) % A));
    }
  for (int e = 0; e < E; e++) {
    for (int j = 0; j < F * CELLS; j++) y.e.planes.push_back(e + j / 16.f);
    for (int j = 0; j <= A; j++) y.e.policy.push_back((7 * e + j) / 32.f);
  }
  y.e.value = {1.f, 2.f, -1.f, 1.f}; y.e.game = {0, 2, 0, 2}; y.e.prev = {-1, -1, 0, 1}; y.e.labelled = {1, 0, 1, 0};
  return y;
}

// the file of `y` at the offsets of `l` (the layout of the UNMUTATED toy: a mutated count must not move anything), E as `ex_written`
static bool write_file(const std::string& path, const Toy& y, Layout l, uint64_t ex_written) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = write_head(f, y.h, y.host, y.s, l);
  for (uint64_t a = 0; ok && a < l.nodes; a += 4) {   // chunks of 4 nodes: trees 2, 3 and 5 are cut
    const uint64_t c = std::min<uint64_t>(4, l.nodes - a);
    const void* runs[NODE_FIELDS] = {&y.n.prior[a], &y.n.visits[a], &y.n.bsum[a], &y.n.kids_off[a], &y.n.kids_n[a], &y.n.nmove[a]};
    ok = write_nodes(f, l, a, c, runs);
  }
  const uint64_t true_ex = l.examples;
  l.examples = ex_written;
  ok = ok && write_counters(f, l, y.s);
  l.examples = true_ex;
  uint64_t es[EX_FIELDS];
  ex_sizes(y.h, es);
  const char* base[EX_FIELDS] = {(const char*)y.e.planes.data(), (const char*)y.e.policy.data(), (const char*)y.e.value.data(), (const char*)y.e.game.data(),
                                 (const char*)y.e.prev.data(), (const char*)y.e.labelled.data()};
  for (int k = 0; k < EX_FIELDS; k++)
    for (uint64_t a = 0; ok && a < E * es[k]; a += 5) ok = write_examples(f, l, k, a, std::min<uint64_t>(5, E * es[k] - a), base[k] + a);
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
static Status scan_path(const std::string& path, const Shape& want, Scan* sc, std::string* why) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { *why = "cannot open"; return NOT_ARENA; }
  const Status st = scan(f, want, sc, why);
  fclose(f);
  return st;
}

template <class V> static bool same(const V& a, const V& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); }

// node_chunks on trees of `counts` nodes: the chunks tile [0, nodes) in order; each is non-empty and fits the staging; t0 is the tree of
// its first node and [t0, t0 + nt) holds every tree it touches, inside the arena and inside one launch's grid.  Returns the largest nt.
static int check_node_plan(const char* name, const std::vector<uint64_t>& counts, uint64_t staging) {
  Layout l;
  l.tree_first.assign(1, 0);
  for (uint64_t c : counts) l.tree_first.push_back(l.tree_first.back() + c);
  l.nodes = l.tree_first.back();
  const std::vector<uint64_t>& f = l.tree_first;
  const int T = (int)counts.size();
  const std::vector<Chunk> ch = node_chunks(l, staging);
  CHECK(l.nodes > 0 || ch.empty(), "%s, %llu bytes: %zu chunks of no nodes", name, (unsigned long long)staging, ch.size());
  uint64_t at = 0;
  int t = 0, most = 0;   // t: the tree that holds node `at` (walked, not searched)
  for (const Chunk& c : ch) {
    CHECK(c.field == -1 && c.a == at && c.b > c.a && c.b <= l.nodes, "%s, %llu bytes: chunk [%llu, %llu) at %llu of %llu", name, (unsigned long long)staging,
          (unsigned long long)c.a, (unsigned long long)c.b, (unsigned long long)at, (unsigned long long)l.nodes);
    CHECK(c.b - c.a <= (staging - 4) / 20, "%s, %llu bytes: a chunk of %llu nodes", name, (unsigned long long)staging, (unsigned long long)(c.b - c.a));
    if (c.a != at || c.b <= c.a || c.b > l.nodes) return most;
    while (f[t + 1] <= c.a) t++;
    int last = t;   // the tree that holds node b - 1
    while (f[last + 1] <= c.b - 1) last++;
    CHECK(c.t0 == t, "%s, %llu bytes: node %llu lies in tree %d, the chunk starts at tree %d", name, (unsigned long long)staging, (unsigned long long)c.a, t, c.t0);
    CHECK(c.nt >= 1 && c.nt <= 65535 && c.t0 + c.nt <= T && last < c.t0 + c.nt, "%s, %llu bytes: chunk [%llu, %llu) ends in tree %d, its launch covers [%d, %d + %d) of %d trees", name,
          (unsigned long long)staging, (unsigned long long)c.a, (unsigned long long)c.b, last, c.t0, c.t0, c.nt, T);
    most = std::max(most, c.nt);
    at = c.b;
  }
  CHECK(at == l.nodes, "%s, %llu bytes: the chunks end at node %llu of %llu", name, (unsigned long long)staging, (unsigned long long)at, (unsigned long long)l.nodes);
  return most;
}

// example_chunks: run by run the chunks tile [0, examples * size); every chunk but a run's last is the staging rounded down to 16 bytes
static void check_example_plan(const Shape& h, const Layout& l, uint64_t staging) {
  uint64_t es[EX_FIELDS];
  ex_sizes(h, es);
  const std::vector<Chunk> ch = example_chunks(h, l, staging);
  size_t i = 0;
  for (int k = 0; k < EX_FIELDS; k++) {
    uint64_t at = 0;
    for (; i < ch.size() && ch[i].field == k; i++) {
      CHECK(ch[i].a == at && ch[i].b > at && ch[i].b <= l.examples * es[k], "%llu bytes, run %d: chunk [%llu, %llu) at %llu", (unsigned long long)staging, k,
            (unsigned long long)ch[i].a, (unsigned long long)ch[i].b, (unsigned long long)at);
      const bool last = i + 1 == ch.size() || ch[i + 1].field != k;
      CHECK(last || ch[i].b - ch[i].a == (staging & ~15ull), "%llu bytes, run %d: an inner chunk of %llu bytes", (unsigned long long)staging, k, (unsigned long long)(ch[i].b - ch[i].a));
      CHECK(ch[i].b - ch[i].a <= staging, "%llu bytes, run %d: a chunk of %llu bytes", (unsigned long long)staging, k, (unsigned long long)(ch[i].b - ch[i].a));
      if (ch[i].b <= at) return;
      at = ch[i].b;
    }
    CHECK(at == l.examples * es[k], "%llu bytes, run %d: the chunks end at byte %llu of %llu", (unsigned long long)staging, k, (unsigned long long)at, (unsigned long long)(l.examples * es[k]));
  }
  CHECK(i == ch.size(), "%llu bytes: %zu chunks out of run order", (unsigned long long)staging, ch.size() - i);
}

static void check_planners(const Toy& y, const Layout& l) {
  const std::vector<std::vector<uint64_t>> small = {{1, 0, 5, 9, 2, 4}, {0, 0, 3, 0, 7, 0, 0}, {0, 0, 0}};
  for (const std::vector<uint64_t>& counts : small)
    for (uint64_t staging : {64, 84, 104, 184, 424, 2004}) check_node_plan("small trees", counts, staging);
  std::vector<uint64_t> many(70000, 1);   // more trees than one launch's grid holds, two of them empty
  many[5] = many[69999] = 0;
  check_node_plan("70000 trees", many, 64);
  const int most = check_node_plan("70000 trees", many, 2000004);
  CHECK(most == 65535, "70000 trees in one staging buffer: the largest launch covers %d trees, a grid holds 65535", most);
  check_example_plan(y.h, l, 64);
  check_example_plan(y.h, l, E * 4 * F * CELLS + 1);   // one byte more than the planes
  check_example_plan(y.h, l, E * 4 * (A + 1) + 1);     // ... than the policies
  CHECK(staging_bytes(y.h, l, 256u << 20) == 20 * 21 + 4 && staging_bytes(y.h, l, 200) == 200 && staging_bytes(y.h, l, 10) == 64, "staging_bytes");
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: arena_ckpt_check DIR\n"); return 2; }
  const std::string dir = argv[1], good = dir + "/toy.bin", bad = dir + "/bad.bin";
  const Toy y = toy();
  const Layout l = layout(y.h, y.s);
  CHECK(l.nodes == 21 && l.examples == 4 && l.tree_first[3] == 6, "layout %llu %llu", (unsigned long long)l.nodes, (unsigned long long)l.examples);
  CHECK(check_small(y.h, y.s).empty(), "%s", check_small(y.h, y.s).c_str());
  CHECK(write_file(good, y, l, E), "write");
  const std::vector<unsigned char> bytes = slurp(good);
  CHECK(bytes.size() == l.total, "file %zu bytes, layout %llu", bytes.size(), (unsigned long long)l.total);

  {  // ---- round trip: every section comes back equal
    Scan sc;
    std::string why;
    const Status st = scan_path(good, y.h, &sc, &why);
    CHECK(st == OK, "%s", why.c_str());
    if (st == OK) {
      const Small &a = sc.small, &b = y.s;
      CHECK(memcmp(&sc.host, &y.host, sizeof(Host)) == 0, "host");
      CHECK(same(a.board, b.board) && same(a.ring, b.ring) && same(a.to_move, b.to_move) && same(a.ply, b.ply) && same(a.passes, b.passes) && same(a.pass_count, b.pass_count), "games 1");
      CHECK(same(a.ended, b.ended) && same(a.winner, b.winner) && same(a.a_is_black, b.a_is_black) && same(a.last_move, b.last_move) && same(a.cap_b, b.cap_b) && same(a.cap_w, b.cap_w), "games 2");
      CHECK(same(a.zhash, b.zhash) && same(a.moves, b.moves) && same(a.amoves, b.amoves) && same(a.n_amoves, b.n_amoves) && same(a.hist_from, b.hist_from), "games 3");
      CHECK(same(a.rng_game, b.rng_game) && same(a.ex_last, b.ex_last) && same(a.best_out, b.best_out), "games 4");
      CHECK(same(a.n_nodes, b.n_nodes) && same(a.cur_pool, b.cur_pool) && same(a.has_root, b.has_root) && same(a.has_prev, b.has_prev) && same(a.prev_ply, b.prev_ply), "trees 1");
      CHECK(same(a.stalled, b.stalled) && same(a.overflow, b.overflow) && same(a.pc_n, b.pc_n) && same(a.prev_board, b.prev_board) && same(a.rng, b.rng), "trees 2");
      for (int t = 0; t < T; t++)
        for (int q = 0; q < S; q++) {   // the first pc_n[t] entries are the file's, the rest zero
          CHECK(a.pc_hash[t * S + q] == (q < b.pc_n[t] ? b.pc_hash[t * S + q] : 0u), "pc_hash %d %d", t, q);
          CHECK(a.pc_move[t * S + q] == (q < b.pc_n[t] ? b.pc_move[t * S + q] : 0), "pc_move %d %d", t, q);
        }
      CHECK(memcmp(a.counters, b.counters, sizeof(a.counters)) == 0 && a.ex_count == E && sc.most == 9, "counters, ex_count, most %llu", (unsigned long long)sc.most);
      CHECK(sc.lay.total == l.total && sc.lay.tree_first == l.tree_first, "layout");
      FILE* f = fopen(good.c_str(), "rb");
      Nodes n;
      n.prior.resize(21); n.visits.resize(21); n.bsum.resize(21); n.kids_off.resize(21); n.kids_n.resize(21); n.nmove.resize(21);
      bool ok = f != nullptr;
      for (uint64_t c0 = 0; ok && c0 < 21; c0 += 4) {   // read back in chunks that cut trees
        const uint64_t c = std::min<uint64_t>(4, 21 - c0);
        void* runs[NODE_FIELDS] = {&n.prior[c0], &n.visits[c0], &n.bsum[c0], &n.kids_off[c0], &n.kids_n[c0], &n.nmove[c0]};
        ok = read_nodes(f, sc.lay, c0, c, runs);
      }
      CHECK(ok && same(n.prior, y.n.prior) && same(n.visits, y.n.visits) && same(n.bsum, y.n.bsum) && same(n.kids_off, y.n.kids_off) && same(n.kids_n, y.n.kids_n) && same(n.nmove, y.n.nmove), "nodes");
      Examples e;
      e.planes.resize(E * F * CELLS); e.policy.resize(E * (A + 1)); e.value.resize(E); e.game.resize(E); e.prev.resize(E); e.labelled.resize(E);
      ok = ok && read_examples(f, sc.lay, 0, 0, e.planes.size() * 4, e.planes.data()) && read_examples(f, sc.lay, 1, 0, e.policy.size() * 4, e.policy.data()) &&
           read_examples(f, sc.lay, 2, 0, E * 4, e.value.data()) && read_examples(f, sc.lay, 3, 0, E * 4, e.game.data()) && read_examples(f, sc.lay, 4, 0, E * 4, e.prev.data()) &&
           read_examples(f, sc.lay, 5, 0, E, e.labelled.data());
      CHECK(ok && same(e.planes, y.e.planes) && same(e.policy, y.e.policy) && same(e.value, y.e.value) && same(e.game, y.e.game) && same(e.prev, y.e.prev) && same(e.labelled, y.e.labelled), "examples");
      if (f) fclose(f);
    }
  }

  {  // ---- every truncation, and a trailing byte
    Scan sc;
    std::string why;
    for (size_t n = 0; n < bytes.size(); n++) {
      CHECK(spit(bad, bytes.data(), n), "spit");
      CHECK(scan_path(bad, y.h, &sc, &why) != OK, "a file cut to %zu of %zu bytes is accepted", n, bytes.size());
    }
    std::vector<unsigned char> more = bytes;
    more.push_back(0);
    CHECK(spit(bad, more.data(), more.size()), "spit");
    CHECK(scan_path(bad, y.h, &sc, &why) != OK, "a trailing byte is accepted");
  }

  // ---- one corruption per rule: the mutated toy is written at the good file's offsets and must be refused, naming `token`
  int cases = 0;
  auto refuse = [&](const char* name, const char* token, Status expect, const std::function<void(Toy&, Shape&, uint64_t&)>& mutate) {
    Toy m = y;
    Shape want = y.h;
    uint64_t ex = E;
    mutate(m, want, ex);
    CHECK(write_file(bad, m, l, ex), "write %s", name);
    Scan sc;
    std::string why;
    const Status st = scan_path(bad, want, &sc, &why);
    CHECK(st == expect, "%s: status %d, expected %d (%s)", name, (int)st, (int)expect, why.c_str());
    CHECK(why.find(token) != std::string::npos, "%s: the refusal \"%s\" does not name %s", name, why.c_str(), token);
    cases++;
  };
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  refuse("the build's RING", "constants", NOT_ARENA, [](Toy&, Shape& w, uint64_t&) { w.ring = 3; });
  refuse("the build's CELLS_PAD", "constants", NOT_ARENA, [](Toy&, Shape& w, uint64_t&) { w.cells_pad = 16; });
  refuse("n_games", "n_games", MISMATCH, [](Toy&, Shape& w, uint64_t&) { w.n_games = 4; });
  refuse("board size", "game.m", MISMATCH, [](Toy&, Shape& w, uint64_t&) { w.game.m = 3; });
  refuse("game kind", "game.kind", MISMATCH, [](Toy&, Shape& w, uint64_t&) { w.game.kind = AGZ_GAME_KOMI; });
  refuse("Budget", "mcts.Budget", MISMATCH, [](Toy&, Shape& w, uint64_t&) { w.mcts.Budget = 5; });
  refuse("moves_stride", "moves_stride", MISMATCH, [](Toy&, Shape& w, uint64_t&) { w.moves_stride = 11; });
  refuse("restart word", "host scalars", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.host.restart = 2; });
  refuse("n_nodes < 0", "n_nodes[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.n_nodes[0] = -1; });
  refuse("n_nodes beyond any pool", "n_nodes[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.n_nodes[1] = 1 << 30; });
  refuse("n_nodes not the node count", "sum of n_nodes", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.n_nodes[1] = 1; });
  refuse("cur_pool", "cur_pool[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.cur_pool[2] = 2; });
  refuse("has_root without nodes", "has_root[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.has_root[1] = 1; });
  refuse("kids_off at the parent", "kids_off[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_off[1] = 0; });          // (node 1 = tree 2's root)
  refuse("kids_off before the parent", "kids_off[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_off[6 + 2] = 1; });
  refuse("kids_off past n_nodes", "kids_off[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_off[1] = 5; });
  refuse("kids_off + kids_n past n_nodes", "kids_off + kids_n", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_n[1] = 5; });
  refuse("kids_n < 0", "kids_n[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_n[1] = -1; });
  refuse("kids_n > A + 1", "kids_n[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_n[6 + 2] = 8; });
  refuse("kids_n without children", "no children", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_n[0] = 1; });
  refuse("a shared child block", "shared child block", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.kids_off[6 + 1] = 4; m.n.kids_n[6 + 1] = 1; });
  refuse("nmove = A", "nmove[3]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.nmove[6 + 3] = 6; });
  refuse("nmove below Resign", "nmove[3]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.n.nmove[6 + 3] = -3; });
  refuse("prior NaN", "prior", BROKEN, [&](Toy& m, Shape&, uint64_t&) { m.n.prior[20] = nan; });
  refuse("bsum infinite", "bsum", BROKEN, [&](Toy& m, Shape&, uint64_t&) { m.n.bsum[0] = -inf; });
  refuse("ply > max_moves", "ply[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.ply[0] = 7; });
  refuse("n_amoves > stride", "n_amoves[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.n_amoves[2] = 11; });
  refuse("pc_n at the stride", "pc_n[5]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.pc_n[5] = 10; });
  refuse("prev_ply > ply", "prev_ply[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.prev_ply[2] = 5; });                  // (tree 2 = game 2, ply 4, has_prev)
  refuse("a move of the history", "moves[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.moves[S + 1] = 6; });
  refuse("last_move", "last_move[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.last_move[0] = 6; });
  refuse("ex_count", "ex_count", BROKEN, [](Toy&, Shape&, uint64_t& ex) { ex = 1ull << 40; });
  refuse("ex_count negative", "ex_count", BROKEN, [](Toy&, Shape&, uint64_t& ex) { ex = ~0ull; });
  refuse("ex_count not the rows", "bytes long", BROKEN, [](Toy&, Shape&, uint64_t& ex) { ex = 3; });
  refuse("ex_prev forward", "ex_prev[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.e.prev[2] = 3; });
  refuse("ex_prev itself", "ex_prev[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.e.prev[1] = 1; });
  refuse("ex_prev below -1", "ex_prev[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.e.prev[0] = -2; });
  refuse("ex_last", "ex_last[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.ex_last[1] = 4; });
  refuse("ex_game = G", "ex_game[3]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.e.game[3] = 3; });
  refuse("ex_game < 0", "ex_game[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.e.game[0] = -1; });
  refuse("ex_labelled", "ex_labelled[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.e.labelled[1] = 2; });
  refuse("to_move None", "to_move[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.to_move[0] = AGZ_NONE; });
  refuse("to_move 3", "to_move[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.to_move[1] = 3; });
  refuse("winner", "winner[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.winner[2] = 3; });
  refuse("a board cell", "board[1]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.board[P + 2] = 3; });
  refuse("a ring cell", "ring[2]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.ring[(2 * R + 1) * P] = -1; });
  refuse("a prev_board cell", "prev_board[4]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.prev_board[4 * P + 5] = 7; });
  refuse("a_is_black", "a_is_black[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.a_is_black[0] = 2; });
  refuse("ended", "ended[0]", BROKEN, [](Toy& m, Shape&, uint64_t&) { m.s.ended[0] = -1; });
  {  // byte patches: the magic words and the length word
    Scan sc;
    std::string why;
    std::vector<unsigned char> b = bytes;
    b[7] = '2';
    CHECK(spit(bad, b.data(), b.size()) && scan_path(bad, y.h, &sc, &why) == NOT_ARENA, "magic: %s", why.c_str());
    b = bytes; b[b.size() - 16] = 'X';
    CHECK(spit(bad, b.data(), b.size()) && scan_path(bad, y.h, &sc, &why) == BROKEN && why.find("end marker") != std::string::npos, "end marker: %s", why.c_str());
    b = bytes; b[b.size() - 8] ^= 1;
    CHECK(spit(bad, b.data(), b.size()) && scan_path(bad, y.h, &sc, &why) == BROKEN && why.find("end marker") != std::string::npos, "length word: %s", why.c_str());
    cases += 3;
  }
  {  // lanes are informational: a file from another lane count loads
    Shape want = y.h;
    want.lanes = 4;
    Scan sc;
    std::string why;
    CHECK(scan_path(good, want, &sc, &why) == OK, "lanes: %s", why.c_str());
  }
  check_planners(y, l);
  remove(bad.c_str());
  printf("%d corruptions refused\n", cases);
  if (fails) { printf("%d check(s) failed\n", fails); return 1; }
  printf("ARENA CKPT OK\n");
  return 0;
}
