// The self-play arena's checkpoint file (agz_arena_save / agz_arena_load): its byte layout, its validation, and the steps its two large
// sections are streamed in (node_chunks, example_chunks), and nothing else.  Host-only:
// include/agz.h and the standard library, so tests/cpp/arena_ckpt_check.cpp checks this very code under g++ (tests/test_arena_ckpt_cpu.py).
// engine.hip describes an arena as a Shape, hands the small state over as whole arrays (Small) and the two large sections — the trees' nodes
// and the example rows — as ranges of their per-field runs; it knows nothing of the bytes.
//
// All words are little-endian, nothing is padded, every count and offset is 64 bits wide (the node section exceeds 4 GB at 19x19 / 512
// games).  G = n_games, T = 2 G trees (tree(agent, g) = agent * G + g), P = CELLS_PAD, R = RING, S = moves_stride, A = the game's action
// space (cells; columns for c4), F = the encoder's planes (2 or 18), cells = m * n.  A file is
//
//     "AGZARN01"
//     conf      agz_game_conf (28 bytes; max_moves as the arena resolved it, never 0), agz_mcts_conf (40 bytes), uint32 n_games,
//               uint32 lanes (agz_arena_set_parallel at save time: informational, not compared), uint32 P, uint32 R, uint32 S
//     host      uint64 seed, uint64 seed0, uint64 prep_expand_seen, int32 moves_done, uint32 restart
//     games     int8 board[G][P], int8 ring[G][R][P], int32 to_move[G], ply[G], passes[G], pass_count[G], ended[G], winner[G], a_is_black[G],
//               last_move[G], float32 cap_b[G], cap_w[G], uint32 zhash[G], int16 moves[G][S], int16 amoves[G][S], int32 n_amoves[G],
//               hist_from[G], uint64 rng_game[G], int32 ex_last[G], best_out[G]
//     trees     int32 n_nodes[T], cur_pool[T], has_root[T], has_prev[T], prev_ply[T], stalled[T], overflow[T], pc_n[T], int8 prev_board[T][P],
//               uint64 rng[T], then per tree t: uint32 pc_hash[pc_n[t]], int16 pc_move[pc_n[t]]
//     nodes     uint64 N = the sum of n_nodes, then six runs of N elements, each tree by tree, a tree's live prefix [0, n_nodes[t]) only:
//               float32 prior[N], uint32 visits[N], float32 bsum[N], int32 kids_off[N], int16 kids_n[N], int16 nmove[N]
//     counters  uint64 [16]
//     examples  uint64 E, float32 planes[E][F * cells], float32 policy[E][A + 1], float32 value[E], int32 game[E], int32 prev[E],
//               uint8 labelled[E]
//     end       "AGZARNZZ", uint64 the file's total length
//
// What is NOT stored, because it is derived or dead at a move boundary (the only place a save is allowed): the virtual-loss flags `vl` (every
// simulation round clears the flags it set before it ends, so they are all clear between rounds and between moves; the loader zeroes them),
// the pool a tree does not live in (it is only the target of the next re-root copy), slot_of_game and the slot counts (recomputed),
// per-simulation scratch (leaf_*, path*, exp_*), callback staging, the zobrist table (a constant of the game).  The host copy of
// a_is_black is refreshed from the file's array.  Differences from the first sketch of the format, following engine.hip: n_amoves may reach
// S (k_end_move appends while na < S; a pass the game ignores does not advance ply), so it is bounded by S, not max_moves; pc_n must leave
// room for the next search's entry (< S); and two rules are stricter than an index check, because a kernel FOLLOWS these links: a node's
// children lie behind it and child blocks are disjoint (the re-root copy walks them without a capacity check), and an example's `prev` is an
// earlier row (the labelling loop walks the chain to its end).
//
// scan() validates the WHOLE file — lengths, constants, configuration, every index a kernel could follow — before the caller changes
// anything; a file it accepts cannot lead a kernel out of bounds or into a cycle.  check_small() is the part of that validation that needs
// no file; agz_arena_save runs it too, so an arena never writes a file it would refuse.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "agz.h"

namespace agz {
namespace arena_ckpt {

constexpr int N_COUNTERS = 16;
constexpr uint64_t MAX_NODES = 1ull << 30;   // per tree: node indices are int32 and pools are addressed as (2 t + pool) * cap + i

struct Shape {
  agz_game_conf game;      // max_moves resolved (> 0)
  agz_mcts_conf mcts;
  uint32_t n_games, lanes, cells_pad, ring, moves_stride;
  uint64_t G() const { return n_games; }
  uint64_t T() const { return 2ull * n_games; }
  int cells() const { return game.m * game.n; }
  int A() const { return game.kind == AGZ_GAME_C4 ? game.n : cells(); }
  int F() const { return game.encoder == AGZ_ENC_WQ ? 18 : 2; }
};
struct Host { uint64_t seed, seed0, prep_expand_seen; int32_t moves_done; uint32_t restart; };

// every per-game and per-tree array, whole and in the arena's own strides (pc_hash / pc_move: [T][S], the file holds the first pc_n[t])
struct Small {
  std::vector<int8_t> board, ring;
  std::vector<int32_t> to_move, ply, passes, pass_count, ended, winner, a_is_black, last_move;
  std::vector<float> cap_b, cap_w;
  std::vector<uint32_t> zhash;
  std::vector<int16_t> moves, amoves;
  std::vector<int32_t> n_amoves, hist_from;
  std::vector<uint64_t> rng_game;
  std::vector<int32_t> ex_last, best_out;
  std::vector<int32_t> n_nodes, cur_pool, has_root, has_prev, prev_ply, stalled, overflow, pc_n;
  std::vector<int8_t> prev_board;
  std::vector<uint64_t> rng;
  std::vector<uint32_t> pc_hash;
  std::vector<int16_t> pc_move;
  uint64_t counters[N_COUNTERS];
  int64_t ex_count;
};

// f(vector, elements per game) / f(vector, elements per tree), in file order.  The one list the writer, the reader and the sizes share.
template <class S, class Fn>
void each_game_array(S& s, const Shape& h, Fn f) {
  f(s.board, (uint64_t)h.cells_pad); f(s.ring, (uint64_t)h.ring * h.cells_pad);
  f(s.to_move, 1); f(s.ply, 1); f(s.passes, 1); f(s.pass_count, 1); f(s.ended, 1); f(s.winner, 1); f(s.a_is_black, 1); f(s.last_move, 1);
  f(s.cap_b, 1); f(s.cap_w, 1); f(s.zhash, 1); f(s.moves, (uint64_t)h.moves_stride); f(s.amoves, (uint64_t)h.moves_stride);
  f(s.n_amoves, 1); f(s.hist_from, 1); f(s.rng_game, 1); f(s.ex_last, 1); f(s.best_out, 1);
}
template <class S, class Fn>
void each_tree_array(S& s, const Shape& h, Fn f) {   // (the variable-length pc_hash / pc_move follow these)
  f(s.n_nodes, 1); f(s.cur_pool, 1); f(s.has_root, 1); f(s.has_prev, 1); f(s.prev_ply, 1); f(s.stalled, 1); f(s.overflow, 1); f(s.pc_n, 1);
  f(s.prev_board, (uint64_t)h.cells_pad); f(s.rng, 1);
}

// the node and example runs: element sizes in file order
enum { NODE_FIELDS = 6, EX_FIELDS = 6 };
constexpr uint64_t NODE_SIZE[NODE_FIELDS] = {4, 4, 4, 4, 2, 2};   // prior, visits, bsum, kids_off, kids_n, nmove: 20 bytes a node
inline void ex_sizes(const Shape& h, uint64_t out[EX_FIELDS]) {     // bytes per row: planes, policy, value, game, prev, labelled
  out[0] = 4ull * h.F() * h.cells(); out[1] = 4ull * (h.A() + 1); out[2] = 4; out[3] = 4; out[4] = 4; out[5] = 1;
}

// where everything behind the per-tree section lies, from the counts alone
struct Layout {
  uint64_t nodes = 0, examples = 0;
  uint64_t node_off[NODE_FIELDS] = {}, counters_off = 0, ex_off[EX_FIELDS] = {}, end_off = 0, total = 0;
  std::vector<uint64_t> tree_first;   // [T + 1] exclusive prefix sum of n_nodes: tree t's nodes are [tree_first[t], tree_first[t + 1])
};
inline uint64_t head_bytes(const Shape& h, const Small& s) {   // magic .. end of the per-tree section
  uint64_t n = 8 + sizeof(agz_game_conf) + sizeof(agz_mcts_conf) + 20 + 32;
  each_game_array(s, h, [&](const auto& v, uint64_t per) { n += h.G() * per * sizeof(v[0]); });
  each_tree_array(s, h, [&](const auto& v, uint64_t per) { n += h.T() * per * sizeof(v[0]); });
  for (uint64_t t = 0; t < h.T(); t++) n += 6ull * (uint64_t)s.pc_n[t];
  return n;
}
inline Layout layout(const Shape& h, const Small& s) {
  Layout l;
  l.tree_first.assign(h.T() + 1, 0);
  for (uint64_t t = 0; t < h.T(); t++) l.tree_first[t + 1] = l.tree_first[t] + (uint64_t)s.n_nodes[t];
  l.nodes = l.tree_first[h.T()];
  l.examples = (uint64_t)s.ex_count;
  uint64_t o = head_bytes(h, s) + 8;
  for (int k = 0; k < NODE_FIELDS; k++) { l.node_off[k] = o; o += l.nodes * NODE_SIZE[k]; }
  l.counters_off = o; o += 8ull * N_COUNTERS + 8;
  uint64_t es[EX_FIELDS];
  ex_sizes(h, es);
  for (int k = 0; k < EX_FIELDS; k++) { l.ex_off[k] = o; o += l.examples * es[k]; }
  l.end_off = o;
  l.total = o + 16;
  return l;
}

// ---- the steps the two large sections are streamed in (engine.hip, through ckpt_stream.hpp's pump) ------------------------------------
// one step: nodes [a, b) of the file's order (trees t0 .. t0 + nt - 1), or bytes [a, b) of example run `field`
struct Chunk { int field; uint64_t a, b; int t0, nt; };   // field < 0: nodes
// a chunk of cnt nodes takes 20 * cnt + 4 bytes of staging: six runs, every run on a 4-byte boundary
inline uint64_t chunk_nodes(uint64_t staging_bytes) { return (staging_bytes - 4) / 20; }
// the staging a save or load takes: what the caller allows, no more than the larger section needs, no less than 64 bytes
inline uint64_t staging_bytes(const Shape& h, const Layout& l, uint64_t allowed) {
  uint64_t es[EX_FIELDS], ex_most = 0;
  ex_sizes(h, es);
  for (uint64_t e : es) ex_most = std::max(ex_most, l.examples * e);
  return std::max<uint64_t>(std::min<uint64_t>(allowed, std::max<uint64_t>(l.nodes * 20 + 4, ex_most)), 64);
}
// the node section: whole trees while they fit the staging buffer; a tree that does not fit alone is cut by node range
inline std::vector<Chunk> node_chunks(const Layout& l, uint64_t staging) {
  std::vector<Chunk> out;
  const std::vector<uint64_t>& f = l.tree_first;
  const uint64_t capn = chunk_nodes(staging);
  const int T = (int)f.size() - 1;
  for (uint64_t n0 = 0; n0 < l.nodes;) {
    const int t0 = (int)(std::upper_bound(f.begin(), f.end(), n0) - f.begin()) - 1;   // the tree that holds node n0 (empty trees before it skipped)
    uint64_t n1 = std::min(n0 + capn, l.nodes);
    int t1 = (int)(std::upper_bound(f.begin(), f.end(), n1) - f.begin()) - 1;          // largest t with first[t] <= n1
    if (t1 > t0 + 65535) t1 = t0 + 65535;                                                // (a launch's grid holds so many trees)
    if (f[t1] > n0) n1 = f[t1];                                                          // end on a tree boundary when one lies inside
    const int last = (int)(std::lower_bound(f.begin(), f.end(), n1) - f.begin()) - 1;    // the tree that holds node n1 - 1
    out.push_back({-1, n0, n1, t0, std::min(last, T - 1) - t0 + 1});
    n0 = n1;
  }
  return out;
}
// the example section: run by run, in steps of the staging buffer rounded down to 16 bytes
inline std::vector<Chunk> example_chunks(const Shape& h, const Layout& l, uint64_t staging) {
  std::vector<Chunk> out;
  uint64_t es[EX_FIELDS];
  ex_sizes(h, es);
  const uint64_t step = staging & ~(uint64_t)15;
  for (int k = 0; k < EX_FIELDS; k++)
    for (uint64_t a = 0; a < l.examples * es[k]; a += step) out.push_back({k, a, std::min(a + step, l.examples * es[k]), 0, 0});
  return out;
}

// ---- validation of the small state (no file needed).  Returns "" or what is wrong. ----------------------------------------------------
inline std::string check_small(const Shape& h, const Small& s) {
  const int A = h.A(), mm = h.game.max_moves, S = (int)h.moves_stride, cells = h.cells();
  char buf[160];
  auto bad = [&](const char* what, uint64_t i, long long v) { snprintf(buf, sizeof(buf), "%s[%llu] = %lld", what, (unsigned long long)i, v); return std::string(buf); };
  auto colour = [](int v) { return v == AGZ_NONE || v == AGZ_BLACK || v == AGZ_WHITE; };
  auto flag = [](int v) { return v == 0 || v == 1; };
  auto move = [&](int v) { return v >= AGZ_RESIGN && v < A; };
  for (uint64_t g = 0; g < h.G(); g++) {
    for (int i = 0; i < cells; i++) if (!colour(s.board[g * h.cells_pad + i])) return bad("board", g, s.board[g * h.cells_pad + i]);
    for (uint64_t r = 0; r < h.ring; r++)
      for (int i = 0; i < cells; i++) if (!colour(s.ring[(g * h.ring + r) * h.cells_pad + i])) return bad("ring", g, s.ring[(g * h.ring + r) * h.cells_pad + i]);
    if (s.to_move[g] != AGZ_BLACK && s.to_move[g] != AGZ_WHITE) return bad("to_move", g, s.to_move[g]);
    if (s.ply[g] < 0 || s.ply[g] > mm) return bad("ply", g, s.ply[g]);
    if (s.passes[g] < 0) return bad("passes", g, s.passes[g]);
    if (s.pass_count[g] < 0) return bad("pass_count", g, s.pass_count[g]);
    if (!flag(s.ended[g])) return bad("ended", g, s.ended[g]);
    if (!colour(s.winner[g])) return bad("winner", g, s.winner[g]);
    if (!flag(s.a_is_black[g])) return bad("a_is_black", g, s.a_is_black[g]);
    if (!move(s.last_move[g])) return bad("last_move", g, s.last_move[g]);
    if (!std::isfinite(s.cap_b[g]) || !std::isfinite(s.cap_w[g])) return bad("cap_b/cap_w", g, 0);
    if (s.n_amoves[g] < 0 || s.n_amoves[g] > S) return bad("n_amoves", g, s.n_amoves[g]);
    if (s.hist_from[g] < 0 || s.hist_from[g] > mm) return bad("hist_from", g, s.hist_from[g]);
    for (int j = 0; j < s.ply[g]; j++) if (!move(s.moves[g * S + j])) return bad("moves", g, s.moves[g * S + j]);
    if (s.ex_last[g] < -1 || s.ex_last[g] >= s.ex_count) return bad("ex_last", g, s.ex_last[g]);
  }
  for (uint64_t t = 0; t < h.T(); t++) {
    const uint64_t g = t % h.G();
    if (s.n_nodes[t] < 0 || (uint64_t)s.n_nodes[t] >= MAX_NODES) return bad("n_nodes", t, s.n_nodes[t]);
    if (s.cur_pool[t] != 0 && s.cur_pool[t] != 1) return bad("cur_pool", t, s.cur_pool[t]);
    if (!flag(s.has_root[t]) || (s.has_root[t] && s.n_nodes[t] < 1)) return bad("has_root", t, s.has_root[t]);
    if (!flag(s.has_prev[t])) return bad("has_prev", t, s.has_prev[t]);
    if (s.prev_ply[t] < 0 || s.prev_ply[t] > mm || (s.has_prev[t] && s.prev_ply[t] > s.ply[g])) return bad("prev_ply", t, s.prev_ply[t]);
    if (!flag(s.stalled[t])) return bad("stalled", t, s.stalled[t]);
    if (!flag(s.overflow[t])) return bad("overflow", t, s.overflow[t]);
    if (s.pc_n[t] < 0 || s.pc_n[t] >= S) return bad("pc_n", t, s.pc_n[t]);
    for (int i = 0; i < cells; i++) if (!colour(s.prev_board[t * h.cells_pad + i])) return bad("prev_board", t, s.prev_board[t * h.cells_pad + i]);
  }
  if (s.ex_count < 0 || s.ex_count > 0x7fffffffll) return bad("ex_count", 0, (long long)s.ex_count);
  return "";
}

// one tree's links: a child block lies behind its parent, inside the live prefix, and belongs to one parent only
inline std::string check_tree(const Shape& h, uint64_t t, int64_t n, const float* prior, const float* bsum, const int32_t* kids_off, const int16_t* kids_n,
                              const int16_t* nmove, std::vector<uint8_t>& claimed) {
  char buf[160];
  auto bad = [&](const char* what, int64_t i, long long v) { snprintf(buf, sizeof(buf), "tree %llu: %s[%lld] = %lld", (unsigned long long)t, what, (long long)i, v); return std::string(buf); };
  claimed.assign((size_t)n, 0);
  const int A = h.A();
  for (int64_t i = 0; i < n; i++) {
    if (!std::isfinite(prior[i])) return bad("prior (not finite)", i, 0);
    if (!std::isfinite(bsum[i])) return bad("bsum (not finite)", i, 0);
    if (nmove[i] < AGZ_RESIGN || nmove[i] >= A) return bad("nmove", i, nmove[i]);
    const int64_t off = kids_off[i], kn = kids_n[i];
    if (kn < 0 || kn > A + 1) return bad("kids_n", i, kn);
    if (off == -1) { if (kn != 0) return bad("kids_n (no children)", i, kn); continue; }
    if (off <= i || off >= n) return bad("kids_off", i, off);
    if (kn < 1 || off + kn > n) return bad("kids_off + kids_n", i, off + kn);
    for (int64_t j = off; j < off + kn; j++) { if (claimed[(size_t)j]) return bad("kids_off (shared child block)", i, off); claimed[(size_t)j] = 1; }
  }
  return "";
}

// ---- writer -----------------------------------------------------------------------------------------------------------------------------
template <class V>
inline bool put(FILE* f, const V& v, uint64_t n) { return n == 0 || fwrite(v.data(), sizeof(v[0]), (size_t)n, f) == n; }
inline bool seek_to(FILE* f, uint64_t off) { return fseeko(f, (off_t)off, SEEK_SET) == 0; }

// magic .. per-tree section, and the node count.  The arrays must have the arena's full sizes.
inline bool write_head(FILE* f, const Shape& h, const Host& host, const Small& s, const Layout& l) {
  const uint32_t tail[5] = {h.n_games, h.lanes, h.cells_pad, h.ring, h.moves_stride};
  bool ok = fwrite("AGZARN01", 1, 8, f) == 8 && fwrite(&h.game, sizeof(h.game), 1, f) == 1 && fwrite(&h.mcts, sizeof(h.mcts), 1, f) == 1 &&
            fwrite(tail, 4, 5, f) == 5 && fwrite(&host.seed, 8, 1, f) == 1 && fwrite(&host.seed0, 8, 1, f) == 1 &&
            fwrite(&host.prep_expand_seen, 8, 1, f) == 1 && fwrite(&host.moves_done, 4, 1, f) == 1 && fwrite(&host.restart, 4, 1, f) == 1;
  each_game_array(s, h, [&](const auto& v, uint64_t per) { ok = ok && v.size() == h.G() * per && put(f, v, h.G() * per); });
  each_tree_array(s, h, [&](const auto& v, uint64_t per) { ok = ok && v.size() == h.T() * per && put(f, v, h.T() * per); });
  ok = ok && s.pc_hash.size() == h.T() * h.moves_stride && s.pc_move.size() == h.T() * h.moves_stride;
  for (uint64_t t = 0; ok && t < h.T(); t++) {
    const size_t n = (size_t)s.pc_n[t];
    ok = (n == 0 || (fwrite(&s.pc_hash[t * h.moves_stride], 4, n, f) == n && fwrite(&s.pc_move[t * h.moves_stride], 2, n, f) == n));
  }
  return ok && fwrite(&l.nodes, 8, 1, f) == 1;
}
// nodes [first, first + count) of the file's node order: run k of them is at runs[k]
inline bool write_nodes(FILE* f, const Layout& l, uint64_t first, uint64_t count, const void* const runs[NODE_FIELDS]) {
  for (int k = 0; k < NODE_FIELDS; k++)
    if (count && !(seek_to(f, l.node_off[k] + first * NODE_SIZE[k]) && fwrite(runs[k], NODE_SIZE[k], (size_t)count, f) == count)) return false;
  return true;
}
inline bool write_counters(FILE* f, const Layout& l, const Small& s) {
  return seek_to(f, l.counters_off) && fwrite(s.counters, 8, N_COUNTERS, f) == N_COUNTERS && fwrite(&l.examples, 8, 1, f) == 1;
}
// bytes [first, first + count) of example run k
inline bool write_examples(FILE* f, const Layout& l, int k, uint64_t first, uint64_t count, const void* bytes) {
  return count == 0 || (seek_to(f, l.ex_off[k] + first) && fwrite(bytes, 1, (size_t)count, f) == count);
}
inline bool write_end(FILE* f, const Layout& l) {
  return seek_to(f, l.end_off) && fwrite("AGZARNZZ", 1, 8, f) == 8 && fwrite(&l.total, 8, 1, f) == 1;
}

// ---- reader ---------------------------------------------------------------------------------------------------------------------------
enum Status {
  OK = 0,
  NOT_ARENA,   // no arena checkpoint, or of a build with other constants
  MISMATCH,    // of another game / search configuration or game count (why names the field)
  BROKEN       // truncated, too long, or inconsistent
};
struct Scan { Host host; Small small; Layout lay; uint64_t most = 0; };   // most: the fullest tree's node count

template <class V>
inline bool get(FILE* f, V& v, uint64_t n) { v.resize((size_t)n); return n == 0 || fread(v.data(), sizeof(v[0]), (size_t)n, f) == n; }
inline bool read_nodes(FILE* f, const Layout& l, uint64_t first, uint64_t count, void* const runs[NODE_FIELDS]) {
  for (int k = 0; k < NODE_FIELDS; k++)
    if (count && !(seek_to(f, l.node_off[k] + first * NODE_SIZE[k]) && fread(runs[k], NODE_SIZE[k], (size_t)count, f) == count)) return false;
  return true;
}
inline bool read_examples(FILE* f, const Layout& l, int k, uint64_t first, uint64_t count, void* bytes) {
  return count == 0 || (seek_to(f, l.ex_off[k] + first) && fread(bytes, 1, (size_t)count, f) == count);
}

// `want`: the loading arena (lanes is not compared).  The whole file is read and checked; *why says what was wrong.
inline Status scan(FILE* f, const Shape& want, Scan* out, std::string* why) {
  char buf[200];
  auto fail = [&](Status st, const std::string& w) { *why = w; return st; };
  if (fseeko(f, 0, SEEK_END) != 0) return fail(NOT_ARENA, "cannot seek");
  const int64_t len = (int64_t)ftello(f);
  char magic[8];
  Shape h = want;
  uint32_t tail[5];
  if (len < 0 || !seek_to(f, 0) || fread(magic, 1, 8, f) != 8 || memcmp(magic, "AGZARN01", 8) != 0) return fail(NOT_ARENA, "not an arena checkpoint (magic)");
  if (fread(&h.game, sizeof(h.game), 1, f) != 1 || fread(&h.mcts, sizeof(h.mcts), 1, f) != 1 || fread(tail, 4, 5, f) != 5) return fail(BROKEN, "truncated inside the configuration");
  h.n_games = tail[0]; h.lanes = tail[1]; h.cells_pad = tail[2]; h.ring = tail[3]; h.moves_stride = tail[4];
  if (h.cells_pad != want.cells_pad || h.ring != want.ring) {
    snprintf(buf, sizeof(buf), "written by a build with other constants (CELLS_PAD %u, RING %u; this build %u, %u)", h.cells_pad, h.ring, want.cells_pad, want.ring);
    return fail(NOT_ARENA, buf);
  }
#define AGZ_ARN_SAME(field, fmt, cast)                                                                                        \
  if (memcmp(&h.field, &want.field, sizeof(h.field)) != 0) {                                                                  \
    snprintf(buf, sizeof(buf), "%s differs: the file has " fmt ", this arena " fmt, #field, (cast)h.field, (cast)want.field); \
    return fail(MISMATCH, buf);                                                                                               \
  }
  AGZ_ARN_SAME(n_games, "%d", int)
  AGZ_ARN_SAME(game.kind, "%d", int) AGZ_ARN_SAME(game.m, "%d", int) AGZ_ARN_SAME(game.n, "%d", int) AGZ_ARN_SAME(game.k, "%d", int)
  AGZ_ARN_SAME(game.komi, "%g", double) AGZ_ARN_SAME(game.max_moves, "%d", int) AGZ_ARN_SAME(game.encoder, "%d", int)
  AGZ_ARN_SAME(mcts.PUCT, "%g", double) AGZ_ARN_SAME(mcts.M, "%d", int) AGZ_ARN_SAME(mcts.N, "%d", int) AGZ_ARN_SAME(mcts.RandomCount, "%d", int)
  AGZ_ARN_SAME(mcts.Budget, "%d", int) AGZ_ARN_SAME(mcts.RandomMinVisits, "%d", int) AGZ_ARN_SAME(mcts.RandomTemperature, "%g", double)
  AGZ_ARN_SAME(mcts.DumbPass, "%d", int) AGZ_ARN_SAME(mcts.ResignPercentage, "%g", double) AGZ_ARN_SAME(mcts.PassPreference, "%d", int)
  AGZ_ARN_SAME(moves_stride, "%d", int)
#undef AGZ_ARN_SAME
  Host& host = out->host;
  Small& s = out->small;
  bool ok = fread(&host.seed, 8, 1, f) == 1 && fread(&host.seed0, 8, 1, f) == 1 && fread(&host.prep_expand_seen, 8, 1, f) == 1 &&
            fread(&host.moves_done, 4, 1, f) == 1 && fread(&host.restart, 4, 1, f) == 1;
  if (ok && (host.restart > 1 || host.moves_done < 0)) return fail(BROKEN, "host scalars out of range");
  each_game_array(s, h, [&](auto& v, uint64_t per) { ok = ok && get(f, v, h.G() * per); });
  each_tree_array(s, h, [&](auto& v, uint64_t per) { ok = ok && get(f, v, h.T() * per); });
  if (!ok) return fail(BROKEN, "truncated inside the per-game or per-tree state");
  s.pc_hash.assign((size_t)(h.T() * h.moves_stride), 0); s.pc_move.assign((size_t)(h.T() * h.moves_stride), 0);
  for (uint64_t t = 0; t < h.T(); t++) {
    if (s.pc_n[t] < 0 || s.pc_n[t] >= (int)h.moves_stride) { snprintf(buf, sizeof(buf), "pc_n[%llu] = %d", (unsigned long long)t, s.pc_n[t]); return fail(BROKEN, buf); }
    const size_t n = (size_t)s.pc_n[t];
    if (n && (fread(&s.pc_hash[t * h.moves_stride], 4, n, f) != n || fread(&s.pc_move[t * h.moves_stride], 2, n, f) != n)) return fail(BROKEN, "truncated inside the cached policies");
  }
  // the counts the rest of the layout follows from: the node count must be the sum of n_nodes, the example count is read where it lies
  uint64_t nodes = 0;
  if (fread(&nodes, 8, 1, f) != 1) return fail(BROKEN, "truncated before the nodes");
  for (uint64_t t = 0; t < h.T(); t++)
    if (s.n_nodes[t] < 0 || (uint64_t)s.n_nodes[t] >= MAX_NODES) { snprintf(buf, sizeof(buf), "n_nodes[%llu] = %d", (unsigned long long)t, s.n_nodes[t]); return fail(BROKEN, buf); }
  s.ex_count = 0;
  Layout l = layout(h, s);
  if (nodes != l.nodes) return fail(BROKEN, "the node count is not the sum of n_nodes");
  uint64_t ex = 0;
  if ((uint64_t)len < l.counters_off + 8ull * N_COUNTERS + 8 || !seek_to(f, l.counters_off) || fread(s.counters, 8, N_COUNTERS, f) != N_COUNTERS || fread(&ex, 8, 1, f) != 1)
    return fail(BROKEN, "truncated inside the nodes or counters");
  if (ex > 0x7fffffffull) return fail(BROKEN, "ex_count out of range");
  s.ex_count = (int64_t)ex;
  l = layout(h, s);
  out->lay = l;
  if ((uint64_t)len != l.total) { snprintf(buf, sizeof(buf), "truncated or overlong: the file is %lld bytes long, its counts say %llu", (long long)len, (unsigned long long)l.total); return fail(BROKEN, buf); }
  char endm[8];
  uint64_t total = 0;
  if (!seek_to(f, l.end_off) || fread(endm, 1, 8, f) != 8 || fread(&total, 8, 1, f) != 1 || memcmp(endm, "AGZARNZZ", 8) != 0 || total != l.total) return fail(BROKEN, "bad end marker");
  std::string w = check_small(h, s);
  if (!w.empty()) return fail(BROKEN, w);
  // the nodes, tree by tree
  std::vector<float> prior, bsum;
  std::vector<uint32_t> visits;
  std::vector<int32_t> koff;
  std::vector<int16_t> kn, nm;
  std::vector<uint8_t> claimed;
  out->most = 0;
  for (uint64_t t = 0; t < h.T(); t++) {
    const uint64_t n = (uint64_t)s.n_nodes[t];
    out->most = std::max(out->most, n);
    if (!n) continue;
    prior.resize(n); visits.resize(n); bsum.resize(n); koff.resize(n); kn.resize(n); nm.resize(n);
    void* runs[NODE_FIELDS] = {prior.data(), visits.data(), bsum.data(), koff.data(), kn.data(), nm.data()};
    if (!read_nodes(f, l, l.tree_first[t], n, runs)) return fail(BROKEN, "reading the nodes failed");
    w = check_tree(h, t, (int64_t)n, prior.data(), bsum.data(), koff.data(), kn.data(), nm.data(), claimed);
    if (!w.empty()) return fail(BROKEN, w);
  }
  // the example links: game in [0, G), prev an EARLIER row or -1, labelled a flag, value finite
  const uint64_t E = l.examples, BLK = 1 << 16;
  std::vector<int32_t> eg(BLK), ep(BLK);
  std::vector<uint8_t> el(BLK);
  std::vector<float> ev(BLK);
  for (uint64_t e0 = 0; e0 < E; e0 += BLK) {
    const uint64_t n = std::min(BLK, E - e0);
    if (!read_examples(f, l, 2, e0 * 4, n * 4, ev.data()) || !read_examples(f, l, 3, e0 * 4, n * 4, eg.data()) || !read_examples(f, l, 4, e0 * 4, n * 4, ep.data()) ||
        !read_examples(f, l, 5, e0, n, el.data()))
      return fail(BROKEN, "reading the examples failed");
    for (uint64_t i = 0; i < n; i++) {
      const int64_t e = (int64_t)(e0 + i);
      if (eg[i] < 0 || (uint64_t)eg[i] >= h.G()) { snprintf(buf, sizeof(buf), "ex_game[%lld] = %d", (long long)e, eg[i]); return fail(BROKEN, buf); }
      if (ep[i] < -1 || ep[i] >= e) { snprintf(buf, sizeof(buf), "ex_prev[%lld] = %d", (long long)e, ep[i]); return fail(BROKEN, buf); }
      if (el[i] > 1) { snprintf(buf, sizeof(buf), "ex_labelled[%lld] = %d", (long long)e, el[i]); return fail(BROKEN, buf); }
      if (!std::isfinite(ev[i])) { snprintf(buf, sizeof(buf), "ex_value[%lld] is not finite", (long long)e); return fail(BROKEN, buf); }
    }
  }
  return OK;
}

}  // namespace arena_ckpt
}  // namespace agz
