// Forced playouts and policy-target pruning at the root (agz_arena_set_forced_playouts, DESIGN.md §2 forced-playouts).  ONE definition
// for host and device: select_child and k_end_move (engine.hip), the host functions agz_root_select_of and agz_pruned_target_of, and a
// plain g++ check (tests/cpp/forced_check.cpp).
//
// Like noise.hpp and target.hpp: IEEE float and double + - * / (each rounded once), integer operations, contraction off.  The one square
// root of PUCT's numerator is handed in: the device computes it with sqrt_cr (engine.hip), the host with sqrtf, both correctly rounded.
// The root's children i = 0..n-1 as they stand in the child block:
//
//   N_i, n_i     stored visits (>= 1: a child is created with visits = 1) and playouts n_i = N_i - 1
//   B_i, P_i     the stored score sum and the stored prior (root noise, if on, is already in it)
//   pv, T        sum of N_i; sum of n_i = pv - n
//   q_i          evaluate(B_i, N_i, player): B_i / N_i, for White 1 - that
//   U(i, m)      fadd(q_i, fmul(fmul(PUCT, P_i), fdiv(num, fadd(1.0f, (float)m)))), num = sqrt((float)pv) correctly rounded;
//                U(i, N_i) is Node.Select's usa
//   rhs_i        ((double)k * (double)P_i) * (double)T
//
// Forced selection (the root of a descent only): child i is forced iff n_i >= 1 and (double)(n_i + mark_i)^2 < rhs_i, mark_i the child's
// stored virtual-loss mark in a lane round (0 in the sequential search).  A forced child's usa is +INFINITY: the argmax and its tie rule
// (first maximum, lowest block index) pick the lowest-index forced child.  k = 0 forces nothing.
//
// Pruned target: c* = the child with the largest N_i (ties: the smallest move as an int, so Pass = -1 first), U* = U(c*, N_c*).
//   F_i          the largest integer f >= 0 with (double)f * (double)f <= rhs_i (only min(F_i, n_i) matters)
//   n'_i         i == c*: n_i;  n_i == 0: 0;  else with lo = N_i - min(F_i, n_i): N'_i = the smallest m in [lo, N_i] with U(i, m) < U*
//                (N_i if U(i, N_i) >= U*; U does not increase with m because no float operation in it does), n'_i = N'_i - 1, and a child
//                reduced to a single playout is pruned outright: N'_i < N_i and n'_i == 1 gives n'_i = 0.  q_i, pv and U* stay fixed.
//   row          target::row_of(moves, n', A, tau); n_c* == 0: no row
#pragma once
#include <cmath>
#include <cstdint>

#include "target.hpp"

namespace agz {
namespace forced {

constexpr int MAX_N = 4096;   // the host functions' largest n and action space
constexpr int WHITE = 2;      // AGZ_WHITE

// one float operation, rounded once: the device's round-to-nearest intrinsics (what select_child is written in), the host's operators
#if defined(__HIP_DEVICE_COMPILE__)
AGZ_NOISE_HD float fadd(float a, float b) { return __fadd_rn(a, b); }
AGZ_NOISE_HD float fsub(float a, float b) { return __fsub_rn(a, b); }
AGZ_NOISE_HD float fmul(float a, float b) { return __fmul_rn(a, b); }
AGZ_NOISE_HD float fdiv(float a, float b) { return __fdiv_rn(a, b); }
#else
AGZ_NOISE_HD float fadd(float a, float b) { AGZ_NOISE_NOFMA return a + b; }
AGZ_NOISE_HD float fsub(float a, float b) { AGZ_NOISE_NOFMA return a - b; }
AGZ_NOISE_HD float fmul(float a, float b) { AGZ_NOISE_NOFMA return a * b; }
AGZ_NOISE_HD float fdiv(float a, float b) { AGZ_NOISE_NOFMA return a / b; }
#endif

// Evaluate (mcts/node.go:147-159)
AGZ_NOISE_HD float evaluate(float bs, uint32_t visits, int player) {
  float score = fdiv(bs, (float)visits);
  if (player == WHITE) score = fsub(1.0f, score);
  return score;
}

// U(i, m) from q_i, P_i and the numerator sqrt((float)pv)
AGZ_NOISE_HD float U(float q, float prior, float PUCT, float num, uint32_t m) {
  const float denominator = fadd(1.0f, (float)m);
  const float lastTerm = fdiv(num, denominator);
  const float puct = fmul(fmul(PUCT, prior), lastTerm);
  return fadd(q, puct);
}

AGZ_NOISE_HD double rhs(double k, float prior, uint32_t T) {
  AGZ_NOISE_NOFMA
  return (k * (double)prior) * (double)T;
}

// the forced rule for a child with `visits` stored visits and a virtual-loss mark of 0 or 1
AGZ_NOISE_HD bool is_forced(uint32_t visits, uint32_t mark, double r) {
  AGZ_NOISE_NOFMA
  if (visits < 2) return false;   // no playout yet (visits == 0 is no child of a root)
  const double m = (double)(visits - 1u) + (double)mark;
  return m * m < r;
}

// min(F_i, n_i): any estimate, then an integer fix-up against the double products the definition names
AGZ_NOISE_HD uint32_t fmin_of(double r, uint32_t ni) {
  AGZ_NOISE_NOFMA
  if (!(r > 0.0)) return 0;
  if ((double)ni * (double)ni <= r) return ni;
#if defined(__HIP_DEVICE_COMPILE__)
  const float e = __builtin_amdgcn_sqrtf((float)r);
#else
  const float e = sqrtf((float)r);
#endif
  uint32_t f = e >= (float)ni ? ni : (uint32_t)e;   // r < ni^2 < 2^64
  while (f > 0 && (double)f * (double)f > r) f--;
  while (f < ni && (double)(f + 1u) * (double)(f + 1u) <= r) f++;
  return f;
}

// n'_i of a child that is not c*
AGZ_NOISE_HD uint32_t pruned_playouts(uint32_t visits, float bs, float prior, int player, float PUCT, float num, double k, uint32_t T, float ustar) {
  if (visits < 2) return 0;
  const float q = evaluate(bs, visits, player);
  if (!(U(q, prior, PUCT, num, visits) < ustar)) return visits - 1u;
  uint32_t lo = visits - fmin_of(rhs(k, prior, T), visits - 1u), hi = visits;   // U(i, hi) < U* holds
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (U(q, prior, PUCT, num, mid) < ustar) hi = mid; else lo = mid + 1u;
  }
  const uint32_t np = hi - 1u;
  return (hi < visits && np == 1u) ? 0u : np;
}

// does child (visits a, move ma) come before child (visits b, move mb) as c*
AGZ_NOISE_HD bool star_before(uint32_t a, int ma, uint32_t b, int mb) { return a > b || (a == b && ma < mb); }

// ---- the whole block on one thread, host only (the host functions; the kernels spread the children over a wavefront) ----

inline uint32_t parent_visits(const uint32_t* visits, int n) {
  uint32_t pv = 0;
  for (int i = 0; i < n; i++) pv += visits[i];
  return pv;
}

// Node.Select over the root's block with the forced rule; marks may be nullptr (the sequential search: no mark, no +3.0 term).
// Returns the block index (-1: no child compares greater than -inf), *forced = 1 iff the chosen child was forced.
inline int select_of(const uint32_t* visits, const float* bsum, const float* prior, const uint8_t* marks, int n, int player, float PUCT, float k, int* forced_out) {
  const uint32_t pv = parent_visits(visits, n);
  const float num = sqrtf((float)pv);
  const uint32_t T = pv - (uint32_t)n;
  float best = -INFINITY;
  int idx = -1, f = 0;
  for (int i = 0; i < n; i++) {
    float bs = bsum[i];
    if (marks && player == WHITE) bs = fadd(bs, marks[i] ? 3.0f : 0.0f);
    float usa = U(evaluate(bs, visits[i], player), prior[i], PUCT, num, visits[i]);
    const bool fc = k > 0.f && is_forced(visits[i], marks && marks[i] ? 1u : 0u, rhs((double)k, prior[i], T));
    if (fc) usa = INFINITY;
    if (usa > best) { best = usa; idx = i; f = fc ? 1 : 0; }
  }
  if (forced_out) *forced_out = f;
  return idx;
}

// n' of every child and the row; false: n_c* == 0, nothing written.  np_out may be nullptr, scratch holds n words
inline bool pruned_row_of(const int32_t* moves, const uint32_t* visits, const float* bsum, const float* prior, int n, int A, int player, float PUCT, float k,
                          double tau, uint32_t* scratch, uint32_t* np_out, float* row) {
  int cs = 0;
  for (int i = 1; i < n; i++) if (star_before(visits[i], moves[i], visits[cs], moves[cs])) cs = i;
  if (visits[cs] < 2) return false;
  const uint32_t pv = parent_visits(visits, n);
  const float num = sqrtf((float)pv);
  const uint32_t T = pv - (uint32_t)n;
  const float ustar = U(evaluate(bsum[cs], visits[cs], player), prior[cs], PUCT, num, visits[cs]);
  for (int i = 0; i < n; i++)
    scratch[i] = i == cs ? visits[i] - 1u : pruned_playouts(visits[i], bsum[i], prior[i], player, PUCT, num, (double)k, T, ustar);
  target::row_of(moves, scratch, n, A, tau, row);
  if (np_out) for (int i = 0; i < n; i++) np_out[i] = scratch[i];
  return true;
}

}  // namespace forced
}  // namespace agz
