// Root visit counts as policy targets (agz_arena_set_policy_target, DESIGN.md §2 visit-target).  ONE definition for host and device:
// k_end_move (engine.hip), the host function agz_visit_target_of, and a plain g++ check (tests/cpp/target_check.cpp).
//
// pi(a) ~ N(a)^(1/tau) over the root's children, as a row of A + 1 floats (the last entry is Pass).  Like noise.hpp, whose ln_b / exp_b
// it reuses: IEEE double + - * / (each rounded once), integer and bit operations, contraction off.  The weights are 64-bit INTEGERS, so
// their sum is exact and the row depends neither on the order of the child block (fancySort and randomizeChildren reorder it in the
// kernel that writes the row) nor on how a wavefront reduces the sum.
//
//   Nmax       max N_i;  Nmax == 0: no target
//   w_i        tau == 1: N_i;  else 2^40 if N_i == Nmax, 0 if N_i == 0, else (uint64)(exp_b(ln_b((double)N_i / (double)Nmax) / tau) * 2^40)
//   S          sum of w_i, exact (below 2^53 for up to 4096 children)
//   row[idx]   (float)((double)w_i / (double)S), idx = the move, A for Pass;  every other entry +0.0f
#pragma once
#include <cstdint>

#include "noise.hpp"

namespace agz {
namespace target {

constexpr int MAX_N = 4096;           // agz_visit_target_of's largest n and action space
constexpr int PASS = -1;              // AGZ_PASS
constexpr uint64_t ONE = 1ull << 40;  // the weight of a child with Nmax visits when tau != 1

// w_i; tau is the double of the float setting, nmax >= 1
AGZ_NOISE_HD uint64_t weight(uint32_t n, uint32_t nmax, double tau) {
  AGZ_NOISE_NOFMA
  if (tau == 1.0) return (uint64_t)n;
  if (n == nmax) return ONE;
  if (n == 0) return 0;
  const double r = (double)n / (double)nmax;
  return (uint64_t)(noise::exp_b(noise::ln_b(r) / tau) * 1099511627776.0);   // y < 0: exp_b <= 1, the product is in [0, 2^40]
}

AGZ_NOISE_HD float entry(uint64_t w, uint64_t S) {
  AGZ_NOISE_NOFMA
  return (float)((double)w / (double)S);
}

// the row index of a child's move: a board move is its own index, Pass is the last entry
AGZ_NOISE_HD int index_of(int move, int A) { return move == PASS ? A : move; }

// the whole row on one thread (the host function; the kernel spreads the children over a wavefront).  false: Nmax == 0, row untouched
AGZ_NOISE_HD bool row_of(const int32_t* moves, const uint32_t* visits, int n, int A, double tau, float* row) {
  uint32_t nmax = 0;
  for (int i = 0; i < n; i++) nmax = visits[i] > nmax ? visits[i] : nmax;
  if (nmax == 0) return false;
  uint64_t S = 0;
  for (int i = 0; i < n; i++) S += weight(visits[i], nmax, tau);
  for (int a = 0; a <= A; a++) row[a] = 0.0f;
  for (int i = 0; i < n; i++) row[index_of(moves[i], A)] = entry(weight(visits[i], nmax, tau), S);
  return true;
}

}  // namespace target
}  // namespace agz
