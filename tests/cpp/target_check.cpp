// Plain g++ check of agogo_amd/csrc/target.hpp (no HIP): the visit-count policy target on the code the kernel compiles.  Driven by
// tests/test_policy_target_cpu.py, which builds this file at -O0 and at -O2 and requires the same output from both, then recomputes every
// line with its pure-Python restatement.  Output, all floating-point values as hexadecimal bit patterns:
//   w <n> <nmax> <tau float bits> <weight>
//   row <A> <tau float bits> <n> <move_0> .. <move_{n-1}> <visits_0> .. <visits_{n-1}> <row_0 bits> .. <row_A bits>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../agogo_amd/csrc/target.hpp"

using namespace agz;

static uint32_t fbits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

int main() {
  uint64_t s = 20261021;
  const float taus[] = {1.0f, 0.5f, 0.25f, 2.0f, 0.03f, 1.5f, 100.0f};
  for (float tau : taus) {
    for (int i = 0; i < 40; i++) {
      uint32_t nmax = i < 20 ? 1u + (uint32_t)(noise::next(s) % 800) : (uint32_t)(noise::next(s) >> 32) | 1u;
      uint32_t n = (uint32_t)(noise::next(s) % ((uint64_t)nmax + 1));
      if (i == 0) { nmax = 16777215u; n = 16777214u; }
      if (i == 1) { nmax = 4294967295u; n = 1u; }
      if (i == 2) { nmax = 4294967295u; n = 4294967294u; }
      printf("w %u %u %08x %" PRIu64 "\n", n, nmax, fbits(tau), target::weight(n, nmax, (double)tau));
    }
  }
  const struct { int A, n, pass; } cases[] = {{9, 1, 0}, {9, 9, 0}, {25, 26, 1}, {81, 82, 1}, {361, 362, 1}, {7, 5, 1}, {42, 17, 0}};
  for (const auto& c : cases) {
    for (float tau : taus) {
      for (int rep = 0; rep < 3; rep++) {
        // moves: a shuffled choice of n of the A cells (Pass takes the place of the last one), visits: Budget-like counts with zeros and ties
        std::vector<int32_t> cells(c.A), mv(c.n);
        for (int i = 0; i < c.A; i++) cells[i] = i;
        for (int i = c.A - 1; i > 0; i--) { const int j = (int)(noise::next(s) % (uint64_t)(i + 1)); const int32_t t = cells[i]; cells[i] = cells[j]; cells[j] = t; }
        for (int i = 0; i < c.n; i++) mv[i] = c.pass && i == c.n - 1 ? target::PASS : cells[i];
        if (c.n > 1) { const int j = (int)(noise::next(s) % (uint64_t)c.n); const int32_t t = mv[j]; mv[j] = mv[c.n - 1]; mv[c.n - 1] = t; }
        std::vector<uint32_t> vis(c.n);
        for (int i = 0; i < c.n; i++) {
          const uint64_t z = noise::next(s);
          vis[i] = rep == 0 ? (uint32_t)(z % 100) : (rep == 1 ? (uint32_t)(z % 4) * 7u : (uint32_t)(z % 5 == 0 ? 0 : z % 16777216));
        }
        if (rep == 2) vis[0] = 16777215u;
        vis[(size_t)(noise::next(s) % (uint64_t)c.n)] |= 1u;   // never all zero
        std::vector<float> row(c.A + 1, -1.0f);
        if (!target::row_of(mv.data(), vis.data(), c.n, c.A, (double)tau, row.data())) { printf("no target\n"); return 1; }
        printf("row %d %08x %d", c.A, fbits(tau), c.n);
        for (int i = 0; i < c.n; i++) printf(" %d", mv[i]);
        for (int i = 0; i < c.n; i++) printf(" %u", vis[i]);
        for (int a = 0; a <= c.A; a++) printf(" %08x", fbits(row[a]));
        printf("\n");
      }
    }
  }
  {  // Nmax == 0: no target, the row is left alone
    const int32_t mv[2] = {0, 1};
    const uint32_t vis[2] = {0, 0};
    float row[4] = {-1.0f, -1.0f, -1.0f, -1.0f};
    if (target::row_of(mv, vis, 2, 3, 1.0, row) || row[0] != -1.0f || row[3] != -1.0f) { printf("a target without visits\n"); return 1; }
  }
  printf("TARGET OK\n");
  return 0;
}
