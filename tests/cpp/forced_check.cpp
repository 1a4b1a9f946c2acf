// Plain g++ check of agogo_amd/csrc/forced.hpp (no HIP): forced playouts and the pruned policy target on the code the kernels compile.
// Driven by tests/test_forced_playouts_cpu.py, which builds this file at -O0 and at -O2 and requires the same output from both, then
// recomputes every line with its pure-Python restatement.  Output, all floating-point values as hexadecimal bit patterns:
//   sel <player> <puct> <k> <has marks> <n> <visits> x n <score sums> x n <priors> x n <marks> x n <index> <forced>
//   prn <A> <player> <puct> <k> <tau> <n> <moves> x n <visits> x n <score sums> x n <priors> x n <n'> x n <row> x (A + 1)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../agogo_amd/csrc/forced.hpp"

using namespace agz;

static uint32_t fbits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float u01f(uint64_t& s) { return (float)(noise::next(s) >> 40) * (1.0f / 16777216.0f); }

int main() {
  uint64_t s = 20261022;
  const float ks[] = {0.0f, 0.5f, 2.0f, 8.0f};
  const float taus[] = {1.0f, 0.5f, 2.0f};
  const struct { int A, n, pass; } cases[] = {{9, 1, 0}, {9, 9, 0}, {7, 7, 0}, {25, 26, 1}, {81, 82, 1}, {361, 362, 1}, {42, 17, 0}};
  for (const auto& c : cases) {
    for (int rep = 0; rep < 12; rep++) {
      const float k = ks[rep % 4], tau = taus[rep % 3], puct = rep % 5 == 0 ? 1.0f : 0.75f;
      const int player = 1 + (rep & 1);
      std::vector<int32_t> cells(c.A), mv(c.n);
      for (int i = 0; i < c.A; i++) cells[i] = i;
      for (int i = c.A - 1; i > 0; i--) { const int j = (int)(noise::next(s) % (uint64_t)(i + 1)); const int32_t t = cells[i]; cells[i] = cells[j]; cells[j] = t; }
      for (int i = 0; i < c.n; i++) mv[i] = c.pass && i == c.n - 1 ? target::PASS : cells[i];
      if (c.n > 1) { const int j = (int)(noise::next(s) % (uint64_t)c.n); const int32_t t = mv[j]; mv[j] = mv[c.n - 1]; mv[c.n - 1] = t; }
      // visits: what a search leaves (most children near 1, a few large), with ties at the top in every third block; priors: a
      // normalised random vector, or all equal; score sums: a value in (-1, 1) per visit
      std::vector<uint32_t> vis(c.n);
      std::vector<float> bs(c.n), pr(c.n);
      std::vector<uint8_t> mk(c.n);
      float psum = 0.f;
      for (int i = 0; i < c.n; i++) {
        const uint64_t z = noise::next(s);
        vis[i] = z % 4 == 0 ? 1u + (uint32_t)((z >> 8) % 2000) : 1u + (uint32_t)((z >> 8) % 6);
        pr[i] = rep % 4 == 3 ? 1.0f : u01f(s) * u01f(s) + 1e-4f;
        psum += pr[i];
        mk[i] = noise::next(s) % 5 == 0 ? 1 : 0;
      }
      if (rep % 3 == 1 && c.n > 1) { vis[0] = 1500u; vis[c.n - 1] = 1500u; for (int i = 1; i < c.n - 1; i++) if (vis[i] > 1500u) vis[i] = 1500u; }
      for (int i = 0; i < c.n; i++) { pr[i] = pr[i] / psum; bs[i] = (float)vis[i] * (2.0f * u01f(s) - 1.0f); }
      for (int with_marks = 0; with_marks < 2; with_marks++) {
        int forced_flag = -1;
        const int idx = forced::select_of(vis.data(), bs.data(), pr.data(), with_marks ? mk.data() : nullptr, c.n, player, puct, k, &forced_flag);
        printf("sel %d %08x %08x %d %d", player, fbits(puct), fbits(k), with_marks, c.n);
        for (int i = 0; i < c.n; i++) printf(" %u", vis[i]);
        for (int i = 0; i < c.n; i++) printf(" %08x", fbits(bs[i]));
        for (int i = 0; i < c.n; i++) printf(" %08x", fbits(pr[i]));
        for (int i = 0; i < c.n; i++) printf(" %d", (int)mk[i]);
        printf(" %d %d\n", idx, forced_flag);
      }
      std::vector<uint32_t> scratch(c.n), np(c.n, 0xFFFFFFFFu);
      std::vector<float> row(c.A + 1, -1.0f);
      uint32_t nmax = 0;
      for (int i = 0; i < c.n; i++) nmax = vis[i] > nmax ? vis[i] : nmax;
      const bool ok = forced::pruned_row_of(mv.data(), vis.data(), bs.data(), pr.data(), c.n, c.A, player, puct, k, (double)tau, scratch.data(), np.data(), row.data());
      if (ok != (nmax >= 2)) { printf("a row without a playout, or none with one\n"); return 1; }
      if (!ok) { if (row[0] != -1.0f || np[0] != 0xFFFFFFFFu) { printf("a refused block was written\n"); return 1; } continue; }
      printf("prn %d %d %08x %08x %08x %d", c.A, player, fbits(puct), fbits(k), fbits(tau), c.n);
      for (int i = 0; i < c.n; i++) printf(" %d", mv[i]);
      for (int i = 0; i < c.n; i++) printf(" %u", vis[i]);
      for (int i = 0; i < c.n; i++) printf(" %08x", fbits(bs[i]));
      for (int i = 0; i < c.n; i++) printf(" %08x", fbits(pr[i]));
      for (int i = 0; i < c.n; i++) printf(" %u", np[i]);
      for (int a = 0; a <= c.A; a++) printf(" %08x", fbits(row[a]));
      printf("\n");
    }
  }
  printf("FORCED OK\n");
  return 0;
}
