// The window digest of agogo_amd/csrc/replay.hpp under a plain C++ compiler (tests/test_replay_sharded_cpu.py builds this with
// g++ -Wall -Werror): prints the digest of a few fixed row sets, which the test recomputes with Python integers.
//   pattern(i) = 0x80000000 (-0.0) if i % 7 == 3, 0x7FC00123 (a NaN) if i % 11 == 5, else (i * 2654435761 + 12345) mod 2^32
//   planes[j][e] = pattern(j * xs + e), policy[j][e] = pattern(1000 + j * A1 + e), value[j] = pattern(2000 + j)
#include <cstdio>
#include <vector>

#include "../../agogo_amd/csrc/replay.hpp"

static uint32_t pattern(uint64_t i) {
  if (i % 7 == 3) return 0x80000000u;
  if (i % 11 == 5) return 0x7FC00123u;
  return (uint32_t)(i * 2654435761ull + 12345ull);
}

int main() {
  using namespace agz::replay;
  if (mix64(GAMMA) != OUT_0_0 || out(0, 0) != OUT_0_0) { printf("mix64 is not the finaliser of out()\n"); return 1; }
  const uint64_t NS[] = {0, 1, 5}, XS[] = {1, 18, 25}, AS[] = {1, 10};
  for (uint64_t n : NS)
    for (uint64_t xs : XS)
      for (uint64_t A1 : AS) {
        std::vector<uint32_t> p(n * xs + 1), q(n * A1 + 1), v(n + 1);
        for (uint64_t j = 0; j < n; j++) {
          for (uint64_t e = 0; e < xs; e++) p[j * xs + e] = pattern(j * xs + e);
          for (uint64_t e = 0; e < A1; e++) q[j * A1 + e] = pattern(1000 + j * A1 + e);
          v[j] = pattern(2000 + j);
        }
        const uint64_t d = digest_rows(p.data(), q.data(), v.data(), n, xs, A1);
        // the same sum term by term, in the reverse order: an integer sum does not depend on it
        uint64_t rev = n;
        const uint64_t rowlen = xs + A1 + 1;
        for (uint64_t j = n; j-- > 0;)
          for (uint64_t e = rowlen; e-- > 0;)
            rev += digest_term(j, rowlen, e, e < xs ? p[j * xs + e] : e < xs + A1 ? q[j * A1 + (e - xs)] : v[j]);
        if (rev != d) { printf("the digest depends on the order of the sum\n"); return 1; }
        printf("digest %llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)xs, (unsigned long long)A1, (unsigned long long)d);
      }
  printf("DIGEST OK\n");
  return 0;
}
