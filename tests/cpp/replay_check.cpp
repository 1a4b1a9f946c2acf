// Plain g++ check of agogo_amd/csrc/replay.hpp (no HIP): the replay window's draw and ring arithmetic, on the code k_replay_sample
// compiles.  Driven by tests/test_replay_cpu.py.
//   out(0, 0) is the known first output of SplitMix64 seeded with 0; out(seed, i) is the i-th output of the sequential generator
//   (restated below as common.hpp has it); a run of draws consumes that stream two outputs per row, row after row, step after step;
//   symmetric off: every k is 0 and the js are unchanged; appends one row at a time keep the ring's logical order.
// Then it prints `draw <seed> <step> <rows> <n> <symmetric> <r> <j> <k>` and `slot <cap> <total> <j> <slot> <head>` lines, which the Python
// test recomputes with Python integers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../agogo_amd/csrc/replay.hpp"

using namespace agz;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the build's sequential SplitMix64 (agogo_amd/csrc/common.hpp), restated
struct SplitMix64 {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

int main() {
  CHECK(replay::out(0, 0) == 0xE220A8397B1DCDAFull, "out(0, 0) = %016llx", (unsigned long long)replay::out(0, 0));
  CHECK(replay::OUT_0_0 == 0xE220A8397B1DCDAFull, "OUT_0_0");
  const uint64_t seeds[] = {1, 7, 2024}, steps[] = {0, 1, 1ull << 33}, ns[] = {1, 5, 7, (1ull << 31) + 3};
  const int rowss[] = {1, 3, 64};
  for (uint64_t seed : seeds) {
    SplitMix64 g{seed};
    for (uint64_t i = 0; i < 1000; i++) {
      const uint64_t z = g.next();
      CHECK(replay::out(seed, i) == z, "out(%llu, %llu) is not the sequential generator's output", (unsigned long long)seed, (unsigned long long)i);
    }
    // a run: 3 steps of 5 rows consume outputs 0..29 in order
    SplitMix64 h{seed};
    for (uint64_t step = 0; step < 3; step++)
      for (int r = 0; r < 5; r++) {
        const uint64_t z0 = h.next(), z1 = h.next();
        const replay::Draw d = replay::draw(seed, step, 5, r, 7, true);
        CHECK(d.j == (uint64_t)(((unsigned __int128)z0 * 7) >> 64) && d.k == (int)(z1 >> 61), "seed %llu step %llu row %d leaves the stream",
              (unsigned long long)seed, (unsigned long long)step, r);
      }
    for (uint64_t step : steps)
      for (int rows : rowss)
        for (uint64_t n : ns)
          for (int symmetric = 0; symmetric < 2; symmetric++)
            for (int r = 0; r < rows; r++) {
              const replay::Draw d = replay::draw(seed, step, rows, r, n, symmetric != 0);
              CHECK(d.j < n && d.k >= 0 && d.k < 8, "draw out of range");
              if (!symmetric) {
                CHECK(d.k == 0, "k %d with symmetric sampling off", d.k);
                CHECK(d.j == replay::draw(seed, step, rows, r, n, true).j, "the switch changed the row drawn");
              }
              printf("draw %llu %llu %d %llu %d %d %llu %d\n", (unsigned long long)seed, (unsigned long long)step, rows, (unsigned long long)n,
                     symmetric, r, (unsigned long long)d.j, d.k);
            }
  }
  // the ring: single-row appends of the values 0, 1, 2, ...; before, at and after the wrap the live rows are the last n, oldest first
  for (uint64_t cap : {1ull, 5ull, 7ull}) {
    std::vector<long long> ring(cap, -1);
    uint64_t total = 0;
    for (long long v = 0; v < (long long)(3 * cap + 2); v++) {
      const uint64_t hd = replay::head(total, cap);
      CHECK(hd < cap, "head out of range");
      ring[hd] = v;
      total++;
      const uint64_t n = replay::live(total, cap);
      CHECK(n == (total < cap ? total : cap), "live(%llu, %llu)", (unsigned long long)total, (unsigned long long)cap);
      for (uint64_t j = 0; j < n; j++) {
        const uint64_t s = replay::slot(total, cap, j);
        CHECK(s < cap && ring[s] == (long long)(total - n + j), "cap %llu total %llu: logical %llu is not row %llu", (unsigned long long)cap,
              (unsigned long long)total, (unsigned long long)j, (unsigned long long)(total - n + j));
        printf("slot %llu %llu %llu %llu %llu\n", (unsigned long long)cap, (unsigned long long)total, (unsigned long long)j, (unsigned long long)s,
               (unsigned long long)replay::head(total, cap));
      }
    }
  }
  // far past 2^32 appends
  for (uint64_t total : {(1ull << 40) + 3, ~0ull}) {
    const uint64_t cap = 7, n = replay::live(total, cap);
    for (uint64_t j = 0; j < n; j++)
      printf("slot %llu %llu %llu %llu %llu\n", (unsigned long long)cap, (unsigned long long)total, (unsigned long long)j,
             (unsigned long long)replay::slot(total, cap, j), (unsigned long long)replay::head(total, cap));
  }
  if (fails) { printf("REPLAY CHECK FAILED (%d)\n", fails); return 1; }
  printf("REPLAY OK\n");
  return 0;
}
