// Plain g++ check of agogo_amd/csrc/noise.hpp (no HIP): the Dirichlet root noise on the code the kernel compiles.  Driven by
// tests/test_root_noise_cpu.py, which builds this file at -O0 and at -O2 and requires the same output from both, then recomputes every
// line with its pure-Python restatement.  Output, all floating-point values as hexadecimal bit patterns:
//   ln <x bits> <ln_b(x) bits>          exp <y bits> <exp_b(y) bits>
//   eta <key> <n> <alpha float bits> <eta_0 bits> ... <eta_{n-1} bits>
//   mix <eps bits> <prior bits> <eta bits> <result bits>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../agogo_amd/csrc/noise.hpp"

using namespace agz;

static uint32_t fbits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float ffrom(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

int main() {
  uint64_t s = 20261020;
  // ln_b over many binades and around 1 and sqrt 2; exp_b over [-700, 0]
  for (int i = 0; i < 200; i++) {
    const double u = noise::u01(noise::next(s));
    double x = i < 60 ? 0.5 + 1.5 * u : (i < 120 ? u * 1e-3 : (i < 160 ? u : 1.0 + 40.0 * u));
    if (i == 0) x = 1.0;
    if (i == 1) x = 1.4142135623730951;
    if (i == 2) x = 2.2250738585072014e-308;
    printf("ln %016" PRIx64 " %016" PRIx64 "\n", noise::as_bits(x), noise::as_bits(noise::ln_b(x)));
  }
  for (int i = 0; i < 200; i++) {
    const double u = noise::u01(noise::next(s));
    double y = i < 100 ? -700.0 * u : (i < 180 ? -5.0 * u : -1e-6 * u);
    if (i == 0) y = -0.0;
    if (i == 1) y = -700.0;
    if (i == 2) y = -700.5;
    printf("exp %016" PRIx64 " %016" PRIx64 "\n", noise::as_bits(y), noise::as_bits(noise::exp_b(y)));
  }
  const struct { int n; float alpha; } cases[] = {{1, 0.3f}, {2, 0.9f}, {10, 0.3f}, {26, 0.3f}, {82, 0.15f}, {362, 0.03f}, {5, 1.0f}, {7, 0.5f}};
  for (const auto& c : cases) {
    for (int rep = 0; rep < 6; rep++) {
      const uint64_t key = rep == 0 ? 0ull : (rep == 1 ? ~0ull : noise::next(s));
      std::vector<double> g(c.n);
      std::vector<float> eta(c.n);
      noise::eta_all(key, c.n, (double)c.alpha, g.data(), eta.data());
      printf("eta %" PRIu64 " %d %08x", key, c.n, fbits(c.alpha));
      for (int i = 0; i < c.n; i++) printf(" %08x", fbits(eta[i]));
      printf("\n");
    }
  }
  for (int i = 0; i < 64; i++) {
    const float eps = i % 4 == 0 ? 0.25f : (i % 4 == 1 ? 1.0f : (i % 4 == 2 ? 0.0f : (float)noise::u01(noise::next(s))));
    const float prior = (float)noise::u01(noise::next(s));
    const float eta = (float)(noise::u01(noise::next(s)) * noise::u01(noise::next(s)));
    printf("mix %08x %08x %08x %08x\n", fbits(eps), fbits(prior), fbits(eta), fbits(noise::mix(eps, ffrom(fbits(prior)), eta)));
  }
  printf("NOISE OK\n");
  return 0;
}
