// Dirichlet root noise (agz_arena_set_root_noise, DESIGN.md §2 root-noise).  ONE definition for host and device: k_root_noise
// (engine.hip), the host function agz_root_noise_of, and a plain g++ check (tests/cpp/noise_check.cpp).
//
// Everything below is IEEE double + - * / (each rounded once), integer and bit operations: no libm, no sqrt, no fma.  A device math
// function is not the host's to the last bit (sqrtf was found one ulp off on this toolchain), so ln and exp are two polynomials of our
// own, ln_b and exp_b — a few ulp from the true functions, the SAME few ulp everywhere, which is all a sampler needs.  Contraction is
// switched off per function (AGZ_NOISE_NOFMA / the attribute in AGZ_NOISE_HD), so the result does not depend on -ffp-contract either way.
//
//   RNG        SplitMix64: s += 0x9E3779B97F4A7C15; z = s; z = (z^(z>>30))*0xBF58476D1CE4E5B9; z = (z^(z>>27))*0x94D049BB133111EB; z ^= z>>31
//   u01(z)     ((double)(z >> 12) + 0.5) * 2^-52                     exact, strictly inside (0,1)
//   child i    of a draw with key `key`: the SplitMix64 stream from state key + (i+1)*0xD1B54A32D192ED03
//   gamma_i    ~ Gamma(alpha, 1), Ahrens-Dieter GS for 0 < alpha < 1, at most 64 rounds (then 0); alpha == 1: -ln_b(u1)
//   eta_i      (float)(gamma_i / S), S = gamma_0 + ... + gamma_{n-1} in index order in double; S == 0: (float)(1.0 / n)
//   mix        fadd(fmul(1.0f - eps, prior), fmul(eps, eta_i)) in float, one rounding per operation
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGZ_NOISE_HD __host__ __device__ __forceinline__
#elif defined(__GNUC__) && !defined(__clang__)
#define AGZ_NOISE_HD inline __attribute__((optimize("fp-contract=off")))
#else
#define AGZ_NOISE_HD inline
#endif
#if defined(__clang__)
#define AGZ_NOISE_NOFMA _Pragma("clang fp contract(off)")
#define AGZ_NOISE_ROLLED _Pragma("clang loop unroll(disable)")   // the two Horner loops stay loops: their constants would fill the scalar registers
#else
#define AGZ_NOISE_NOFMA
#define AGZ_NOISE_ROLLED
#endif

namespace agz {
namespace noise {

constexpr int MAX_ROUNDS = 64;        // Ahrens-Dieter rounds per child (rejection < 0.28 per round: unreachable, but the loop is bounded)
constexpr int MAX_N = 4096;           // agz_root_noise_of's largest n

AGZ_NOISE_HD uint64_t as_bits(double x) { union { double d; uint64_t u; } v; v.d = x; return v.u; }
AGZ_NOISE_HD double from_bits(uint64_t u) { union { double d; uint64_t u; } v; v.u = u; return v.d; }

// one SplitMix64 output; advances the state
AGZ_NOISE_HD uint64_t next(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
AGZ_NOISE_HD double u01(uint64_t z) {
  AGZ_NOISE_NOFMA
  return ((double)(z >> 12) + 0.5) * (1.0 / 4503599627370496.0);   // 2^-52
}
AGZ_NOISE_HD uint64_t child_state(uint64_t key, int i) { return key + (uint64_t)(i + 1) * 0xD1B54A32D192ED03ull; }

// natural logarithm of a positive normal double: x = m 2^e, m in (sqrt(1/2), sqrt 2]; ln m = 2 atanh(s), s = (m-1)/(m+1), 13 odd terms
AGZ_NOISE_HD double ln_b(double x) {
  AGZ_NOISE_NOFMA
  const uint64_t b = as_bits(x);
  int e = (int)((b >> 52) & 0x7FFull) - 1023;
  double m = from_bits((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
  if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
  const double s = (m - 1.0) / (m + 1.0);
  const double s2 = s * s;
  double acc = 0.0;
  AGZ_NOISE_ROLLED
  for (int k = 12; k >= 0; k--) acc = acc * s2 + 1.0 / (double)(2 * k + 1);
  return (double)e * 0.6931471805599453 + (2.0 * s) * acc;
}

// e^y for y <= 0: y = k ln 2 + r, |r| <= ln2 / 2 (+ the rounding of k ln 2), Taylor to degree 16 in Horner form, 2^k from the exponent bits
AGZ_NOISE_HD double exp_b(double y) {
  AGZ_NOISE_NOFMA
  if (y < -700.0) return 0.0;
  const double t = y * 1.4426950408889634 + 0.5;
  long long k = (long long)t;               // truncates towards zero ...
  if ((double)k > t) k -= 1;                // ... corrected to floor
  const double r = y - (double)k * 0.6931471805599453;
  double acc = 1.0;
  AGZ_NOISE_ROLLED
  for (int j = 16; j >= 1; j--) acc = 1.0 + (acc * r) / (double)j;
  return acc * from_bits((uint64_t)(k + 1023) << 52);   // y >= -700: k >= -1010, a normal power of two
}

// gamma_i of the draw `key`, 0 < alpha <= 1
AGZ_NOISE_HD double gamma_of(uint64_t key, int i, double alpha) {
  AGZ_NOISE_NOFMA
  uint64_t s = child_state(key, i);
  if (alpha == 1.0) return -ln_b(u01(next(s)));
  const double b = 1.0 + alpha / 2.718281828459045;
  for (int round = 0; round < MAX_ROUNDS; round++) {
    const double u1 = u01(next(s));
    const double u2 = u01(next(s));
    const double p = b * u1;
    if (p <= 1.0) {
      const double x = exp_b(ln_b(p) / alpha);
      if (u2 <= exp_b(-x)) return x;
    } else {
      const double x = -ln_b((b - p) / alpha);
      if (u2 <= exp_b((alpha - 1.0) * ln_b(x))) return x;
    }
  }
  return 0.0;
}

// eta_i from gamma_i and the sum S of all n (index order, double)
AGZ_NOISE_HD float eta_of(double gamma_i, double S, int n) {
  AGZ_NOISE_NOFMA
  return S == 0.0 ? (float)(1.0 / (double)n) : (float)(gamma_i / S);
}

AGZ_NOISE_HD float mix(float eps, float prior, float eta) {
  AGZ_NOISE_NOFMA
  const float c1 = 1.0f - eps;
  const float a = c1 * prior;
  const float b = eps * eta;
  return a + b;
}

// the whole draw on one thread (the host function; the kernel spreads gamma_of over a wavefront and sums in the same order).
// g: n doubles of scratch
AGZ_NOISE_HD void eta_all(uint64_t key, int n, double alpha, double* g, float* eta) {
  AGZ_NOISE_NOFMA
  double S = 0.0;
  for (int i = 0; i < n; i++) { g[i] = gamma_of(key, i, alpha); S = S + g[i]; }
  for (int i = 0; i < n; i++) eta[i] = eta_of(g[i], S, n);
}

}  // namespace noise
}  // namespace agz
