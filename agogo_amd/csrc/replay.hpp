// The replay window's draw and ring arithmetic (agz_replay, DESIGN.md §2 replay-window).  ONE definition for host and device:
// k_replay_sample (replay.hip), the host function agz_replay_draw, and a plain g++ check (tests/cpp/replay_check.cpp).
// Integer arithmetic only, and nothing of HIP is included.
//
//   out(seed, i)   the i-th output (from 0) of the build's SplitMix64 (common.hpp) seeded with `seed`: the finaliser of
//                  seed + (i + 1) * 0x9E3779B97F4A7C15 — counter based, so any output is reached without the ones before it
//   draw q         q = step * rows + r (uint64) is row r of minibatch `step`, every minibatch `rows` rows; z0 = out(seed, 2q),
//                  z1 = out(seed, 2q + 1): a whole run is ONE sequential SplitMix64 stream, two outputs per row, row after row, step
//                  after step, whatever the launch geometry
//   j              high 64 bits of z0 * n: uniform on [0, n), n = the live rows, 0 = the oldest; with replacement
//   k              z1 >> 61 under symmetric sampling, else 0; z1 is consumed either way, so the rows drawn do not depend on the switch
//   ring           cap slots, total = rows ever appended (uint64), n = min(total, cap); logical j lives in slot (total - n + j) mod cap;
//                  an append writes slot total mod cap, then total++
//   digest         of a window's LOGICAL content (DESIGN.md §2 replay-sharded): rowlen = F*H*W + PolicyLen + 1, bits(j, e) the 32-bit pattern
//                  of element e of logical row j (planes, then policy, then value; a packed window's decoded palette pattern),
//                  digest = live + sum over j < live, e < rowlen of mix64(mix64(j * rowlen + e) ^ bits(j, e)), uint64 and wrapping: an
//                  integer sum, the same in any order — k_replay_digest (replay.hip) and the host function agz_replay_digest_host
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGZ_REPLAY_HD __host__ __device__ inline __attribute__((always_inline))   // (no macro of hip_runtime.h: includable before it)
#else
#define AGZ_REPLAY_HD inline
#endif

namespace agz {
namespace replay {

constexpr uint64_t GAMMA = 0x9E3779B97F4A7C15ull;
constexpr uint64_t OUT_0_0 = 0xE220A8397B1DCDAFull;   // out(0, 0): the guard against a mistyped constant (tests/cpp/replay_check.cpp)

// the SplitMix64 finaliser
AGZ_REPLAY_HD uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

AGZ_REPLAY_HD uint64_t out(uint64_t seed, uint64_t i) { return mix64(seed + (i + 1) * GAMMA); }

// high 64 bits of a * b (device code includes hip_runtime.h before this header)
AGZ_REPLAY_HD uint64_t mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

AGZ_REPLAY_HD uint64_t draw_number(uint64_t step, int rows, int r) { return step * (uint64_t)rows + (uint64_t)r; }

struct Draw { uint64_t j; int k; };
// row r of minibatch `step`: logical index j in [0, n) and symmetry k
AGZ_REPLAY_HD Draw draw(uint64_t seed, uint64_t step, int rows, int r, uint64_t n, bool symmetric) {
  const uint64_t q = draw_number(step, rows, r);
  const uint64_t z0 = out(seed, 2 * q), z1 = out(seed, 2 * q + 1);
  Draw d;
  d.j = mulhi(z0, n);
  d.k = symmetric ? (int)(z1 >> 61) : 0;
  return d;
}

AGZ_REPLAY_HD uint64_t live(uint64_t total, uint64_t cap) { return total < cap ? total : cap; }
// physical slot of logical row j (0 = oldest live row), j < live(total, cap)
AGZ_REPLAY_HD uint64_t slot(uint64_t total, uint64_t cap, uint64_t j) { return (total - live(total, cap) + j) % cap; }
// the slot the next append writes
AGZ_REPLAY_HD uint64_t head(uint64_t total, uint64_t cap) { return total % cap; }

// one term of the digest: element e of logical row j, whose 32-bit pattern is `bits`
AGZ_REPLAY_HD uint64_t digest_term(uint64_t j, uint64_t rowlen, uint64_t e, uint32_t bits) { return mix64(mix64(j * rowlen + e) ^ (uint64_t)bits); }
// the digest of n rows held as three arrays of bit patterns in logical order (planes [n][xs], policy [n][A1], value [n])
inline uint64_t digest_rows(const uint32_t* planes, const uint32_t* policy, const uint32_t* value, uint64_t n, uint64_t xs, uint64_t A1) {
  const uint64_t rowlen = xs + A1 + 1;
  uint64_t d = n;
  for (uint64_t j = 0; j < n; j++) {
    for (uint64_t e = 0; e < xs; e++) d += digest_term(j, rowlen, e, planes[j * xs + e]);
    for (uint64_t e = 0; e < A1; e++) d += digest_term(j, rowlen, xs + e, policy[j * A1 + e]);
    d += digest_term(j, rowlen, xs + A1, value[j]);
  }
  return d;
}

}  // namespace replay
}  // namespace agz
