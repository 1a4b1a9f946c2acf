// Playout cap randomization (agz_arena_set_playout_cap, DESIGN.md §2 playout-cap).  ONE definition for host and device: k_cap_decide
// (engine.hip) and the host function agz_playout_cap_of.
//
// Every ply of every game is a FULL search (mcts.Budget simulations, root noise, a recorded row) with probability p_full, else a FAST
// one (fast_budget simulations, no noise, no row).  Integer and bit operations only, as noise.hpp, target.hpp and replay.hpp: the one
// float product below is exact (a power of two), so host, device and a restatement in any language agree bit for bit.
//
//   mix64     the SplitMix64 finaliser: z = (z^(z>>30))*0xBF58476D1CE4E5B9; z = (z^(z>>27))*0x94D049BB133111EB; z ^= z>>31
//   z         mix64(seed ^ mix64(key + 0x9E3779B97F4A7C15 * (uint64)(ply + 1)))
//   thr       (uint32)(p_full * 16777216.0f)          p_full = 1 gives 2^24, p_full = 0 gives 0
//   kind      FULL if (uint32)(z >> 40) < thr, else FAST
//
// key = the game slot's own key d.rng_game[g] (seeded by k_reset, advanced when the slot restarts, stored in arena checkpoints), ply =
// d.ply[g], both as they stand at agz_arena_begin_move.  The decision draws from no RNG stream: it is a pure function of checkpointed
// state and the setting.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGZ_CAP_HD __host__ __device__ __forceinline__
#else
#define AGZ_CAP_HD inline
#endif

namespace agz {
namespace cap {

constexpr int FULL = 0;   // AGZ_CAP_FULL
constexpr int FAST = 1;   // AGZ_CAP_FAST

AGZ_CAP_HD uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 0 <= p_full <= 1: the product is exact and at most 2^24
AGZ_CAP_HD uint32_t threshold(float p_full) { return (uint32_t)(p_full * 16777216.0f); }

AGZ_CAP_HD int kind_of(uint64_t seed, uint64_t key, int32_t ply, uint32_t thr) {
  const uint64_t z = mix64(seed ^ mix64(key + 0x9E3779B97F4A7C15ull * (uint64_t)(ply + 1)));
  return (uint32_t)(z >> 40) < thr ? FULL : FAST;
}

}  // namespace cap
}  // namespace agz
