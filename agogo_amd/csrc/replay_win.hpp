// What train.hip needs of a replay window (replay.hip): its context, row shape and ring counters, and one sampler launch.
#pragma once
#include "common.hpp"

struct agz_replay;
struct agz_examples;

namespace agz {
struct ReplayInfo {
  agz_ctx* ctx;
  int F, H, W, A1;
  uint64_t ring_total, cap;   // ring_total: the rows the ring has taken, what replay.hpp's arithmetic calls `total` (agz_replay_count's
                              // total, less the rows a loaded checkpoint did not hold: agz_replay_load into a larger window)
  bool packed;
};
ReplayInfo replay_info(const agz_replay* rp);
// enqueue ONE k_replay_sample (k_replay_sample_packed for a packed window) on the window's context stream: rows [row0, row0 + cnt) of
// minibatch `step` of `rows` rows drawn from the n live rows of the ring state (total, cap), written to rows [0, cnt) of the device buffers
// X [cnt, F*H*W], Pi [cnt, A1], V [cnt].  The whole minibatch: row0 = 0, cnt = rows.  No synchronisation, nothing uploaded.
int replay_sample_launch(agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric, uint64_t n,
                         uint64_t total, float* X, float* Pi, float* V);

// symmetric sampling needs a square board whose policy row holds every cell (the augmenter's preconditions and wording)
int replay_check_symmetric(const agz_replay* rp, int symmetric, const char* who);
// (examples.hip) the raw store of an example set as the window's agz_replay_append_examples reads it: rows in append order
struct ExamplesInfo {
  agz_ctx* ctx;
  int F, H, W, A1;
  const float *planes, *policy, *value;
  uint64_t n;
};
ExamplesInfo examples_info(const agz_examples* ex);
}  // namespace agz
