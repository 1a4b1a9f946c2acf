// The exchange hooks of a sharded trainer (agz_trainer_create_sharded): rank r of n trains rows [r * B, (r + 1) * B) of a global batch of
// n * B rows, and dual.Train at the global batch needs a few collectives inside its step — the BatchNorm statistics of every layer in the
// forward and the backward pass, the cost, the shared tensors' gradients.  train.hip does not talk to RCCL: it calls these hooks, which the
// communicator (comm.hip) installs.  Every hook that moves data runs on the trainer's ctx stream, so no two collectives of one
// communicator are ever in flight on different queues.
#pragma once
#include <cstddef>
#include <functional>
#include <utility>
#include <vector>

#include "agz.h"

struct agz_shard_hooks {
  // all-gather of `count` doubles from every rank into recv [n][count] (rank order).  site: the tower layer 0 .. L whose statistics these
  // are, L + 1 for the heads (failure injection: agz_comm_debug_fail_layer)
  std::function<int(int site, const double* send, double* recv, size_t count)> gather;
  // one collective training step: runs body (the forward / backward pass, which calls gather), then — whatever body returned — enters the
  // gathers body did not reach, sums the shared tensors' gradients over the ranks and exchanges the one-word status.  Returns body's error
  // on the rank that failed and AGZ_E_PEER on the others.
  std::function<int(const std::function<int()>& body)> step;
  // one collective forward-only pass (agz_trainer_eval): body, then the one gather of the cost words if body did not reach it, then the
  // status word.  No gradient is summed.
  std::function<int(const std::function<int()>& body)> eval_step;
  // all-gather of `bytes` from every rank into recv [n][bytes] (synchronous; agz_trainer_save)
  std::function<int(const void* send, void* recv, size_t bytes)> allgather_bytes;
  // broadcast of `bytes` from rank 0 (synchronous; agz_trainer_export)
  std::function<int(void* buf, size_t bytes)> bcast0;
  // the status word of a collective call: rc on this rank if it failed, AGZ_E_PEER if another rank did, else AGZ_OK
  std::function<int(int rc)> agree;
};

// (train.hip) make a trainer built for B = BatchSize / n rows the rank-th shard of the global batch; allocates the gather buffer
int agz_trainer_bind_shard(agz_trainer* t, int rank, int n, agz_shard_hooks hooks);
bool agz_trainer_is_sharded(const agz_trainer* t);
// the element counts of the gathers one step issues, in issue order, and the buffer they land in ([n][largest count])
// (eval: the plan of agz_trainer_eval's pass, the one gather of the cost words)
void agz_trainer_exchange_plan(const agz_trainer* t, std::vector<size_t>& counts, bool eval = false);
double* agz_trainer_gather_buf(agz_trainer* t);
// (offset, count) of the shared tensors in the flat gradient buffer: every filter, the heads' 1x1 convolution, Wp, W1, W2
void agz_trainer_shared_ranges(const agz_trainer* t, std::vector<std::pair<size_t, size_t>>& out);
