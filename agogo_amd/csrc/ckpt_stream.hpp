// The device side of a checkpoint stream, shared by the arena's (engine.hip) and the replay window's (replay.hip) save and load.  HIP host
// code, no kernels.  A large section moves between the device and its codec (arena_ckpt.hpp, replay_ckpt.hpp) in chunks through TWO
// page-locked host buffers and, where a kernel gathers or scatters the chunk, ONE device buffer, all on one queue: the copy of chunk i + 1
// runs while the file system has chunk i.  The callers say what a chunk is (the planners of the two codecs) and what moves it; the order
// of the copies, the events and the waits — what keeps a host buffer from being reused while it is still in flight — is here, once.
// Every callback returns the library's status; the first failure ends the stream and is returned unchanged.
#pragma once
#include "common.hpp"

namespace agz {

// the staging of one save or load; released (after the queue has drained) when the call returns, whatever happened
struct CkptStaging {
  hipStream_t s = nullptr;
  void* dev = nullptr;
  void* host[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  int init(hipStream_t stream, size_t bytes, bool device) {   // device: with the device buffer
    s = stream;
    for (int i = 0; i < 2; i++) { AGZ_HIP_TRY(hipHostMalloc(&host[i], bytes, hipHostMallocDefault)); AGZ_HIP_TRY(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)); }
    if (device) AGZ_HIP_TRY(hipMalloc(&dev, bytes));
    return AGZ_OK;
  }
  ~CkptStaging() {
    if (s) hipStreamSynchronize(s);
    if (dev) hipFree(dev);
    for (int i = 0; i < 2; i++) { if (host[i]) hipHostFree(host[i]); if (ev[i]) hipEventDestroy(ev[i]); }
  }
};

// a device allocation of the caller's that the stream's kernels read or write, released as the staging is.  A local declared AFTER the
// CkptStaging it goes with (so it goes first).  from: `bytes` of the host's to start with.
struct CkptScratch {
  hipStream_t s = nullptr;
  void* p = nullptr;
  int init(hipStream_t stream, size_t bytes, const void* from = nullptr) {
    s = stream;
    AGZ_HIP_TRY(hipMalloc(&p, bytes));
    if (from) { AGZ_HIP_TRY(hipMemcpyAsync(p, from, bytes, hipMemcpyHostToDevice, s)); AGZ_HIP_TRY(hipStreamSynchronize(s)); }
    return AGZ_OK;
  }
  ~CkptScratch() { if (s) hipStreamSynchronize(s); if (p) hipFree(p); }
};

// device -> file.  issue(i, host) enqueues the copies of chunk i into `host`; sink(i, host) hands the arrived chunk to the codec.  Chunk
// i + 1 is issued before chunk i is waited for: its copy runs under chunk i's write.
template <class Issue, class Sink>
int stream_out(CkptStaging& st, size_t n_chunks, Issue issue, Sink sink) {
  int r;
  auto go = [&](size_t i) -> int {
    if ((r = issue(i, st.host[i & 1])) != AGZ_OK) return r;
    AGZ_HIP_TRY(hipEventRecord(st.ev[i & 1], st.s));
    return AGZ_OK;
  };
  if (n_chunks && (r = go(0)) != AGZ_OK) return r;
  for (size_t i = 0; i < n_chunks; i++) {
    if (i + 1 < n_chunks && (r = go(i + 1)) != AGZ_OK) return r;
    AGZ_HIP_TRY(hipEventSynchronize(st.ev[i & 1]));
    if ((r = sink(i, st.host[i & 1])) != AGZ_OK) return r;
  }
  return AGZ_OK;
}

// file -> device.  fill(i, host) reads chunk i from the file into `host`; copy(i, host) enqueues its copies to the device, behind which
// the buffer's event is recorded; after(i) launches what consumes the device buffer, if anything does.  The file read of chunk i runs
// under the copy and the kernel of chunk i - 1; the one queue orders the device buffer's reuse.
template <class Fill, class Copy, class After>
int stream_in(CkptStaging& st, size_t n_chunks, Fill fill, Copy copy, After after) {
  int r;
  for (size_t i = 0; i < n_chunks; i++) {
    if (i >= 2) AGZ_HIP_TRY(hipEventSynchronize(st.ev[i & 1]));   // host[i & 1] has left for the device
    if ((r = fill(i, st.host[i & 1])) != AGZ_OK || (r = copy(i, st.host[i & 1])) != AGZ_OK) return r;
    AGZ_HIP_TRY(hipEventRecord(st.ev[i & 1], st.s));
    if ((r = after(i)) != AGZ_OK) return r;
  }
  return AGZ_OK;
}

}  // namespace agz
