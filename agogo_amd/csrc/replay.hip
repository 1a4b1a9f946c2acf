// agz_replay: a sliding window over the most recent `capacity` examples, device resident, and its sampler (BUILD EXTENSION, DESIGN.md §2
// replay-window).  The standard AlphaZero arrangement around dual.Train: a ring of recent positions, minibatches drawn uniformly from it
// with replacement, each row under a random board symmetry applied AS IT IS DRAWN — no materialised copies (agz_examples_augment_dihedral
// holds eight), no index array and no host synchronisation per minibatch.  The draw and the ring arithmetic are replay.hpp's, the eight maps
// sym.hpp's.  Rows are agz_examples rows: planes [F*H*W], policy [PolicyLen], value, fp32.
#include <algorithm>
#include <vector>

#include "replay_win.hpp"   // (hip_runtime.h first: replay.hpp's device half uses __umul64hi)
#include "replay.hpp"
#include "sym.hpp"

namespace agz {

constexpr int REPLAY_THREADS = 256;
constexpr int REPLAY_SEG = REPLAY_THREADS * 8;   // elements of one output row that one workgroup moves
constexpr int REPLAY_TAB = 1024;                 // cells of the largest board sampled under a symmetry (32 x 32); 4 KB of LDS

// One minibatch: out row r = S_k(window row j), (j, k) = replay::draw(seed, step, rows, r, n, symmetric) — computed here, the same in every
// lane of the workgroup.  An output row is the concatenation [planes F*mm | policy A1 | value 1] cut into segments of REPLAY_SEG elements:
// grid = (segments, rows).  The mm source cells of S_k go to LDS once per workgroup; a plane element then costs one LDS read, one gathered
// global read (within a 4*mm-byte board: the same cache lines whatever k is) and one coalesced write.  k == 0 copies straight through.
// Pure data movement: algorithmic bytes = 2 x payload of `rows` rows.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_sample(const float* __restrict__ planes, const float* __restrict__ policy,
                                                                  const float* __restrict__ value, float* __restrict__ X,
                                                                  float* __restrict__ Pi, float* __restrict__ V, int F, int m, int mm,
                                                                  int A1, int rows, uint64_t seed, uint64_t step, int symmetric,
                                                                  uint64_t n, uint64_t total, uint64_t cap) {
  __shared__ int tab[REPLAY_TAB];
  const int xs = F * mm, row = xs + A1 + 1;
  const int e0 = (int)blockIdx.x * REPLAY_SEG;
  const int e1 = min(e0 + REPLAY_SEG, row);
  for (int r = (int)blockIdx.y; r < rows; r += (int)gridDim.y) {
    const replay::Draw d = replay::draw(seed, step, rows, r, n, symmetric != 0);
    const size_t s = (size_t)replay::slot(total, cap, d.j);
    const bool mapped = d.k != 0;     // (the host refuses symmetric sampling unless the board is square and mm <= REPLAY_TAB)
    if (mapped) {
      for (int c = (int)threadIdx.x; c < mm; c += REPLAY_THREADS) tab[c] = sym::src(m, d.k, c);
      __syncthreads();
    }
    const float* in_x = planes + s * (size_t)xs;
    const float* in_p = policy + s * (size_t)A1;
    float* out_x = X + (size_t)r * xs;
    float* out_p = Pi + (size_t)r * A1;
    for (int e = e0 + (int)threadIdx.x; e < e1; e += REPLAY_THREADS) {
      if (e < xs) {
        const int pl = e / mm, c = e - pl * mm;
        out_x[e] = in_x[pl * mm + (mapped ? tab[c] : c)];
      } else if (e < xs + A1) {
        const int c = e - xs;
        out_p[c] = in_p[(mapped && c < mm) ? tab[c] : c];
      } else {
        V[r] = value[s];
      }
    }
    if (mapped) __syncthreads();      // the table is rewritten for the next row of this workgroup
  }
}

}  // namespace agz

using namespace agz;

struct agz_replay {
  agz_ctx* ctx = nullptr;
  int F = 0, H = 0, W = 0, A1 = 0;
  size_t xs = 0;
  float *planes = nullptr, *policy = nullptr, *value = nullptr;   // [cap][xs], [cap][A1], [cap]
  uint64_t cap = 0, total = 0;

  uint64_t live() const { return replay::live(total, cap); }
  // c rows from (p, q, v) as c single-row appends in order: at most two contiguous row ranges per array; only the last cap rows of a
  // longer append survive
  int append(const float* p, const float* q, const float* v, uint64_t c, hipMemcpyKind kind) {
    const uint64_t skip = c > cap ? c - cap : 0, cnt = c - skip;
    const uint64_t s0 = replay::head(total + skip, cap);
    const uint64_t first = std::min<uint64_t>(cnt, cap - s0);
    hipStream_t s = ctx->stream;
    const uint64_t at[2] = {skip, skip + first}, to[2] = {s0, 0}, len[2] = {first, cnt - first};
    for (int i = 0; i < 2; i++) {
      if (!len[i]) continue;
      AGZ_HIP_TRY(hipMemcpyAsync(planes + to[i] * xs, p + at[i] * xs, len[i] * xs * 4, kind, s));
      AGZ_HIP_TRY(hipMemcpyAsync(policy + to[i] * A1, q + at[i] * A1, len[i] * (size_t)A1 * 4, kind, s));
      AGZ_HIP_TRY(hipMemcpyAsync(value + to[i], v + at[i], len[i] * 4, kind, s));
    }
    total += c;
    return AGZ_OK;
  }
};

ReplayInfo agz::replay_info(const agz_replay* rp) { return ReplayInfo{rp->ctx, rp->F, rp->H, rp->W, rp->A1, rp->total, rp->cap}; }

int agz::replay_check_symmetric(const agz_replay* rp, int symmetric, const char* who) {
  if (!symmetric) return AGZ_OK;
  AGZ_REQUIRE(rp->H == rp->W, AGZ_E_INVALID, "Cannot handle m %d, n %d. This function only takes square boards", rp->H, rp->W);
  AGZ_REQUIRE(rp->A1 >= rp->H * rp->W, AGZ_E_INVALID, "%s: policy shorter than the board", who);
  AGZ_REQUIRE(rp->H * rp->W <= REPLAY_TAB, AGZ_E_INVALID, "%s: symmetric sampling takes boards of at most %d cells", who, REPLAY_TAB);
  return AGZ_OK;
}

int agz::replay_sample_launch(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, uint64_t n, uint64_t total, float* X,
                              float* Pi, float* V) {
  const int mm = rp->H * rp->W;
  const int row = (int)rp->xs + rp->A1 + 1;
  const dim3 grid((unsigned)ceil_div(row, REPLAY_SEG), (unsigned)std::min(rows, 65535));
  hipLaunchKernelGGL(k_replay_sample, grid, dim3(REPLAY_THREADS), 0, rp->ctx->stream, rp->planes, rp->policy, rp->value, X, Pi, V, rp->F,
                     rp->H, mm, rp->A1, rows, seed, step, symmetric, n, total, rp->cap);
  AGZ_HIP_TRY(hipGetLastError());
  return AGZ_OK;
}

extern "C" {

int agz_replay_create(agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, int64_t capacity, agz_replay** out) {
  AGZ_REQUIRE(ctx && out, AGZ_E_INVALID, "agz_replay_create: NULL argument");
  AGZ_REQUIRE(Features >= 1 && Height >= 1 && Width >= 1 && PolicyLen >= 1, AGZ_E_INVALID, "agz_replay_create: bad shape");
  AGZ_REQUIRE(capacity >= 1, AGZ_E_INVALID, "agz_replay_create: capacity %lld (at least 1 row)", (long long)capacity);
  const size_t xs = (size_t)Features * Height * Width;
  AGZ_REQUIRE(xs + (size_t)PolicyLen + 1 <= (size_t)1 << 30, AGZ_E_INVALID, "agz_replay_create: a row of %zu floats is too long", xs + PolicyLen + 1);
  AGZ_HIP_TRY(hipSetDevice(ctx->device));
  const size_t cap = (size_t)capacity;
  float *p = nullptr, *q = nullptr, *v = nullptr;
  if (hipMalloc(&p, cap * xs * 4) != hipSuccess || hipMalloc(&q, cap * PolicyLen * 4) != hipSuccess || hipMalloc(&v, cap * 4) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(p); hipFree(q); hipFree(v);
    agz::set_error("agz_replay_create: out of device memory for a window of %zu rows (%zu bytes)", cap, cap * (xs + PolicyLen + 1) * 4);
    return AGZ_E_NOMEM;
  }
  agz_replay* rp = new agz_replay();
  rp->ctx = ctx; rp->F = Features; rp->H = Height; rp->W = Width; rp->A1 = PolicyLen; rp->xs = xs;
  rp->planes = p; rp->policy = q; rp->value = v; rp->cap = (uint64_t)cap;
  *out = rp;
  return AGZ_OK;
}

void agz_replay_destroy(agz_replay* rp) {
  if (!rp) return;
  hipSetDevice(rp->ctx->device);
  hipStreamSynchronize(rp->ctx->stream);
  hipFree(rp->planes); hipFree(rp->policy); hipFree(rp->value);
  delete rp;
}

int agz_replay_count(const agz_replay* rp, int64_t* live, uint64_t* total, int64_t* capacity) {
  AGZ_REQUIRE(rp, AGZ_E_INVALID, "agz_replay_count: NULL window");
  if (live) *live = (int64_t)rp->live();
  if (total) *total = rp->total;
  if (capacity) *capacity = (int64_t)rp->cap;
  return AGZ_OK;
}

int agz_replay_clear(agz_replay* rp) {
  AGZ_REQUIRE(rp, AGZ_E_INVALID, "agz_replay_clear: NULL window");
  rp->total = 0;
  return AGZ_OK;
}

int agz_replay_append_examples(agz_replay* rp, agz_examples* ex) {
  AGZ_REQUIRE(rp && ex, AGZ_E_INVALID, "agz_replay_append_examples: NULL argument");
  const ExamplesInfo e = examples_info(ex);
  AGZ_REQUIRE(e.ctx == rp->ctx, AGZ_E_INVALID, "agz_replay_append_examples: the window and the example set belong to different contexts");
  AGZ_REQUIRE(e.F == rp->F && e.H == rp->H && e.W == rp->W && e.A1 == rp->A1, AGZ_E_INVALID,
              "agz_replay_append_examples: the example set's rows are [%d, %d, %d] + %d, the window's [%d, %d, %d] + %d", e.F, e.H, e.W, e.A1,
              rp->F, rp->H, rp->W, rp->A1);
  if (e.n == 0) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  return rp->append(e.planes, e.policy, e.value, e.n, hipMemcpyDeviceToDevice);   // (same queue as the set's own appends: ordered after them)
}

int agz_replay_append_dev(agz_replay* rp, const float* planes_dev, const float* policy_dev, const float* value_dev, int64_t n) {
  AGZ_REQUIRE(rp && n >= 0 && (n == 0 || (planes_dev && policy_dev && value_dev)), AGZ_E_INVALID, "agz_replay_append_dev: bad argument");
  if (n == 0) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  return rp->append(planes_dev, policy_dev, value_dev, (uint64_t)n, hipMemcpyDeviceToDevice);
}

int agz_replay_append_host(agz_replay* rp, const float* planes, const float* policy, const float* value, int64_t n) {
  AGZ_REQUIRE(rp && n >= 0 && (n == 0 || (planes && policy && value)), AGZ_E_INVALID, "agz_replay_append_host: bad argument");
  if (n == 0) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  int r = rp->append(planes, policy, value, (uint64_t)n, hipMemcpyHostToDevice);
  AGZ_HIP_TRY(hipStreamSynchronize(rp->ctx->stream));   // the buffers are the caller's
  return r;
}

int agz_replay_get(agz_replay* rp, int64_t j0, int64_t cnt, float* planes, float* policy, float* value) {
  AGZ_REQUIRE(rp, AGZ_E_INVALID, "agz_replay_get: NULL window");
  AGZ_REQUIRE(j0 >= 0 && cnt >= 0 && (uint64_t)j0 + (uint64_t)cnt <= rp->live(), AGZ_E_INVALID,
              "agz_replay_get: rows [%lld, %lld) of %llu live", (long long)j0, (long long)(j0 + cnt), (unsigned long long)rp->live());
  if (cnt == 0) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(rp->ctx->stream));
  const uint64_t s0 = replay::slot(rp->total, rp->cap, (uint64_t)j0);
  const uint64_t first = std::min<uint64_t>((uint64_t)cnt, rp->cap - s0);
  const uint64_t at[2] = {0, first}, from[2] = {s0, 0}, len[2] = {first, (uint64_t)cnt - first};
  for (int i = 0; i < 2; i++) {
    if (!len[i]) continue;
    if (planes) AGZ_HIP_TRY(hipMemcpy(planes + at[i] * rp->xs, rp->planes + from[i] * rp->xs, len[i] * rp->xs * 4, hipMemcpyDeviceToHost));
    if (policy) AGZ_HIP_TRY(hipMemcpy(policy + at[i] * rp->A1, rp->policy + from[i] * rp->A1, len[i] * (size_t)rp->A1 * 4, hipMemcpyDeviceToHost));
    if (value) AGZ_HIP_TRY(hipMemcpy(value + at[i], rp->value + from[i], len[i] * 4, hipMemcpyDeviceToHost));
  }
  return AGZ_OK;
}

int agz_replay_sample_dev(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, float* X_dev, float* Pi_dev, float* V_dev) {
  AGZ_REQUIRE(rp && X_dev && Pi_dev && V_dev, AGZ_E_INVALID, "agz_replay_sample_dev: NULL argument");
  AGZ_REQUIRE(rows >= 1, AGZ_E_INVALID, "agz_replay_sample_dev: rows %d (at least 1)", rows);
  int r = replay_check_symmetric(rp, symmetric, "agz_replay_sample_dev");
  if (r != AGZ_OK) return r;
  AGZ_REQUIRE(rp->total > 0, AGZ_E_STATE, "agz_replay_sample_dev: the window is empty");
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  return replay_sample_launch(rp, rows, seed, step, symmetric, rp->live(), rp->total, X_dev, Pi_dev, V_dev);
}

int agz_replay_sample(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, float* X, float* Pi, float* V) {
  AGZ_REQUIRE(rp && X && Pi && V, AGZ_E_INVALID, "agz_replay_sample: NULL argument");
  AGZ_REQUIRE(rows >= 1, AGZ_E_INVALID, "agz_replay_sample: rows %d (at least 1)", rows);
  int r = replay_check_symmetric(rp, symmetric, "agz_replay_sample");
  if (r != AGZ_OK) return r;
  AGZ_REQUIRE(rp->total > 0, AGZ_E_STATE, "agz_replay_sample: the window is empty");
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  const size_t nx = (size_t)rows * rp->xs, np = (size_t)rows * rp->A1, nv = (size_t)rows;
  float* d = nullptr;
  if (hipMalloc(&d, (nx + np + nv) * 4) != hipSuccess) {
    (void)hipGetLastError();
    agz::set_error("agz_replay_sample: out of device memory for %d rows", rows);
    return AGZ_E_NOMEM;
  }
  hipStream_t s = rp->ctx->stream;
  r = replay_sample_launch(rp, rows, seed, step, symmetric, rp->live(), rp->total, d, d + nx, d + nx + np);
  hipError_t e = hipSuccess;
  if (r == AGZ_OK) e = hipMemcpyAsync(X, d, nx * 4, hipMemcpyDeviceToHost, s);
  if (r == AGZ_OK && e == hipSuccess) e = hipMemcpyAsync(Pi, d + nx, np * 4, hipMemcpyDeviceToHost, s);
  if (r == AGZ_OK && e == hipSuccess) e = hipMemcpyAsync(V, d + nx + np, nv * 4, hipMemcpyDeviceToHost, s);
  const hipError_t se = hipStreamSynchronize(s);
  hipFree(d);
  if (r != AGZ_OK) return r;
  AGZ_HIP_TRY(e);
  AGZ_HIP_TRY(se);
  return AGZ_OK;
}

int agz_replay_draw(uint64_t seed, uint64_t step, int rows, int64_t n, int symmetric, int64_t* j, int32_t* k) {
  AGZ_REQUIRE(rows >= 1 && n >= 1, AGZ_E_INVALID, "agz_replay_draw: rows %d, n %lld (at least 1 each)", rows, (long long)n);
  AGZ_REQUIRE(j || k, AGZ_E_INVALID, "agz_replay_draw: NULL argument");
  for (int r = 0; r < rows; r++) {
    const replay::Draw d = replay::draw(seed, step, rows, r, (uint64_t)n, symmetric != 0);
    if (j) j[r] = (int64_t)d.j;
    if (k) k[r] = d.k;
  }
  return AGZ_OK;
}

}  // extern "C"
