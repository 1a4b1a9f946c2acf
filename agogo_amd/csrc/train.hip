// dual.Train on device: training-mode forward, backward, vanilla SGD.
//
// Reference: dualnet/meta.go:16-54 (Train), dualnet/dual.go:50-132 (fwd + bwd graph),
// dualnet/ermahagerdmonards.go:106-147 (the "xent" on logits), G.NewVanillaSolver(lr 0.1) meta.go:17-20.
// Learnables keep the reference's FULL shapes: BN gamma/beta [B,C,H,W] and FC biases [B,units] are batch-shaped
// (SURVEY App. B b3/b5); inference uses row 0 (agz_trainer_export == the copy loop of dual.Infer, meta.go:141-146).
//
// Device layout: activations / conv outputs padded NHWC (zero halo) like the inference tower; the two convs of a
// block run as ONE GEMM with 2K output channels [a | b]; gamma/beta stored [B][HW][C] so they line up with the
// GEMM rows.  All learnables live in one flat buffer P and all gradients in one flat buffer G (same offsets):
// the SGD step is a single axpy and a data-parallel run needs ONE all-reduce over G (agz_trainer_grads_dev).
//
// Kernels, per compute mode (agz_trainer_set_compute_mode; every mode inside the same gradient tolerance against oracle/train.hpp):
//   AGZ_COMPUTE_F32_MFMA  forward and data-gradient convolutions through conv3x3_mfma_kernel (raw epilogue; the data gradient is the
//                         same GEMM with tap-flipped, transposed weights), weight gradient k_wgrad (fp32 MFMA)            125 ms / G19 step
//   AGZ_COMPUTE_BF16X3    the three GEMMs on the bf16 pipe with exact three-way operand splits (conv3x3_x3 raw, k_wgrad_x3)    82 ms
//   AGZ_COMPUTE_WINO_H2   forward = the DIRECT fp16x2 convolution as a pure DMA GEMM (k_conv_h2dma below: fp16 hi / lo planes of the layer
//                         input — written by the BatchNorm pass that produces the tensor, shared with the weight gradient — and the
//                         fp16x2 weight image, both by LDS-DMA; 0.55-0.58 ms per layer), data gradient = the Winograd fp16x2 path
//                         (conv_wino_h2.hpp), weight gradient = k_wgrad_h2t3 (hi / lo fp16 planes of both operands, LDS-DMA, three taps
//                         per workgroup from one x image, ds_read_b64_tr_b16): 0.55 ms per layer alone, 0.48 of the fp16x2 MFMA roof;
//                         every layer's weight images are built at the start of the step on the side stream (prep_weights)  42.5-43.3 ms
// BatchNorm statistics / apply / backward are bandwidth-bound elementwise + reduction kernels at ~5 TB/s (43 % of a layer's time: the
// reference's batch-shaped gamma / beta fix their bytes); the heads run as wave-per-row reductions and LDS-tiled FC kernels (second form,
// 0.35 ms per step); the batch-shaped gamma / beta take their SGD step inside k_bn_bwd1 on single-process steps; the weight gradient
// runs on its own stream; a data-parallel step reduces every layer's slice of the flat gradient buffer under the backward pass
// (on_slice, comm.hip).  A sharded trainer (agz_trainer_create_sharded) holds its rank's rows of the global batch and
// exchanges the BatchNorm statistics' partial sums through the hooks of shard.hpp (comm.hip), summing them in rank order.
#include <cmath>
#include <cstring>
#include <thread>
#include <functional>
#include <vector>

#include "net.hpp"
#include "conv_maps.hpp"
#include "ckpt.hpp"
#include "replay_win.hpp"
#include "shard.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace agz {

struct TGeo { int B, H, W, HW, Hp, Wp, M; };  // M = B*HW rows

__host__ __device__ constexpr __forceinline__ size_t pix_off(const TGeo& g, int r) {  // padded pixel index of GEMM row r
  int b = r / g.HW, p = r - b * g.HW;
  int h = p / g.W, w = p - h * g.W;
  return ((size_t)b * g.Hp + h + 1) * g.Wp + w + 1;
}
// (the same function as conv_maps.hpp's pix, which the CPU check of k_conv_h2dma3's image geometry uses: compared at compile time)
constexpr bool pix_off_is_cmaps_pix(int B, int H, int W) {
  const TGeo g{B, H, W, H * W, H + 2, W + 2, B * H * W};
  for (int m = 0; m < g.M; m++)
    if (pix_off(g, m) != cmaps::pix(m, g.HW, g.W, g.Hp, g.Wp)) return false;
  return true;
}
static_assert(pix_off_is_cmaps_pix(3, 19, 19) && pix_off_is_cmaps_pix(2, 16, 17) && pix_off_is_cmaps_pix(5, 3, 4), "pix_off != cmaps::pix");

// ---- BatchNorm statistics: per-channel sums over the M interior rows of z [pix][C] -----------------------------
// pass 0: sum(z)                    -> acc[c]
// pass 1: sum((z - mean)^2)         -> acc[c]      (two-pass variance like the oracle)
__global__ void k_bn_sum(TGeo g, const float* __restrict__ z, int C, const float* __restrict__ mean, double* __restrict__ acc,
                         int rows_per_block) {
  int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float mu = mean ? mean[c] : 0.f;
    double s = 0;
    for (int r = r0; r < r1; r++) {
      float v = z[pix_off(g, r) * C + c];
      if (mean) { float d = v - mu; s += (double)d * d; } else s += v;
    }
    atomicAdd(&acc[c], s);
  }
}
// ---- running statistics (agz_trainer_set_bn_tracking; the `bn-running` row of DESIGN §2) -------------------------------------------------
// The state of one finalize launch (a tower layer = one or two BatchNorm ops side by side, or the heads' 2 + 1 channels), all double:
// st = S_mean[C] | S_var[C] | N[C / Kop], Kop = channels per op (channel c belongs to op c / Kop).  Every training forward adds the mean and
// the biased variance it normalises with — the doubles the finalize kernels hold anyway — to accumulators that decay by lam, and N takes the
// same recurrence with 1: S / N is then a weighted mean of the batches' statistics, exact from the first step (N = 1: the very values of
// that forward).  TRACK is a template parameter of the finalize kernels: the <false> instantiation is the code that ran before the state
// existed (BnTrack is then an unused kernel argument, as SolverDev is for k_bn_bwd1<false, false>).
struct BnTrack { double* st; int C; int Kop; double lam; };
__device__ __forceinline__ void bn_track_mean(const BnTrack& tr, int c, double mu) { tr.st[c] = tr.lam * tr.st[c] + mu; }
__device__ __forceinline__ void bn_track_var(const BnTrack& tr, int c, double var) {   // (the last statistic of a forward: N steps with it)
  tr.st[tr.C + c] = tr.lam * tr.st[tr.C + c] + var;
  if (c % tr.Kop == 0) { double* n = tr.st + 2 * tr.C + c / tr.Kop; *n = tr.lam * *n + 1.0; }
}
// the estimates as a layer's mean / inv (agz_trainer_eval in place of the statistics kernels): inv is the finalize kernels' float expression
__global__ void k_bn_from_running(BnTrack tr, float eps, float* __restrict__ mean, float* __restrict__ inv) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= tr.C) return;
  const double n = tr.st[2 * tr.C + c / tr.Kop];
  mean[c] = (float)(tr.st[c] / n);
  inv[c] = 1.0f / sqrtf((float)(tr.st[tr.C + c] / n) + eps);
}
// finalize: pass 0 -> mean = acc/m ; pass 1 -> inv = 1/sqrt(acc/m + eps).  Clears acc.
template <bool TRACK>
__global__ void k_bn_fin(double* acc, int C, double m, float eps, float* mean, float* inv, int pass, BnTrack tr) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  if (pass == 0) mean[c] = (float)(acc[c] / m); else inv[c] = 1.0f / sqrtf((float)(acc[c] / m) + eps);
  if (TRACK) { if (pass == 0) bn_track_mean(tr, c, acc[c] / m); else bn_track_var(tr, c, acc[c] / m); }
  acc[c] = 0;
}

// One pass for both statistics (C % 4 == 0, C <= 1024): sum(z) -> acc[c], sum(z^2) -> acc[1024 + c], both in double (a product of
// two fp32 values is exact in double, so E[z^2] - mean^2 loses nothing against the two-pass form above at these row counts); float4
// loads, 256 / (C/4) row slices per workgroup reduced through LDS, one double atomic per channel and workgroup.
__global__ __launch_bounds__(256) void k_bn_stats(TGeo g, const float* __restrict__ z, int C, double* __restrict__ acc, int rows_per_block) {
  __shared__ double red[2][1024];
  const int c4n = C >> 2, slices = 256 / c4n;
  const int tid = threadIdx.x, cg = tid % c4n, rs = tid / c4n;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  if (rs < slices) {
    int r = r0 + rs;
    for (; r + 3 * slices < r1; r += 4 * slices) {   // four rows in flight (one load per iteration left the kernel at 2.4 TB/s)
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const float4*>(z + pix_off(g, r + u * slices) * C + 4 * cg);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        s[0] += v[u].x; s[1] += v[u].y; s[2] += v[u].z; s[3] += v[u].w;
        q[0] += (double)v[u].x * v[u].x; q[1] += (double)v[u].y * v[u].y; q[2] += (double)v[u].z * v[u].z; q[3] += (double)v[u].w * v[u].w;
      }
    }
    for (; r < r1; r += slices) {
      const float4 v = *reinterpret_cast<const float4*>(z + pix_off(g, r) * C + 4 * cg);
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
      q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
    }
  }
  for (int c = tid; c < C; c += 256) { red[0][c] = 0; red[1][c] = 0; }
  __syncthreads();
  for (int k = 0; k < slices; k++) {          // slice after slice: a fixed summation order inside the workgroup
    if (rs == k) {
#pragma unroll
      for (int e = 0; e < 4; e++) { red[0][4 * cg + e] += s[e]; red[1][4 * cg + e] += q[e]; }
    }
    __syncthreads();
  }
  for (int c = tid; c < C; c += 256) { atomicAdd(&acc[c], red[0][c]); atomicAdd(&acc[1024 + c], red[1][c]); }
}
template <bool TRACK>
__global__ void k_bn_fin2(double* acc, int C, double m, float eps, float* mean, float* inv, BnTrack tr) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mu = acc[c] / m;
  double var = acc[1024 + c] / m - mu * mu;
  var = var > 0 ? var : 0;
  mean[c] = (float)mu;
  inv[c] = 1.0f / sqrtf((float)var + eps);
  if (TRACK) { bn_track_mean(tr, c, mu); bn_track_var(tr, c, var); }
  acc[c] = 0; acc[1024 + c] = 0;
}

// ---- sharded trainer (agz_trainer_create_sharded): the per-channel sums of the n ranks, gathered as n partial vectors --------------
// xg [n][stride] holds every rank's partial sums (an all-gather of each rank's acc), summed here in RANK order: every rank computes the
// same bits, run after run, whatever the collective's own reduction algorithm.  mode 2: the single-pass statistics (sums at [0, C), sums
// of squares at [1024, 1024 + C)) -> mean, inv as k_bn_fin2; mode 0 / 1: the two passes of k_bn_fin.  m = rows of the GLOBAL batch.
// With n = 1 the expressions are those of k_bn_fin2 / k_bn_fin on the same values.  Clears this rank's acc.
template <bool TRACK>
__global__ void k_bn_fin_ranks(const double* __restrict__ xg, int n, int stride, double* __restrict__ acc, int C, double m, float eps,
                               float* __restrict__ mean, float* __restrict__ inv, int mode, BnTrack tr) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = xg[c];
  for (int r = 1; r < n; r++) s += xg[(size_t)r * stride + c];
  if (mode == 2) {
    double q = xg[1024 + c];
    for (int r = 1; r < n; r++) q += xg[(size_t)r * stride + 1024 + c];
    const double mu = s / m;
    double var = q / m - mu * mu;
    var = var > 0 ? var : 0;
    mean[c] = (float)mu;
    inv[c] = 1.0f / sqrtf((float)var + eps);
    if (TRACK) { bn_track_mean(tr, c, mu); bn_track_var(tr, c, var); }   // (the global batch's values: the same bits on every rank)
    acc[c] = 0; acc[1024 + c] = 0;
  } else {
    if (mode == 0) mean[c] = (float)(s / m); else inv[c] = 1.0f / sqrtf((float)(s / m) + eps);
    if (TRACK) { if (mode == 0) bn_track_mean(tr, c, s / m); else bn_track_var(tr, c, s / m); }
    acc[c] = 0;
  }
}
// out[lo + i] = sum over ranks r (in rank order) of xg[r][lo + i], i < cnt: the head statistics, the cost and the backward BatchNorm sums
__global__ void k_sum_ranks(const double* __restrict__ xg, int n, int stride, double* __restrict__ out, int lo, int cnt) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  double s = xg[lo + i];
  for (int r = 1; r < n; r++) s += xg[(size_t)r * stride + lo + i];
  out[lo + i] = s;
}

// ---- tower BN apply (+ReLU, + dual add + ReLU).  z [pix][nbr*Kp]; gamma/beta [M][nbr*Kp]; out [pix][Kp] --------
// TIED (agz_trainer_create_tied; DESIGN §2 `tied-affine`): gamma / beta are ONE [HW][nbr*Kp] tensor shared by every board, indexed by the
// pixel within the board.  A template parameter: the <false> instantiation is the kernel that ran before the option existed.
template <bool TIED>
__device__ __forceinline__ int affine_row(int r, int HW) { return TIED ? r % HW : r; }
template <bool TIED>
__global__ void k_bn_apply(TGeo g, const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta,
                           const float* __restrict__ mean, const float* __restrict__ inv, float* __restrict__ out, int Kp, int nbr) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)g.M * Kp) return;
  int r = (int)(idx / Kp), c = (int)(idx - (size_t)r * Kp);
  size_t po = pix_off(g, r);
  int C = nbr * Kp;
  float acc = 0.f;
  for (int br = 0; br < nbr; br++) {
    int cc = br * Kp + c;
    float xh = (z[po * C + cc] - mean[cc]) * inv[cc];
    float y = gamma[(size_t)(TIED ? r % g.HW : r) * C + cc] * xh + beta[(size_t)(TIED ? r % g.HW : r) * C + cc];
    acc += y > 0.f ? y : 0.f;
  }
  out[po * Kp + c] = (nbr == 2) ? (acc > 0.f ? acc : 0.f) : acc;
}

// block-wide maximum of |.| bit patterns -> one atomicMax per block (the range word of the fp16x2 weight gradient's split)
__device__ __forceinline__ void block_amax_commit(unsigned m, unsigned* __restrict__ out_bits) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o, 64); m = t > m ? t : m; }
  __shared__ unsigned sm[4];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned a = sm[0] > sm[1] ? sm[0] : sm[1], b = sm[2] > sm[3] ? sm[2] : sm[3];
    atomicMax(out_bits, a > b ? a : b);
  }
}
// per-board maxima of a workgroup's rows (rows_per_block <= HW: at most two boards, bf and bf + 1) -> one atomicMax per board and block:
// the per-board range words the fp16x2 convolutions scale their input rows by (board_amax_parts_kernel swept the stored tensor for them)
__device__ __forceinline__ void board_amax_commit(unsigned m0, unsigned m1, int bf, int B, unsigned* __restrict__ board_bits) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t0 = (unsigned)__shfl_xor((int)m0, o, 64), t1 = (unsigned)__shfl_xor((int)m1, o, 64);
    m0 = t0 > m0 ? t0 : m0; m1 = t1 > m1 ? t1 : m1;
  }
  __shared__ unsigned sb[2][4];
  if ((threadIdx.x & 63) == 0) { sb[0][threadIdx.x >> 6] = m0; sb[1][threadIdx.x >> 6] = m1; }
  __syncthreads();
  if (threadIdx.x < 2 && bf + (int)threadIdx.x < B) {
    const unsigned* q = sb[threadIdx.x];
    const unsigned a = q[0] > q[1] ? q[0] : q[1], b = q[2] > q[3] ? q[2] : q[3];
    atomicMax(&board_bits[bf + threadIdx.x], a > b ? a : b);
  }
}
// The same apply, four channels per thread and a fixed channel quad per thread (Kp % 4 == 0, (Kp / 4) divides 256), with max|out| of
// the whole tensor as a by-product: the NEXT layer's weight gradient splits this tensor into fp16 pieces and needs its range — a
// separate sweep (k_absmax) re-read it.  Same expressions per element as k_bn_apply.
// ph != nullptr (round 5): the fp16 hi / lo planes of `out` that the NEXT layer's DMA convolution and weight gradient read are written
// here as well, scaled by the power of two of `est_bits` — the exact range of the same tensor one step earlier.  The exact range of THIS
// step comes out of this very pass; k_split_h2p_cond then keeps the planes if both ranges have the same exponent (the usual case: the
// scale is what the exact range prescribes, the results do not depend on the history) and re-splits the tensor otherwise.
// tests/test_train_history_gpu.py guards that promise: steps on a trainer with history against a fresh one (agz_trainer_last_planes).
__device__ __forceinline__ float wg_h2_scale(unsigned amax_bits);
typedef _Float16 bn_f16x4_t __attribute__((ext_vector_type(4)));
template <bool TIED>
__global__ __launch_bounds__(256) void k_bn_apply_v(TGeo g, const float* __restrict__ z, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ mean,
                                                    const float* __restrict__ inv, float* __restrict__ out, int Kp, int nbr,
                                                    int rows_per_block, unsigned* __restrict__ amax_bits, unsigned* __restrict__ board_bits,
                                                    _Float16* __restrict__ ph = nullptr, _Float16* __restrict__ pl = nullptr, const unsigned* __restrict__ est_bits = nullptr) {
  const int q = Kp >> 2, tpr = 256 / q, cq = threadIdx.x % q, rs = threadIdx.x / q;
  const float ps = ph ? wg_h2_scale(*est_bits) : 1.f;
  const int C = nbr * Kp;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  float4 mu[2], iv[2];
  for (int br = 0; br < nbr; br++) {
    mu[br] = reinterpret_cast<const float4*>(mean + br * Kp)[cq];
    iv[br] = reinterpret_cast<const float4*>(inv + br * Kp)[cq];
  }
  unsigned mx = 0, mb[2] = {0, 0};
  const int bf = r0 / g.HW, r_next = (bf + 1) * g.HW;   // (board_bits: rows_per_block <= HW, so rows >= r_next belong to board bf + 1)
  for (int r = r0 + rs; r < r1; r += tpr) {
    const size_t po = pix_off(g, r);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int br = 0; br < nbr; br++) {
      const float4 zz = reinterpret_cast<const float4*>(z + po * C + br * Kp)[cq];
      const float4 gm = reinterpret_cast<const float4*>(gamma + (size_t)affine_row<TIED>(r, g.HW) * C + br * Kp)[cq];
      const float4 bt = reinterpret_cast<const float4*>(beta + (size_t)affine_row<TIED>(r, g.HW) * C + br * Kp)[cq];
      const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, gv[4] = {gm.x, gm.y, gm.z, gm.w}, bv[4] = {bt.x, bt.y, bt.z, bt.w};
      const float mv[4] = {mu[br].x, mu[br].y, mu[br].z, mu[br].w}, nv[4] = {iv[br].x, iv[br].y, iv[br].z, iv[br].w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float xh = (zv[k] - mv[k]) * nv[k];
        const float y = gv[k] * xh + bv[k];
        acc[k] += y > 0.f ? y : 0.f;
      }
    }
    float o[4];
    unsigned rowm = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      o[k] = (nbr == 2) ? (acc[k] > 0.f ? acc[k] : 0.f) : acc[k];
      const unsigned b = __float_as_uint(o[k]) & 0x7fffffffu;
      rowm = b > rowm ? b : rowm;
    }
    mx = rowm > mx ? rowm : mx;
    if (r >= r_next) mb[1] = rowm > mb[1] ? rowm : mb[1]; else mb[0] = rowm > mb[0] ? rowm : mb[0];
    reinterpret_cast<float4*>(out + po * Kp)[cq] = make_float4(o[0], o[1], o[2], o[3]);
    if (ph) {
      bn_f16x4_t hh, ll;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float xs = o[k] * ps;
        hh[k] = (_Float16)xs;
        ll[k] = (_Float16)(xs - (float)hh[k]);
      }
      reinterpret_cast<bn_f16x4_t*>(ph + po * Kp)[cq] = hh;
      reinterpret_cast<bn_f16x4_t*>(pl + po * Kp)[cq] = ll;
    }
  }
  block_amax_commit(mx, amax_bits);
  if (board_bits) board_amax_commit(mb[0], mb[1], bf, g.B, board_bits);
}

// ---- tower BN backward, step 1: d(out) -> dgamma, dbeta, d(xhat) (stored in dz) and the two channel sums -------
// fuse_lr != 0 (single-process steps, agz_trainer_batch / agz_train_dev): the batch-shaped gamma / beta — 98 % of the learnables,
// 7.7 GB at G19 — take their SGD step HERE (w -= lr * grad on the value just read) instead of writing the gradient and having
// agz_trainer_apply sweep parameters and gradients again: 23 GB less traffic per step.  Same arithmetic (one fp32 multiply-subtract per
// element, as k_axpy); the gradients of these tensors are then not materialised (agz_trainer_forward_backward keeps them: the
// data-parallel path reduces them before its apply).
//
// SOLVER (agz_trainer_set_solver with any option != 0, fused steps only): the same in-place step through solver_step below — L2 with the
// gm / bt already in registers, the clamp, and with MOM the velocity of gamma / beta read and written at the same (r * C + cc) index of the
// flat velocity buffer.  A template parameter, not a run-time branch: the <false, false> instantiation is the code above, instruction for
// instruction (SolverDev is then an unused kernel argument).
//
// The template parameter is the solver kind: SK_VANILLA / SK_OPTIONS / SK_MOMENTUM are the three kernels above (the former <false, false>,
// <true, false>, <true, true>); SK_ADAM (agz_trainer_set_adam) steps gamma / beta through adam_step below, the two moments of each read and
// written at the same (r * C + cc) index of the flat moment buffers M1 / M2.  The Adam members of SolverDev come AFTER the ones that
// existed: the argument offsets the other three kinds read are the ones they always read.
enum SolverKind { SK_VANILLA = 0, SK_OPTIONS = 1, SK_MOMENTUM = 2, SK_ADAM = 3 };
// the per-step constants of Adam: beta, 1 - beta (rounded to float on the host), the bias corrections 1 / (1 - beta^t) (computed in
// double on the host, rounded once), eps
struct AdamK { float b1, omb1, b2, omb2, rc1, rc2, eps; };
struct SolverDev { float mu, l2, clip; float* vgamma; float* vbeta; AdamK ak; float* m1gamma; float* m1beta; float* m2gamma; float* m2beta; };
// One element of the solver step (gorgonia's VanillaSolver / Momentum as documented: L2, then clip, then the update), fp32:
//   g2 = g + l2 * w (l2 != 0);  g3 = clamp(g2, -clip, clip) (clip > 0);  MOM: v = mu * v + (-lr) * g3, w += v;  else w += (-lr) * g3
template <bool MOM>
__device__ __forceinline__ void solver_step(float& w, float& v, float gr, float lr, float mu, float l2, float clip) {
  if (l2 != 0.f) gr = gr + l2 * w;
  if (clip > 0.f) gr = fminf(fmaxf(gr, -clip), clip);
  if (MOM) { v = mu * v + (-lr) * gr; w = w + v; }
  else w = w + (-lr) * gr;
}
// One element of the Adam step (agz_trainer_set_adam; the declared definition of DESIGN §2 `solver-adam`), fp32 — the ONE statement of the
// arithmetic, called by the fused kernel and by the sweep:
//   g2 = g + l2 * w (l2 != 0);  g3 = clamp(g2, -clip, clip) (clip > 0);  m = b1 * m + (1 - b1) * g3;  v = b2 * v + (1 - b2) * g3^2;
//   w += (-lr) * ((m * rc1) / (sqrtf(v * rc2) + eps))
__device__ __forceinline__ void adam_step(float& w, float& m, float& v, float gr, float lr, float l2, float clip, const AdamK& a) {
  if (l2 != 0.f) gr = gr + l2 * w;
  if (clip > 0.f) gr = fminf(fmaxf(gr, -clip), clip);
  m = a.b1 * m + a.omb1 * gr;
  v = a.b2 * v + a.omb2 * (gr * gr);
  w = w + (-lr) * ((m * a.rc1) / (sqrtf(v * a.rc2) + a.eps));
}
template <int KIND>
__global__ void k_bn_bwd1(TGeo g, const float* __restrict__ z, float* gamma, float* beta,
                          const float* __restrict__ mean, const float* __restrict__ inv, const float* __restrict__ out,
                          const float* __restrict__ dout, float* __restrict__ dgamma, float* __restrict__ dbeta,
                          float* __restrict__ dz, double* __restrict__ s1, double* __restrict__ s2, int Kp, int nbr,
                          int rows_per_block, float fuse_lr, SolverDev sv) {
  constexpr bool SOLVER = KIND != SK_VANILLA, MOM = KIND == SK_MOMENTUM;
  int C = nbr * Kp;
  int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  for (int cc = threadIdx.x; cc < C; cc += blockDim.x) {
    int c = cc % Kp;
    double a1 = 0, a2 = 0;
    for (int r = r0; r < r1; r++) {
      size_t po = pix_off(g, r);
      float g0 = dout[po * Kp + c];
      if (nbr == 2 && !(out[po * Kp + c] > 0.f)) g0 = 0.f;
      float xh = (z[po * C + cc] - mean[cc]) * inv[cc];
      float gm = gamma[(size_t)r * C + cc];
      float bt = beta[(size_t)r * C + cc];
      float y = gm * xh + bt;
      float gg = y > 0.f ? g0 : 0.f;
      if (KIND == SK_ADAM) {  // (fused steps only: fuse_lr != 0)
        const size_t e = (size_t)r * C + cc;
        float wg = gm, wb = bt, mg = sv.m1gamma[e], ug = sv.m2gamma[e], mb = sv.m1beta[e], ub = sv.m2beta[e];
        adam_step(wg, mg, ug, gg * xh, fuse_lr, sv.l2, sv.clip, sv.ak);
        adam_step(wb, mb, ub, gg, fuse_lr, sv.l2, sv.clip, sv.ak);
        sv.m1gamma[e] = mg; sv.m2gamma[e] = ug; sv.m1beta[e] = mb; sv.m2beta[e] = ub;
        gamma[e] = wg;
        beta[e] = wb;
      } else if (SOLVER) {    // (fused steps only: fuse_lr != 0)
        float wg = gm, wb = bt, vg = 0.f, vb = 0.f;
        if (MOM) { vg = sv.vgamma[(size_t)r * C + cc]; vb = sv.vbeta[(size_t)r * C + cc]; }
        solver_step<MOM>(wg, vg, gg * xh, fuse_lr, sv.mu, sv.l2, sv.clip);
        solver_step<MOM>(wb, vb, gg, fuse_lr, sv.mu, sv.l2, sv.clip);
        if (MOM) { sv.vgamma[(size_t)r * C + cc] = vg; sv.vbeta[(size_t)r * C + cc] = vb; }
        gamma[(size_t)r * C + cc] = wg;
        beta[(size_t)r * C + cc] = wb;
      } else if (fuse_lr != 0.f) {   // (uniform) p += alpha * g with alpha = -lr, exactly k_axpy's expression
        gamma[(size_t)r * C + cc] = gm + (-fuse_lr) * (gg * xh);
        beta[(size_t)r * C + cc] = bt + (-fuse_lr) * gg;
      } else {
        dgamma[(size_t)r * C + cc] = gg * xh;
        dbeta[(size_t)r * C + cc] = gg;
      }
      float dxh = gg * gm;
      dz[po * C + cc] = dxh;
      a1 += dxh; a2 += (double)dxh * xh;
    }
    atomicAdd(&s1[cc], a1);
    atomicAdd(&s2[cc], a2);
  }
}
// ---- tied affine (agz_trainer_create_tied; DESIGN §2 `tied-affine`): step 1 with gamma / beta [HW][C] shared by every board ------------
// One workgroup owns 64 channels of ONE pixel p for all B boards: 256 threads = 64 channels x TB_RS row slices, slice s walks the boards
// b = s, s + TB_RS, ... (a wave reads 256 contiguous bytes of z per board).  Per element it does what k_bn_bwd1 does — gg, xhat,
// dz = gg * gamma, the channel sums — and accumulates dgamma = sum_b gg * xhat and dbeta = sum_b gg (each term the untied trainer's fp32
// per-row gradient) in double, in board order within the slice; the slices are then added in slice order through LDS and the sum is
// rounded once: no atomics, and the same bits for the same dout whatever the launch geometry.  Channels and pixels, not rows, are split
// across workgroups (grid = HW x ceil(C / 64): 2888 workgroups for 361 pixels x 512 channels).
// fuse_lr != 0: slice 0 — the owner of gamma / beta [p][cc]; every slice of this workgroup, the only readers of the element in the launch,
// read them before the barrier, so dz is computed with the value before the step — takes the solver step of its KIND in place (velocity or
// both moments at the same index) through tied_step (= solver_step / adam_step, out of line); no tied gradient is materialised.  Otherwise it stores dgamma, dbeta.
// The channel sums leave as per-pixel partial sums part[which][p][cc] (double) and k_bn_tied_sums adds them in a fixed order: s1 / s2 do not
// depend on the order workgroups finish in either (k_bn_bwd1 adds its blocks' sums with double atomics).
// SHARDED (agz_trainer_create_sharded_tied; a template parameter: the <KIND, false> instantiations are the kernels that ran before the form
// existed): the rank's rows are B of the n * B the gradient runs over, so nothing is rounded or stepped here.  dgamma / dbeta leave as this
// rank's DOUBLE partials — the very sum the plain form rounds — in the send buffer that follows the a1 / a2 partials in `part`:
// part = [a1 | a2] ([2][HW][2 Kp]) | s1 | s2 (2 x 1024, k_bn_tied_sums) | dgamma [HW][C] | dbeta [HW][C]; k_tied_ranks finishes them
// after the gather.  dz is computed from the gamma of before the step as in the plain form (k_tied_ranks steps later on the same stream).
constexpr int TB_RS = 4;
// The solver step of ONE tied gamma / beta element, compiled ONCE and out of line: solver_step's `mu * v + (-lr) * g` and adam_step's
// `b1 * m + (1 - b1) * g` each have two multiply-adds the compiler may contract them into, and it chooses per call site (inlined into
// k_bn_bwd1_tied it took fma(-lr, g, mu * v) where k_solver_sweep takes fma(mu, v, -(lr * g)): a fused momentum step differed from the
// two-pass step in the last bit).  The fused owner below and the two-pass sweep of the same tensors (k_tied_sweep) both CALL this one body,
// so the two paths of a tied trainer run the same instructions on the same operands.  Everything travels in registers (values in, a
// three-float struct out): no scratch.  a, b: the velocity (b unused) or Adam's two moments; gr: the gradient, grad_scale applied.
// This rests on the compiler honouring __noinline__; test_fused_step_is_the_two_pass_step_to_the_bit_where_a_step_is_one_workgroup
// (tests/test_tied_gpu.py) compares the two paths on bytes for every solver and is the guard: if it fails, look here first.
struct TiedSt { float w, a, b; };
template <int KIND>
__device__ __noinline__ TiedSt tied_step(float w, float a, float b, float gr, float lr, float mu, float l2, float clip, AdamK ak) {
  if (KIND == SK_ADAM) adam_step(w, a, b, gr, lr, l2, clip, ak);
  else solver_step<KIND == SK_MOMENTUM>(w, a, gr, lr, mu, l2, clip);
  return TiedSt{w, a, b};
}
// the two-pass solver step (agz_trainer_apply after agz_trainer_forward_backward, grad_scale honoured) of a tied trainer's tower gamma /
// beta: n elements of p / g (/ v, or m and m2) through tied_step.  0.13 GB per G19 trainer: one element per thread, grid-stride
template <int KIND>
__global__ __launch_bounds__(256) void k_tied_sweep(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v, float* __restrict__ m2,
                                                    size_t n, float lr, float gs, float mu, float l2, float clip, AdamK ak) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float a = KIND == SK_OPTIONS ? 0.f : v[i], b = KIND == SK_ADAM ? m2[i] : 0.f;
    const TiedSt r = tied_step<KIND>(p[i], a, b, gs * g[i], lr, mu, l2, clip, ak);
    p[i] = r.w;
    if (KIND != SK_OPTIONS) v[i] = r.a;
    if (KIND == SK_ADAM) m2[i] = r.b;
  }
}
template <int KIND, bool SHARDED = false>
__global__ __launch_bounds__(256) void k_bn_bwd1_tied(TGeo g, const float* __restrict__ z, float* gamma, float* beta,
                                                      const float* __restrict__ mean, const float* __restrict__ inv, const float* __restrict__ out,
                                                      const float* __restrict__ dout, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                      float* __restrict__ dz, double* __restrict__ part, int Kp, int nbr, float fuse_lr, SolverDev sv) {
  constexpr bool SOLVER = KIND != SK_VANILLA, MOM = KIND == SK_MOMENTUM;
  __shared__ double red[4][TB_RS - 1][64];
  const int C = nbr * Kp, chunks = (C + 63) >> 6;
  const int p = blockIdx.x / chunks, ch = blockIdx.x - p * chunks;
  const int lane = threadIdx.x & 63, rs = threadIdx.x >> 6;
  const int cc = ch * 64 + lane;
  const bool act = cc < C;
  const size_t e = (size_t)p * C + cc;
  // (dgamma / dbeta start from -0.0, the identity of IEEE addition: a sum of one row, and a slice without rows, leave the term as it is —
  // its sign of zero included — so that B = 1 stores the untied trainer's bits)
  double dg = -0.0, db = -0.0, a1 = 0, a2 = 0;
  float gm = 0.f, bt = 0.f;
  if (act) {
    const int c = cc % Kp;
    const int h = p / g.W, w = p - h * g.W;
    const float mu = mean[cc], iv = inv[cc];
    gm = gamma[e]; bt = beta[e];
    const size_t board = (size_t)g.Hp * g.Wp;
    size_t po = ((size_t)rs * g.Hp + h + 1) * g.Wp + w + 1;   // pix_off of row b * HW + p, b = rs
#pragma unroll 2
    for (int b = rs; b < g.B; b += TB_RS, po += TB_RS * board) {
      float g0 = dout[po * Kp + c];
      if (nbr == 2 && !(out[po * Kp + c] > 0.f)) g0 = 0.f;
      const float xh = (z[po * C + cc] - mu) * iv;
      const float y = gm * xh + bt;
      const float gg = y > 0.f ? g0 : 0.f;
      const float gx = gg * xh;
      dg += (double)gx; db += (double)gg;
      const float dxh = gg * gm;
      dz[po * C + cc] = dxh;
      a1 += dxh; a2 += (double)dxh * xh;
    }
  }
  if (rs > 0) { red[0][rs - 1][lane] = dg; red[1][rs - 1][lane] = db; red[2][rs - 1][lane] = a1; red[3][rs - 1][lane] = a2; }
  __syncthreads();
  if (rs != 0 || !act) return;
#pragma unroll
  for (int k = 0; k < TB_RS - 1; k++) { dg += red[0][k][lane]; db += red[1][k][lane]; a1 += red[2][k][lane]; a2 += red[3][k][lane]; }
  part[e] = a1;
  part[(size_t)g.HW * C + e] = a2;
  if (SHARDED) {   // (not rounded: the ranks' partials are added first)
    double* send = part + (size_t)4 * g.HW * Kp + 2048;
    send[e] = dg;
    send[(size_t)g.HW * C + e] = db;
    return;
  }
  const float fg = (float)dg, fb = (float)db;   // (rounded once)
  if (KIND == SK_ADAM) {  // (fused steps only: fuse_lr != 0)
    const TiedSt rg = tied_step<SK_ADAM>(gm, sv.m1gamma[e], sv.m2gamma[e], fg, fuse_lr, 0.f, sv.l2, sv.clip, sv.ak);
    const TiedSt rb = tied_step<SK_ADAM>(bt, sv.m1beta[e], sv.m2beta[e], fb, fuse_lr, 0.f, sv.l2, sv.clip, sv.ak);
    sv.m1gamma[e] = rg.a; sv.m2gamma[e] = rg.b; sv.m1beta[e] = rb.a; sv.m2beta[e] = rb.b;
    gamma[e] = rg.w;
    beta[e] = rb.w;
  } else if (SOLVER) {    // (fused steps only: fuse_lr != 0)
    float vg = 0.f, vb = 0.f;
    if (MOM) { vg = sv.vgamma[e]; vb = sv.vbeta[e]; }
    const TiedSt rg = tied_step<KIND>(gm, vg, 0.f, fg, fuse_lr, sv.mu, sv.l2, sv.clip, sv.ak);
    const TiedSt rb = tied_step<KIND>(bt, vb, 0.f, fb, fuse_lr, sv.mu, sv.l2, sv.clip, sv.ak);
    if (MOM) { sv.vgamma[e] = rg.a; sv.vbeta[e] = rb.a; }
    gamma[e] = rg.w;
    beta[e] = rb.w;
  } else if (fuse_lr != 0.f) {   // (uniform) p += alpha * g with alpha = -lr, exactly k_axpy's expression
    gamma[e] = gm + (-fuse_lr) * fg;
    beta[e] = bt + (-fuse_lr) * fb;
  } else {
    dgamma[e] = fg;
    dbeta[e] = fb;
  }
}
// s1[cc] = sum over the pixels p of part[0][p][cc]; s2 likewise from part[1].  A workgroup holds 16 channels x TS_NS pixel slices: slice k
// adds the pixels [k * TS_PS, (k + 1) * TS_PS) in pixel order (and every TS_NS-th such run after it, on boards of more than TS_NS * TS_PS
// pixels); the slices then meet in LDS and slice 0 adds them in slice order.  The order is fixed by HW alone, whatever the grid, and a board
// of up to TS_PS pixels is one run in pixel order.  (One thread per channel walking all 361 pixels, 16 waves in the whole launch, took
// 131 us per layer at G19 — one memory latency per pixel — and ate the saving of k_bn_bwd1_tied: profiles/tied/train_tied_kernel_stats.txt.)
constexpr int TS_NS = 16, TS_PS = 24;
__global__ __launch_bounds__(256) void k_bn_tied_sums(const double* __restrict__ part, int HW, int C, double* __restrict__ s1, double* __restrict__ s2) {
  __shared__ double red[TS_NS][16];
  const int ci = threadIdx.x & 15, k = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + ci;
  const bool act = i < 2 * C;
  int which = 0, cc = 0;
  double s = 0;
  if (act) {
    which = i / C; cc = i - which * C;
    const double* q = part + (size_t)which * HW * C + cc;
    for (int p0 = k * TS_PS; p0 < HW; p0 += TS_NS * TS_PS) {
      const int p1 = min(p0 + TS_PS, HW);
#pragma unroll 8
      for (int p = p0; p < p1; p++) s += q[(size_t)p * C];
    }
  }
  red[k][ci] = s;
  __syncthreads();
  if (k != 0 || !act) return;
  const int ns = min(TS_NS, (HW + TS_PS - 1) / TS_PS);
  for (int j = 1; j < ns; j++) s += red[j][ci];
  (which ? s2 : s1)[cc] = s;
}
// Tied head gamma / beta and FC biases: the head kernels write the untied trainer's per-row gradients into a scratch of the untied shapes;
// dst[i] = sum over the B rows, in row order, in double, rounded once, for up to five tensors in one launch (n[k] elements per row each)
// PART (tied sharded trainer): the sums leave unrounded, as doubles, one after the other in `part` (the tail of the heads' send buffer);
// k_rows_ranks adds the ranks' partials and rounds.  The <false> instantiation is the kernel that ran before the form existed.
struct RowSum { const float* src[5]; float* dst[5]; int n[5]; };
template <bool PART>
__global__ __launch_bounds__(256) void k_rows_sum(RowSum a, int B, double* __restrict__ part) {
  int i = blockIdx.x * 256 + threadIdx.x;
  const int i0 = i;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    if (i < a.n[k]) {
      double s = -0.0;   // (the identity of IEEE addition: one row is copied with its sign of zero)
      for (int b = 0; b < B; b++) s += (double)a.src[k][(size_t)b * a.n[k] + i];
      if (PART) part[i0] = s; else a.dst[k][i] = (float)s;
      return;
    }
    i -= a.n[k];
  }
}
// ---- tied sharded trainer (agz_trainer_create_sharded_tied; DESIGN §2 `tied-affine`): the gradient of a tied tensor from the n ranks' partials
// xg [n][stride] holds every rank's send buffer after the gather; `xg` points at the first partial of rank 0.  Per element the n double
// partials are added in RANK order, starting from rank 0's, and rounded once: no atomics, the same bits on every rank, and with n = 1 the
// tied trainer's bits.  k_tied_ranks: cnt elements of a tower layer's [gamma | beta] (contiguous in P / G / V / M1 / M2).  fuse_lr == 0
// (KIND = SK_VANILLA): the gradient is stored; a fused step takes the solver step of its KIND in place — the vanilla step with k_axpy's
// expression, the others through tied_step, the body k_bn_bwd1_tied and k_tied_sweep call — identically on every rank: the replicas of
// the parameters, the velocity and the moments stay equal without a broadcast.
template <int KIND>
__global__ __launch_bounds__(256) void k_tied_ranks(const double* __restrict__ xg, int n, size_t stride, size_t cnt, float* __restrict__ p,
                                                    float* __restrict__ gout, float* __restrict__ v, float* __restrict__ m2, float fuse_lr,
                                                    float mu, float l2, float clip, AdamK ak) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) {
    double s = xg[i];
    for (int r = 1; r < n; r++) s += xg[(size_t)r * stride + i];
    const float fg = (float)s;   // (rounded once)
    if (KIND == SK_VANILLA) {
      if (fuse_lr != 0.f) p[i] = p[i] + (-fuse_lr) * fg;   // (uniform) exactly k_axpy's expression
      else gout[i] = fg;
    } else {   // (fused steps only: fuse_lr != 0)
      const float a = KIND == SK_OPTIONS ? 0.f : v[i], b = KIND == SK_ADAM ? m2[i] : 0.f;
      const TiedSt r = tied_step<KIND>(p[i], a, b, fg, fuse_lr, mu, l2, clip, ak);
      p[i] = r.w;
      if (KIND != SK_OPTIONS) v[i] = r.a;
      if (KIND == SK_ADAM) m2[i] = r.b;
    }
  }
}
// the same finish for the five tied head tensors (head gamma / beta [3][HW], bp, b1, b2), whose partials k_rows_sum<true> left one after the
// other: always stored into G (the head region goes through the solver sweep of agz_trainer_apply on a fused step as well)
struct RowDst { float* dst[5]; int n[5]; };
__global__ __launch_bounds__(256) void k_rows_ranks(const double* __restrict__ xg, int n, size_t stride, RowDst a) {
  int i = blockIdx.x * 256 + threadIdx.x;
  const int i0 = i;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    if (i < a.n[k]) {
      double s = xg[i0];
      for (int r = 1; r < n; r++) s += xg[(size_t)r * stride + i0];
      a.dst[k][i] = (float)s;
      return;
    }
    i -= a.n[k];
  }
}
// step 2: dz = inv * (dxhat - s1/m - xhat*s2/m); m = the rows the sums run over (g.M, or the global batch's rows of a sharded trainer)
__global__ void k_bn_bwd2(TGeo g, const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ inv,
                          float* __restrict__ dz, const double* __restrict__ s1, const double* __restrict__ s2, int C, float m) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)g.M * C) return;
  int r = (int)(idx / C), cc = (int)(idx - (size_t)r * C);
  size_t po = pix_off(g, r);
  float xh = (z[po * C + cc] - mean[cc]) * inv[cc];
  dz[po * C + cc] = inv[cc] * (dz[po * C + cc] - (float)s1[cc] / m - xh * ((float)s2[cc] / m));
}

// step 2, four channels per thread, a fixed channel quad per thread (C % 4 == 0, (C / 4) divides 256: the per-channel terms are
// loaded once), with max|dz| of the tensor as a by-product (the weight gradient's range word).  Same expression per element.
__global__ __launch_bounds__(256) void k_bn_bwd2_v(TGeo g, const float* __restrict__ z, const float* __restrict__ mean,
                                                   const float* __restrict__ inv, float* __restrict__ dz, const double* __restrict__ s1,
                                                   const double* __restrict__ s2, int C, int rows_per_block, unsigned* __restrict__ amax_bits,
                                                   unsigned* __restrict__ board_bits, float m) {
  const int q = C >> 2, tpr = 256 / q, cq = threadIdx.x % q, rs = threadIdx.x / q;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  float mv[4], nv[4], a1[4], a2[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int cc = 4 * cq + k;
    mv[k] = mean[cc]; nv[k] = inv[cc]; a1[k] = (float)s1[cc] / m; a2[k] = (float)s2[cc] / m;
  }
  unsigned mx = 0, mb[2] = {0, 0};
  const int bf = r0 / g.HW, r_next = (bf + 1) * g.HW;
  for (int r = r0 + rs; r < r1; r += tpr) {
    const size_t po = pix_off(g, r);
    const float4 zz = reinterpret_cast<const float4*>(z + po * C)[cq];
    const float4 dd = reinterpret_cast<const float4*>(dz + po * C)[cq];
    const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, dv[4] = {dd.x, dd.y, dd.z, dd.w};
    float o[4];
    unsigned rowm = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float xh = (zv[k] - mv[k]) * nv[k];
      o[k] = nv[k] * (dv[k] - a1[k] - xh * a2[k]);
      const unsigned b = __float_as_uint(o[k]) & 0x7fffffffu;
      rowm = b > rowm ? b : rowm;
    }
    mx = rowm > mx ? rowm : mx;
    if (r >= r_next) mb[1] = rowm > mb[1] ? rowm : mb[1]; else mb[0] = rowm > mb[0] ? rowm : mb[0];
    reinterpret_cast<float4*>(dz + po * C)[cq] = make_float4(o[0], o[1], o[2], o[3]);
  }
  block_amax_commit(mx, amax_bits);
  if (board_bits) board_amax_commit(mb[0], mb[1], bf, g.B, board_bits);
}

// ---- weight gradient: dW[tap][n][c] += sum_r dz[pix(r)][n] * x[pix(r)+off(tap)][c]  (fp32 MFMA, split over rows) ----
// block tile 128 (n) x 128 (c), 4 waves x (2x2 MFMA 32x32x2), K-loop over `rows` GEMM rows in steps of 32; partial
// results are added with float atomics (one wgrad launch per layer; order-dependent rounding is within tolerance).
struct WgArgs {
  const float* dz; const float* x; float* dw;
  TGeo g; int N, Cin, rows_per_block, n_tiles, c_tiles, n_chunks;
};
__global__ __launch_bounds__(256) void k_wgrad(WgArgs a) {
  __shared__ float As[32][132];  // [k row][n]   (+4 pad: conflict-free ds_read_b32 across the two lane halves)
  __shared__ float Bs[32][132];  // [k row][c]
  int bid = blockIdx.x;
  int ct = bid % a.c_tiles; bid /= a.c_tiles;
  int nt = bid % a.n_tiles; bid /= a.n_tiles;
  int tap = bid % 9; int chunk = bid / 9;
  int n0 = nt * 128, c0 = ct * 128;
  int ky = tap / 3, kx = tap - ky * 3;
  long tapoff = (long)(ky - 1) * a.g.Wp + (kx - 1);
  int r_begin = chunk * a.rows_per_block, r_end = min(r_begin + a.rows_per_block, a.g.M);
  int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  f32x16 acc[2][2];
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  // staging: 32 rows x 128 cols = 1024 float4 / 256 threads = 4 each
  for (int rb = r_begin; rb < r_end; rb += 32) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int e = tid + 256 * q;        // float4 index
      int row = e >> 5, col = (e & 31) * 4;
      int r = rb + row;
      float4 va = make_float4(0, 0, 0, 0), vb = va;
      if (r < r_end) {
        size_t po = pix_off(a.g, r);
        if (n0 + col < a.N) va = *reinterpret_cast<const float4*>(a.dz + po * a.N + n0 + col);
        if (c0 + col < a.Cin) vb = *reinterpret_cast<const float4*>(a.x + (size_t)((long)po + tapoff) * a.Cin + c0 + col);
      }
      *reinterpret_cast<float4*>(&As[row][col]) = va;
      *reinterpret_cast<float4*>(&Bs[row][col]) = vb;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 32; k += 2) {
      int kr = k + (lane >> 5);
      float a0 = As[kr][wm * 64 + (lane & 31)], a1 = As[kr][wm * 64 + 32 + (lane & 31)];
      float b0 = Bs[kr][wn * 64 + (lane & 31)], b1 = Bs[kr][wn * 64 + 32 + (lane & 31)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        int n = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int c = c0 + wn * 64 + j * 32 + (lane & 31);
        if (n < a.N && c < a.Cin) atomicAdd(&a.dw[((size_t)tap * a.N + n) * a.Cin + c], acc[i][j][r]);
      }
}

// ---- the same weight gradient on the bf16 matrix pipe (AGZ_COMPUTE_BF16X3) ------------------------------------------------
// Both GEMM operands are activations here (dz and x), so both are split on the way into LDS: every fp32 value = three bf16
// pieces by exact truncation (conv_x3.hpp), six v_mfma_f32_32x32x16_bf16 per product instead of sixteen fp32-MFMA passes.  The
// reduction dimension is the pixel row r, and the MFMA wants eight consecutive k per lane: a thread fetches the SAME column of
// eight consecutive rows (a wave = 64 consecutive columns of one row per load: 256-byte runs), splits, and writes the eight
// bf16 of one piece as one 16-byte LDS word.  LDS image per operand and piece: [128 columns][32 k] bf16, the 16-byte slot of
// (column, k group) XOR-ed with bits 2..3 of the column: ds_write_b128 (16 lanes = 16 columns, one k group) and the fragment
// ds_read_b128 (16 lanes = 16 columns) both touch 16 different slots of the 256-byte bank window.
// Tile 128 (n) x 128 (c), 4 waves of 64 x 64, K step 32 rows; next step's 32 values per thread are fetched under the MFMAs.
typedef short wg_bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned wg_u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void wg_split(float v, unsigned& h, unsigned& m, unsigned& l) {
  unsigned hu = __float_as_uint(v) & 0xffff0000u;
  float r = v - __uint_as_float(hu);
  unsigned mu = __float_as_uint(r) & 0xffff0000u;
  float r2 = r - __uint_as_float(mu);
  h = hu; m = mu; l = __float_as_uint(r2);
}
__device__ __forceinline__ unsigned wg_pack(unsigned e0, unsigned e1) { return __builtin_amdgcn_perm(e1, e0, 0x07060302u); }
__device__ __forceinline__ unsigned wg_lds_off(int col, int kg) { return (unsigned)(col * 64 + ((kg ^ ((col >> 2) & 3)) << 4)); }

__global__ __launch_bounds__(256, 2) void k_wgrad_x3(WgArgs a) {
  constexpr int PIECE = 128 * 64;                 // one piece image of one operand: 128 columns x 32 k x 2 B
  __shared__ __attribute__((aligned(16))) unsigned char lds[6 * PIECE];   // A (dz) pieces 0..2, B (x) pieces 3..5
  // XCD-aware order: the 9 taps x tiles of one row chunk re-read the same dz / x rows (6 MB per 2048 rows at K = 256); workgroup ids
  // go round-robin over the 8 XCDs, so chunk c runs entirely on XCD c % 8 and its re-reads hit that XCD's L2 instead of missing in 8
  const int per_chunk = a.n_tiles * a.c_tiles * 9;
  const int local = (int)(blockIdx.x >> 3);
  const int chunk = (local / per_chunk) * 8 + (int)(blockIdx.x & 7);
  if (chunk >= a.n_chunks) return;
  int bid = local % per_chunk;
  const int ct = bid % a.c_tiles; bid /= a.c_tiles;
  const int nt = bid % a.n_tiles; bid /= a.n_tiles;
  const int tap = bid;
  const int n0 = nt * 128, c0 = ct * 128;
  const int ky = tap / 3, kx = tap - ky * 3;
  const long tapoff = (long)(ky - 1) * a.g.Wp + (kx - 1);
  const int r_begin = chunk * a.rows_per_block, r_end = min(r_begin + a.rows_per_block, a.g.M);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wid >> 1, wn = wid & 1;
  const int kg = wid;                             // staging: this wave's k group = rows rb + 8 kg .. + 7
  const bool na0 = n0 + lane < a.N, na1 = n0 + 64 + lane < a.N;
  const bool cb0 = c0 + lane < a.Cin, cb1 = c0 + 64 + lane < a.Cin;
  // (buffer loads, masked lanes and rows past the chunk read zero through an out-of-range offset: see k_wgrad_h2)
  const size_t n_pix = (size_t)a.g.B * a.g.Hp * a.g.Wp;
  const __amdgpu_buffer_rsrc_t rdz = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dz), 0, (int)(n_pix * a.N * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)(n_pix * a.Cin * 4), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  float va0[8], va1[8], vb0[8], vb1[8];
  auto fetch = [&](int rb) {
    const int r0 = rb + kg * 8;                   // wave-uniform
    int b = r0 / a.g.HW, p = r0 - b * a.g.HW;
    int h = p / a.g.W, w = p - h * a.g.W;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      // (rows past the last board lie past the end of both buffers and read zero; chunk ends are multiples of the 32-row K step)
      const int po = (b * a.g.Hp + h + 1) * a.g.Wp + w + 1;
      const unsigned oa = (unsigned)(po * a.N + n0 + lane) * 4u;
      const unsigned ob = (unsigned)((po + (int)tapoff) * a.Cin + c0 + lane) * 4u;
      va0[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rdz, na0 ? oa : OOB, 0, 0));
      va1[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rdz, na1 ? oa + 256u : OOB, 0, 0));
      vb0[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, cb0 ? ob : OOB, 0, 0));
      vb1[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, cb1 ? ob + 256u : OOB, 0, 0));
      const bool we = ++w == a.g.W;                 // (selects, not branches)
      w = we ? 0 : w; h += we ? 1 : 0;
      const bool he = h == a.g.H;
      h = he ? 0 : h; b += he ? 1 : 0;
    }
  };
  auto stage = [&](const float* v, int piece0, int col) {   // split eight k of one column, one 16-byte word per piece
    unsigned hh[8], mm[8], ll[8];
#pragma unroll
    for (int q = 0; q < 8; q++) wg_split(v[q], hh[q], mm[q], ll[q]);
    wg_u32x4_t ph, pm, pl;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      ph[q] = wg_pack(hh[2 * q], hh[2 * q + 1]);
      pm[q] = wg_pack(mm[2 * q], mm[2 * q + 1]);
      pl[q] = wg_pack(ll[2 * q], ll[2 * q + 1]);
    }
    const unsigned off = wg_lds_off(col, kg);
    *reinterpret_cast<wg_u32x4_t*>(lds + (piece0 + 0) * PIECE + off) = ph;
    *reinterpret_cast<wg_u32x4_t*>(lds + (piece0 + 1) * PIECE + off) = pm;
    *reinterpret_cast<wg_u32x4_t*>(lds + (piece0 + 2) * PIECE + off) = pl;
  };
  fetch(r_begin);
  for (int rb = r_begin; rb < r_end; rb += 32) {
    stage(va0, 0, lane); stage(va1, 0, 64 + lane);
    stage(vb0, 3, lane); stage(vb1, 3, 64 + lane);
    __syncthreads();
    if (rb + 32 < r_end) fetch(rb + 32);          // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const int kgr = ks * 2 + (lane >> 5);
      wg_bf16x8_t A_[2][3], B_[2][3];
#pragma unroll
      for (int pz = 0; pz < 3; pz++) {
#pragma unroll
        for (int i = 0; i < 2; i++)
          A_[i][pz] = *reinterpret_cast<const wg_bf16x8_t*>(lds + pz * PIECE + wg_lds_off(wm * 64 + i * 32 + (lane & 31), kgr));
#pragma unroll
        for (int j = 0; j < 2; j++)
          B_[j][pz] = *reinterpret_cast<const wg_bf16x8_t*>(lds + (3 + pz) * PIECE + wg_lds_off(wn * 64 + j * 32 + (lane & 31), kgr));
      }
#define WG_MF(I, J, PA, PB) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_[I][PA], B_[J][PB], acc[I][J], 0, 0, 0);
#define WG_QUAD(PA, PB) WG_MF(0, 0, PA, PB) WG_MF(0, 1, PA, PB) WG_MF(1, 0, PA, PB) WG_MF(1, 1, PA, PB)
      WG_QUAD(2, 0) WG_QUAD(0, 2) WG_QUAD(1, 1) WG_QUAD(1, 0) WG_QUAD(0, 1) WG_QUAD(0, 0)   // smallest terms first
#undef WG_QUAD
#undef WG_MF
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        int n = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int c = c0 + wn * 64 + j * 32 + (lane & 31);
        if (n < a.N && c < a.Cin) atomicAdd(&a.dw[((size_t)tap * a.N + n) * a.Cin + c], acc[i][j][r]);
      }
}

// ---- the weight gradient with fp16x2 products (AGZ_COMPUTE_WINO_H2) --------------------------------------------------------
// k_wgrad_x3 spends as many cycles splitting as multiplying: every element of dz and x is split (4 VALU ops + packing) by each of the
// 9 tap workgroups that read it, and a product costs six MFMAs.  Here both operands are split ONCE per layer by an elementwise pass
// (k_absmax -> power-of-two scale putting the tensor's maximum into [2^13, 2^14); k_split_h2 writes hi = RN16(v s), lo = RN16(v s - hi)
// as one 32-bit word per element, 4 bytes like the fp32 it replaces), the GEMM's staging only regroups eight rows of a column into
// 16-byte words (one v_perm per two halves), and a product is three v_mfma_f32_32x32x16_f16 (hi hi, hi lo, lo hi; the dropped
// lo lo <= 2^-22 relative).  hi + lo carries v s to an absolute error <= 2^-25 (scaled units) = 2^-38 of the tensor's range.
// The sums come out scaled by s_dz s_x and are un-scaled (exact powers of two) before the atomic add.
typedef _Float16 wg_f16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float wg_h2_scale(unsigned amax_bits) {   // 2^(13 - E(amax)); 1 for an all-zero (or non-finite) tensor
  const int e = (int)((amax_bits >> 23) & 0xff);
  if (e == 0 || e == 255) return 1.f;
  int se = 127 + 13 - (e - 127);
  se = se < 1 ? 1 : (se > 254 ? 254 : se);
  return __uint_as_float((unsigned)se << 23);
}
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ x, size_t n4, unsigned* __restrict__ out_bits) {
  unsigned m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const unsigned a = __float_as_uint(v.x) & 0x7fffffffu, b = __float_as_uint(v.y) & 0x7fffffffu;
    const unsigned c = __float_as_uint(v.z) & 0x7fffffffu, d = __float_as_uint(v.w) & 0x7fffffffu;
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d, q = ab > cd ? ab : cd;
    m = q > m ? q : m;
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o, 64); m = t > m ? t : m; }
  __shared__ unsigned sm[4];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned a = sm[0] > sm[1] ? sm[0] : sm[1], b = sm[2] > sm[3] ? sm[2] : sm[3];
    atomicMax(out_bits, a > b ? a : b);
  }
}
__global__ __launch_bounds__(256) void k_split_h2(const float* __restrict__ x, unsigned* __restrict__ y, size_t n4, const unsigned* __restrict__ amax_bits) {
  const float s = wg_h2_scale(*amax_bits);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const float in[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
    unsigned o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const _Float16 hi = (_Float16)in[k];
      const _Float16 lo = (_Float16)(in[k] - (float)hi);
      o[k] = (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
    }
    reinterpret_cast<uint4*>(y)[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
struct WgH2Args {
  const unsigned* dz2; const unsigned* x2;   // (hi | lo << 16) per element, the layouts of dz and x
  const unsigned* amax;                      // [0] dz, [1] x: bits of max|.|
  float* dw;
  TGeo g; int N, Cin, rows_per_block, n_tiles, c_tiles, n_chunks;
};
// LDS image of this kernel: [k group of 8 rows (4)][column slot (128)][16 B = 8 k], slot = column with its low two bits XORed by
// bits 4-5 (the staging writes of a half wave — columns 4 cg + c, 8 bytes each — then fall on 16 distinct 16-byte bank groups, and the
// fragment reads of 32 consecutive columns stay a permutation of 32 consecutive slots)
__device__ __forceinline__ unsigned wg2_lds_off(int col, int kg) { return (unsigned)(kg * 2048 + ((col ^ ((col >> 4) & 3)) << 4)); }
typedef unsigned wg_u32x2_t __attribute__((ext_vector_type(2)));
// Loads are 16 bytes (four channels of one row), 8 per thread and step, the next step's issued under this step's MFMAs.  Deeper
// prefetch (2-4 steps in flight in registers) measured no faster, 4 workgroups per CU (this form: 123 registers) 0.67 ms per G19
// layer against 0.76 for round 3's kernel (profiles/r04/wgrad_ab.log): the bound is the L2 -> CU operand stream (see k_wgrad_h2t3, which
// replaces this kernel on boards >= 16 wide).
__global__ __launch_bounds__(256, 2) void k_wgrad_h2(WgH2Args a) {
  constexpr int D = 1;                             // K steps in flight in registers (2, 3, 4 measured no faster: the comment above)
  constexpr int PIECE = 128 * 64;                 // one piece image of one operand: 128 columns x 32 k x 2 B
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * PIECE];   // A (dz) hi, lo; B (x) hi, lo
  // XCD-aware order: the 9 taps x tiles of one row chunk re-read the same dz / x rows (6 MB per 2048 rows at K = 256); workgroup ids
  // go round-robin over the 8 XCDs, so chunk c runs entirely on XCD c % 8 and its re-reads hit that XCD's L2 instead of missing in 8
  const int per_chunk = a.n_tiles * a.c_tiles * 9;
  const int local = (int)(blockIdx.x >> 3);
  const int chunk = (local / per_chunk) * 8 + (int)(blockIdx.x & 7);
  if (chunk >= a.n_chunks) return;
  int bid = local % per_chunk;
  const int ct = bid % a.c_tiles; bid /= a.c_tiles;
  const int nt = bid % a.n_tiles; bid /= a.n_tiles;
  const int tap = bid;
  const int n0 = nt * 128, c0 = ct * 128;
  const int ky = tap / 3, kx = tap - ky * 3;
  const int tapoff = (ky - 1) * a.g.Wp + (kx - 1);
  const int r_begin = chunk * a.rows_per_block, r_end = min(r_begin + a.rows_per_block, a.g.M);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wid >> 1, wn = wid & 1;
  const int cg = lane & 31, half = lane >> 5;     // staging: columns 4 cg .. + 3, rows 8 wid + 4 half .. + 3 of the step
  const bool na = n0 + 4 * cg < a.N, cb = c0 + 4 * cg < a.Cin;   // (N and Cin are multiples of 4)
  // buffer loads with a per-lane byte offset: masked lanes and rows past the chunk get an out-of-range offset and read zero — a
  // conditional global_load costs a saveexec + two branches per load
  const size_t n_pix = (size_t)a.g.B * a.g.Hp * a.g.Wp;
  const __amdgpu_buffer_rsrc_t rdz = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(a.dz2), 0, (int)(n_pix * a.N * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(a.x2), 0, (int)(n_pix * a.Cin * 4), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  wg_u32x4_t va[D][4], vb[D][4];
  auto fetch = [&](wg_u32x4_t* pa, wg_u32x4_t* pb, int rb) {
    const int r0 = rb + wid * 8;                  // wave-uniform
    int b = r0 / a.g.HW, p = r0 - b * a.g.HW;
    int h = p / a.g.W, w = p - h * a.g.W;
    int r = r0 + 4 * half;
#pragma unroll
    for (int q = 0; q < 4; q++) {                 // the upper half wave starts four rows on (selects, not branches)
      const bool adv = half != 0;
      const bool we = adv && (w + 1 == a.g.W);
      w = adv ? (we ? 0 : w + 1) : w; h += we ? 1 : 0;
      const bool he = h == a.g.H;
      h = he ? 0 : h; b += he ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      // (rows past the last board lie past the end of both buffers and read zero; rows of the padding steps past the chunk are masked)
      const int po = (b * a.g.Hp + h + 1) * a.g.Wp + w + 1;
      const bool in = r + q < r_end;
      const unsigned oa = (unsigned)(po * a.N + n0 + 4 * cg) * 4u;
      const unsigned ob = (unsigned)((po + tapoff) * a.Cin + c0 + 4 * cg) * 4u;
      pa[q] = __builtin_bit_cast(wg_u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rdz, (na && in) ? oa : OOB, 0, 0));
      pb[q] = __builtin_bit_cast(wg_u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rx, (cb && in) ? ob : OOB, 0, 0));
      const bool we = ++w == a.g.W;
      w = we ? 0 : w; h += we ? 1 : 0;
      const bool he = h == a.g.H;
      h = he ? 0 : h; b += he ? 1 : 0;
    }
  };
  auto stage = [&](const wg_u32x4_t* v, int piece0) {   // four k of four columns: per column one 8-byte word of hi halves, one of lo halves
#pragma unroll
    for (int c = 0; c < 4; c++) {
      wg_u32x2_t ph, pl;
      ph[0] = __builtin_amdgcn_perm(v[1][c], v[0][c], 0x05040100u);
      ph[1] = __builtin_amdgcn_perm(v[3][c], v[2][c], 0x05040100u);
      pl[0] = __builtin_amdgcn_perm(v[1][c], v[0][c], 0x07060302u);
      pl[1] = __builtin_amdgcn_perm(v[3][c], v[2][c], 0x07060302u);
      const unsigned off = wg2_lds_off(4 * cg + c, wid) + 8u * half;
      *reinterpret_cast<wg_u32x2_t*>(lds + (piece0 + 0) * PIECE + off) = ph;
      *reinterpret_cast<wg_u32x2_t*>(lds + (piece0 + 1) * PIECE + off) = pl;
    }
  };
#pragma unroll
  for (int d = 0; d < D; d++) {
    fetch(va[d], vb[d], r_begin + 32 * d);
    __builtin_amdgcn_sched_barrier(0);            // issue order = consumption order: the loop's waits count loads, whichever edge it is entered by
  }
  // (the step count is rounded up to a multiple of D: the padding steps multiply zeros)
  for (int rb = r_begin; rb < r_end; rb += 32 * D) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      stage(va[d], 0); stage(vb[d], 2);
      __syncthreads();
      fetch(va[d], vb[d], rb + 32 * (d + D));     // in flight under the next D steps
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
        const int kgr = ks * 2 + (lane >> 5);
        wg_f16x8_t A_[2][2], B_[2][2];
#pragma unroll
        for (int pz = 0; pz < 2; pz++) {
#pragma unroll
          for (int i = 0; i < 2; i++)
            A_[i][pz] = *reinterpret_cast<const wg_f16x8_t*>(lds + pz * PIECE + wg2_lds_off(wm * 64 + i * 32 + (lane & 31), kgr));
#pragma unroll
          for (int j = 0; j < 2; j++)
            B_[j][pz] = *reinterpret_cast<const wg_f16x8_t*>(lds + (2 + pz) * PIECE + wg2_lds_off(wn * 64 + j * 32 + (lane & 31), kgr));
        }
#define WG_MF(I, J, PA, PB) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A_[I][PA], B_[J][PB], acc[I][J], 0, 0, 0);
#define WG_QUAD(PA, PB) WG_MF(0, 0, PA, PB) WG_MF(0, 1, PA, PB) WG_MF(1, 0, PA, PB) WG_MF(1, 1, PA, PB)
        WG_QUAD(1, 0) WG_QUAD(0, 1) WG_QUAD(0, 0)   // smaller terms first
#undef WG_QUAD
#undef WG_MF
      }
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);          // (the next step's regrouping hoisted into these MFMAs would wait on the NEWEST loads)
    }
  }
  const float un = 1.f / (wg_h2_scale(a.amax[0]) * wg_h2_scale(a.amax[1]));   // exact: a power of two
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        int n = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int c = c0 + wn * 64 + j * 32 + (lane & 31);
        if (n < a.N && c < a.Cin) atomicAdd(&a.dw[((size_t)tap * a.N + n) * a.Cin + c], acc[i][j][r] * un);
      }
}

// ---- the weight gradient with the operands DMA'd into LDS and transposed by the LDS read (gfx950: ds_read_b64_tr_b16) ---------------
// What bounds the register-staged kernel above is the L2 -> CU operand stream: 32 KB per workgroup and K step for 128 x 128 x 32
// products is 6.9 GB per G19 layer, 10.3 TB/s at 0.67 ms — the rate round 3's l2_probe and round 4's all-from-cache GEMM floor gave
// for that path (a single-tap DMA form of the same tile measured 0.88 ms: the same bytes through the narrower DMA path).  Fewer
// bytes per product: the three taps of one kernel ROW read the same dz rows and x rows one pixel apart.  k_split_h2p writes the hi
// and lo halves as two fp16 planes in the operand's own [pixel][channel] layout; a plane's rows arrive by buffer_load ... lds
// (16 bytes per lane: one row, eight channels; each lane computes ITS row's padded pixel, so shifts and masks cost nothing) into
// the image [row / 4][channel / 8 (16)][row % 4][16 B] — a DMA instruction fills 1 KB (four rows) — and are read k-major by the
// transposing LDS read: within 16 lanes, lane i supplies the address of (row i / 4, channels 4 (i % 4) .. + 3) and receives channel
// i's four rows (scripts/probes/tr16_probe.hip confirms the lane mapping); the 32 lanes such a read serves per cycle touch 256
// contiguous bytes.  The x image is indexed by PADDED PIXEL (40 consecutive pixels cover a step's 32 rows, its <= 2 row ends and the
// +-1 shifts): one landing serves all three taps, row of (k, kx) = delta(k) + kx, delta(k) = k + 2 (row ends between the step's first
// row and row k).  36 KB per step for 3 x the products: 2.6 x less traffic per product.  K steps never straddle a board (12 steps of 32
// rows per 19 x 19 board, the last one 9 rows + zeros: 6 % padding).  Boards >= 16 wide (two row ends per step at most); others keep
// the register-staged kernel.  G19 layer: 0.55 ms (0.76 in round 3); without the DMA 0.41, DMA alone 0.34, neither 0.12 (the
// epilogue's float atomics): landing and arithmetic of two workgroups per CU overlap only partly (profiles/r04/wgrad_ab.log).
typedef short wg_s4_t __attribute__((vector_size(8)));
typedef _Float16 wg_f16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* wg_lds_ptr_t;
typedef unsigned wg_rsrc_t __attribute__((ext_vector_type(4)));
// One LDS-DMA instruction, written out: the compiler's own bookkeeping of buffer_load ... lds keeps at most eight such stores apart and
// waits vmcnt(0) before LDS reads it can no longer tell from the NEXT stage's DMA (seen in the ISA: a drain in the middle of every K
// step).  As inline assembly the DMA is invisible to that pass; the waits are the counted ones below.  (Compiler-known vector-memory
// instructions stay safe: its counts can only be too strict, never too loose, with extra loads in flight.)
__device__ __forceinline__ void wg_dma16(wg_rsrc_t rsrc, unsigned lds_addr, unsigned voff) {
  unsigned keep;                                   // (M0 is put back: the compiler does not model assembly writes to it)
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(rsrc) : "memory");
}
typedef __attribute__((address_space(3))) wg_s4_t* wg_lds_s4_t;
__global__ __launch_bounds__(256) void k_split_h2p(const float* __restrict__ x, _Float16* __restrict__ yh, _Float16* __restrict__ yl, size_t n4,
                                                   const unsigned* __restrict__ amax_bits) {
  const float s = wg_h2_scale(*amax_bits);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const float in[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
    wg_f16x4_t h, l;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      h[k] = (_Float16)in[k];
      l[k] = (_Float16)(in[k] - (float)h[k]);
    }
    reinterpret_cast<wg_f16x4_t*>(yh)[i] = h;
    reinterpret_cast<wg_f16x4_t*>(yl)[i] = l;
  }
}
// the same split, skipped when the planes already hold it: written by k_bn_apply_v under the previous step's range `est_bits`, valid when
// that range and this step's exact one prescribe the same power of two
__global__ __launch_bounds__(256) void k_split_h2p_cond(const float* __restrict__ x, _Float16* __restrict__ yh, _Float16* __restrict__ yl, size_t n4,
                                                        const unsigned* __restrict__ amax_bits, const unsigned* __restrict__ est_bits) {
  if (est_bits && *est_bits != 0u && wg_h2_scale(*est_bits) == wg_h2_scale(*amax_bits)) return;
  const float s = wg_h2_scale(*amax_bits);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const float in[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
    wg_f16x4_t h, l;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      h[k] = (_Float16)in[k];
      l[k] = (_Float16)(in[k] - (float)h[k]);
    }
    reinterpret_cast<wg_f16x4_t*>(yh)[i] = h;
    reinterpret_cast<wg_f16x4_t*>(yl)[i] = l;
  }
}
struct WgH2t3Args {
  const _Float16 *dzh, *dzl, *xh, *xl;
  const unsigned* amax;
  float* dw;
  TGeo g; int N, Cin, steps_per_board, n_tiles, c_tiles, n_chunks;
};
__global__ __launch_bounds__(256, 2) void k_wgrad_h2t3(WgH2t3Args a) {
  constexpr int PA = 32 * 128 * 2, PB = 40 * 128 * 2, STAGE = 2 * PA + 2 * PB;   // dz hi, lo (32 rows); x hi, lo (40 pixels)
  __shared__ __attribute__((aligned(1024))) unsigned char lds0[STAGE];
  __shared__ __attribute__((aligned(1024))) unsigned char lds1[STAGE];
  const int per_chunk = a.n_tiles * a.c_tiles * 3;   // XCD-aware order, as above
  const int local = (int)(blockIdx.x >> 3);
  const int chunk = (local / per_chunk) * 8 + (int)(blockIdx.x & 7);
  if (chunk >= a.n_chunks) return;
  int bid = local % per_chunk;
  const int ct = bid % a.c_tiles; bid /= a.c_tiles;
  const int nt = bid % a.n_tiles; bid /= a.n_tiles;
  const int ky = bid;
  const int n0 = nt * 128, c0 = ct * 128;
  const int b_begin = (int)((long)chunk * a.g.B / a.n_chunks), b_end = (int)((long)(chunk + 1) * a.g.B / a.n_chunks);   // 6 or 7 boards, say
  const int n_steps = (b_end - b_begin) * a.steps_per_board;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wid >> 1, wn = wid & 1;
  const int cs = lane >> 2, kk = lane & 3;        // DMA: this lane's eight channels and row of a four-row group
  const bool na = n0 + 8 * cs < a.N, cb = c0 + 8 * cs < a.Cin;
  const size_t n_pix = (size_t)a.g.B * a.g.Hp * a.g.Wp;
  auto mk = [](const void* p, size_t bytes) -> wg_rsrc_t {
    const unsigned long long u = (unsigned long long)p;
    wg_rsrc_t r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)u); r[1] = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane((unsigned)bytes); r[3] = 0x00020000u;
    return r;
  };
  const wg_rsrc_t rah = mk(a.dzh, n_pix * a.N * 2), ral = mk(a.dzl, n_pix * a.N * 2);
  const wg_rsrc_t rbh = mk(a.xh, n_pix * a.Cin * 2), rbl = mk(a.xl, n_pix * a.Cin * 2);
  constexpr unsigned OOB = 0x80000000u;
  f32x16 acc[3][2][2];
#pragma unroll
  for (int t = 0; t < 3; t++)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][i][j][r] = 0.f;
  // step s of the chunk: board b_begin + s / steps_per_board, rows 32 (s % steps_per_board) .. of that board
  struct Step { int po0, w0, nv; };
  auto step_of = [&](int s) -> Step {
    const int bq = s / a.steps_per_board, sib = s - bq * a.steps_per_board;
    const int r0 = sib * 32, h0 = r0 / a.g.W, w0 = r0 - h0 * a.g.W;
    Step st;
    st.po0 = ((b_begin + bq) * a.g.Hp + h0 + 1) * a.g.Wp + w0 + 1;
    st.w0 = w0;
    st.nv = s < n_steps ? min(32, a.g.HW - r0) : 0;   // (a padding step past the chunk lands zeros)
    return st;
  };
  auto delta = [&](int k, int w0) -> int {         // padded-pixel distance of the step's row k from its first row (boards >= 16 wide)
    const int c = w0 + k;
    return k + (c >= a.g.W ? 2 : 0) + (c >= 2 * a.g.W ? 2 : 0);
  };
  // the landing of step s, in five pieces (two for dz: wave w lands rows 8 w .. 8 w + 7; three for x: ten four-row groups, waves 0, 1
  // land three, waves 2, 3 two) so that they can be issued BETWEEN the MFMA groups of the step before: as one block ahead of the
  // barrier their address arithmetic and issue slots (~0.4 us) delayed every step
  auto issue_piece = [&](unsigned char* stage, const Step& st, int piece) {
    const unsigned base = (unsigned)(size_t)(wg_lds_ptr_t)stage;
    if (piece < 2) {
      const int t = piece;
      const int k = 8 * wid + 4 * t + kk;
      const int po = st.po0 + delta(k, st.w0);
      const unsigned oa = (na && k < st.nv) ? (unsigned)(po * a.N + n0 + 8 * cs) * 2u : OOB;
      const unsigned d = base + (unsigned)(2 * wid + t) * 1024u;
      wg_dma16(rah, d, oa);
      wg_dma16(ral, d + PA, oa);
    } else {
      const int qb = st.po0 + (ky - 1) * a.g.Wp - 1;   // x: image row rho <-> padded pixel qb + rho (halo pixels hold zeros)
      const int m = wid + 4 * (piece - 2);
      if (m < 10) {
        const int q = qb + 4 * m + kk;
        const unsigned ob = (cb && st.nv > 0 && q >= 0) ? (unsigned)(q * a.Cin + c0 + 8 * cs) * 2u : OOB;
        const unsigned d = base + 2 * PA + (unsigned)m * 1024u;
        wg_dma16(rbh, d, ob);
        wg_dma16(rbl, d + PB, ob);
      }
    }
  };
  const int i16 = lane & 15, kh = lane >> 5;
  const unsigned cpart = (unsigned)(((((lane >> 4) & 1) * 2 + ((i16 & 3) >> 1)) * 4) * 16 + (i16 & 1) * 8);   // channel part of a read address
  const unsigned foa = (unsigned)(kh * 2048 + (i16 >> 2) * 16) + cpart;                                   // dz: rows are the k themselves
  auto tr2 = [&](const unsigned char* p0, const unsigned char* p1) -> wg_f16x8_t {
    const wg_s4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s4_t)(p0));
    const wg_s4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s4_t)(p1));
    return __builtin_shufflevector(__builtin_bit_cast(wg_f16x4_t, v0), __builtin_bit_cast(wg_f16x4_t, v1), 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto compute = [&](const unsigned char* stage, int s, unsigned char* next_stage) {
    const int w0 = step_of(s).w0;
    const Step nx = step_of(s + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      wg_f16x8_t A_[2][2];
#pragma unroll
      for (int pz = 0; pz < 2; pz++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const unsigned char* q = stage + pz * PA + foa + (wm * 64 + i * 32) * 8 + ks * 4096;
          A_[i][pz] = tr2(q, q + 1024);
        }
      const int k0 = ks * 16 + kh * 8 + (i16 >> 2);  // this lane's rows of the step: k0 and k0 + 4
      const int d0 = delta(k0, w0), d1 = delta(k0 + 4, w0);
#pragma unroll
      for (int kx = 0; kx < 3; kx++) {
        const int r0 = d0 + kx, r1 = d1 + kx;
        const unsigned o0 = (unsigned)((r0 >> 2) * 1024 + (r0 & 3) * 16) + cpart, o1 = (unsigned)((r1 >> 2) * 1024 + (r1 & 3) * 16) + cpart;
        wg_f16x8_t B_[2][2];
#pragma unroll
        for (int pz = 0; pz < 2; pz++)
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const unsigned char* q = stage + 2 * PA + pz * PB + (wn * 64 + j * 32) * 8;
            B_[j][pz] = tr2(q + o0, q + o1);
          }
#define WG_MF(I, J, PA_, PB_) acc[kx][I][J] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A_[I][PA_], B_[J][PB_], acc[kx][I][J], 0, 0, 0);
#define WG_QUAD(PA_, PB_) WG_MF(0, 0, PA_, PB_) WG_MF(0, 1, PA_, PB_) WG_MF(1, 0, PA_, PB_) WG_MF(1, 1, PA_, PB_)
        WG_QUAD(1, 0) WG_QUAD(0, 1) WG_QUAD(0, 0)   // smaller terms first
#undef WG_QUAD
#undef WG_MF
        const int piece = ks * 3 + kx;               // next step's landing, a piece after each of the first five MFMA groups
        if (piece < 5) issue_piece(next_stage, nx, piece);
      }
    }
  };
  // raw s_barrier + explicit vmcnt: a __syncthreads() fence knows nothing of the assembly DMA
  {
    const Step st0 = step_of(0);
#pragma unroll
    for (int piece = 0; piece < 5; piece++) issue_piece(lds0, st0, piece);
  }
  for (int s = 0; s < n_steps; s += 2) {            // (an odd step count runs one step of zeros)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of step s has landed; after the barrier every wave's
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    compute(lds0, s, lds1);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                    // (also: every wave is done reading lds0 before step s + 2 lands there)
    __builtin_amdgcn_sched_barrier(0);
    compute(lds1, s + 1, lds0);
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const float un = 1.f / (wg_h2_scale(a.amax[0]) * wg_h2_scale(a.amax[1]));   // exact: a power of two
#pragma unroll
  for (int kx = 0; kx < 3; kx++)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          int n = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          int c = c0 + wn * 64 + j * 32 + (lane & 31);
          if (n < a.N && c < a.Cin) atomicAdd(&a.dw[((size_t)(ky * 3 + kx) * a.N + n) * a.Cin + c], acc[kx][i][j][r] * un);
        }
}

// wt[8-tap][c][n] = wf[tap][n][c]   (data-gradient weights: flipped taps, transposed)
__global__ void k_make_wt(const float* __restrict__ wf, float* __restrict__ wt, int N, int Cin) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t tot = (size_t)9 * N * Cin;
  if (idx >= tot) return;
  int c = (int)(idx % Cin); size_t t = idx / Cin; int n = (int)(t % N); int tap = (int)(t / N);
  wt[((size_t)(8 - tap) * Cin + c) * N + n] = wf[idx];
}

__global__ void k_pack_planes_t(const float* __restrict__ planes, float* __restrict__ out, TGeo g, int F, int Fp) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)g.M * Fp) return;
  int r = (int)(idx / Fp), c = (int)(idx - (size_t)r * Fp);
  int b = r / g.HW, p = r - b * g.HW;
  out[pix_off(g, r) * Fp + c] = c < F ? planes[((size_t)b * F + c) * g.HW + p] : 0.f;
}

// dst[r][:] = src[idx[r]][:] — batch assembly for agz_train_dev (rows stay where they are; the shuffle moves indices)
__global__ void k_gather_rows_t(const float* __restrict__ src, const int32_t* __restrict__ idx, float* __restrict__ dst, int row_len,
                                size_t total) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  size_t r = i / row_len;
  dst[i] = src[(size_t)idx[r] * row_len + (i - r * row_len)];
}

__global__ void k_axpy(float* __restrict__ p, const float* __restrict__ g, float alpha, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] += alpha * g[i];
}
// The solver form of the same sweep (agz_trainer_set_solver): solver_step over n4 float4 of p / g (/ v with MOM), g scaled by gs first
// (grad_scale of the two-pass and data-parallel paths).  Grid-stride, the grid sized by the CU count: it streams p, g, v -> p, v.
// SK_ADAM (agz_trainer_set_adam): adam_step over p / g / m / m2 (v is then the first moment, m2 the second); the two arguments it adds
// come last and the other kinds do not read them.
template <int KIND>
__global__ __launch_bounds__(256) void k_solver_sweep(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v, size_t n4,
                                                      float lr, float gs, float mu, float l2, float clip, float* __restrict__ m2, AdamK ak) {
  constexpr bool MOM = KIND == SK_MOMENTUM;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 w = reinterpret_cast<float4*>(p)[i];
    if (KIND == SK_ADAM) {
      float4 m = reinterpret_cast<float4*>(v)[i], u = reinterpret_cast<float4*>(m2)[i];
      adam_step(w.x, m.x, u.x, gs * gg.x, lr, l2, clip, ak);
      adam_step(w.y, m.y, u.y, gs * gg.y, lr, l2, clip, ak);
      adam_step(w.z, m.z, u.z, gs * gg.z, lr, l2, clip, ak);
      adam_step(w.w, m.w, u.w, gs * gg.w, lr, l2, clip, ak);
      reinterpret_cast<float4*>(v)[i] = m;
      reinterpret_cast<float4*>(m2)[i] = u;
      reinterpret_cast<float4*>(p)[i] = w;
      continue;
    }
    float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MOM) vv = reinterpret_cast<float4*>(v)[i];
    solver_step<MOM>(w.x, vv.x, gs * gg.x, lr, mu, l2, clip);
    solver_step<MOM>(w.y, vv.y, gs * gg.y, lr, mu, l2, clip);
    solver_step<MOM>(w.z, vv.z, gs * gg.z, lr, mu, l2, clip);
    solver_step<MOM>(w.w, vv.w, gs * gg.w, lr, mu, l2, clip);
    if (MOM) reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(p)[i] = w;
  }
}

// ---- heads (small; one thread per output element, plain loops) --------------------------------------------------
// zh[r][j] = sum_c x[pix(r)][c] * hc[j][c], j = 0,1 policy, 2 value
__global__ void k_head_conv(TGeo g, const float* __restrict__ x, const float* __restrict__ hc, float* __restrict__ zh, int Kp) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= g.M * 3) return;
  int r = idx / 3, j = idx - r * 3;
  const float* xp = x + pix_off(g, r) * Kp;
  float s = 0.f;
  for (int c = 0; c < Kp; c++) s += xp[c] * hc[j * Kp + c];
  zh[idx] = s;
}
// per-channel stats of zh [M][3]: one block per channel (the same summation order as the single-block form: 0.28 -> 0.09 ms at G19)
template <bool TRACK>
__global__ void k_head_stats(TGeo g, const float* __restrict__ zh, float eps, float* __restrict__ mean, float* __restrict__ inv, BnTrack tr) {
  __shared__ double red[256];
  {
    const int j = blockIdx.x;
    double s = 0;
    for (int r = threadIdx.x; r < g.M; r += 256) s += zh[r * 3 + j];
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    float mu = (float)(red[0] / g.M);
    if (TRACK) { if (threadIdx.x == 0) bn_track_mean(tr, j, red[0] / g.M); }
    __syncthreads();
    s = 0;
    for (int r = threadIdx.x; r < g.M; r += 256) { float d = zh[r * 3 + j] - mu; s += (double)d * d; }
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) { mean[j] = mu; inv[j] = 1.0f / sqrtf((float)(red[0] / g.M) + eps); }
    if (TRACK) { if (threadIdx.x == 0) bn_track_var(tr, j, red[0] / g.M); }
    __syncthreads();
  }
}
// yh[b][j][p] = relu(gamma*xhat+beta); head gamma/beta layout [B][3][HW]
template <bool TIED>
__global__ void k_head_apply(TGeo g, const float* __restrict__ zh, const float* __restrict__ hg, const float* __restrict__ hb,
                             const float* __restrict__ mean, const float* __restrict__ inv, float* __restrict__ yh) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= g.M * 3) return;
  int r = idx / 3, j = idx - r * 3;
  int b = r / g.HW, p = r - b * g.HW;
  float xh = (zh[idx] - mean[j]) * inv[j];
  size_t o = ((size_t)b * 3 + j) * g.HW + p;
  const size_t og = TIED ? (size_t)j * g.HW + p : o;   // (tied: head gamma / beta [3][HW], shared by every board)
  float y = hg[og] * xh + hb[og];
  yh[o] = y > 0.f ? y : 0.f;
}
struct HeadT {
  int B, HW, A, FC;
  int Bn;           // the batch the loss is normalised by: B, or the GLOBAL batch of a sharded trainer (B is the loop bound: this rank's rows)
  const float* yh;  // [B][3][HW]
  const float *Wp, *bp, *W1, *b1, *W2, *b2;
  const float *Pi, *V;
  float *logits, *hpre, *o;
  float *dWp, *dbp, *dW1, *db1, *dW2, *db2, *dyh;  // dyh [B][3][HW]
  float* cost;  // [2]: pcost, vcost sums
  // AGZ_LOSS_ALPHAZERO only (k_az_loss writes them, the <AZ = true> backward kernels read them; NULL otherwise)
  float *az_dz, *az_do;  // [B][A] d cost / d logits, [B] d cost / d o
  double* az_row;        // [B][2] the row's policy and value cost terms
};
// TIED: the biases are [A], [FC], [1], shared by every row
template <bool TIED>
__global__ void k_fc_fwd(HeadT h) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int nl = h.B * h.A, nh = h.B * h.FC;
  if (idx < nl) {
    int b = idx / h.A, j = idx - b * h.A;
    const float* yp = h.yh + (size_t)b * 3 * h.HW;  // policy features: channels 0,1 contiguous = flatten c-major
    float s = 0.f;
    for (int i = 0; i < 2 * h.HW; i++) s += yp[i] * h.Wp[(size_t)i * h.A + j];
    h.logits[idx] = s + h.bp[TIED ? j : idx];
  } else if (idx < nl + nh) {
    int k = idx - nl;
    int b = k / h.FC, j = k - b * h.FC;
    const float* yv = h.yh + ((size_t)b * 3 + 2) * h.HW;
    float s = 0.f;
    for (int i = 0; i < h.HW; i++) s += yv[i] * h.W1[(size_t)i * h.FC + j];
    h.hpre[k] = s + h.b1[TIED ? j : k];
  }
}
template <bool TIED>
__global__ void k_value_out(HeadT h) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= h.B) return;
  float s = 0.f;
  for (int j = 0; j < h.FC; j++) { float hv = h.hpre[(size_t)b * h.FC + j]; s += (hv > 0.f ? hv : 0.f) * h.W2[j]; }
  h.o[b] = s + h.b2[TIED ? 0 : b];
}
__global__ void k_cost(HeadT h) {  // single block
  __shared__ double red[256];
  double s = 0;
  for (int i = threadIdx.x; i < h.B * h.A; i += 256) s += -(double)(h.Pi[i] * h.logits[i] + (1.f - h.Pi[i]) * (1.f - h.logits[i]));
  red[threadIdx.x] = s; __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) h.cost[0] = (float)(red[0] / ((double)h.Bn * h.A));
  __syncthreads();
  s = 0;
  for (int b = threadIdx.x; b < h.B; b += 256) { double d = h.o[b] - h.V[b]; s += d * d; }
  red[threadIdx.x] = s; __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) h.cost[1] = (float)(red[0] / h.Bn);
}
// backward of the FC parts.  One thread per gradient element (sums over the batch inside).
// AZ (here and in the second form below): the per-(b, j) factor of the policy head and the per-b factor of the value head are read from
// k_az_loss's az_dz / az_do instead of being computed inline; <false> is the reference loss, the code as it always was.
template <bool AZ>
__global__ void k_fc_bwd(HeadT h) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const float sc = 1.0f / ((float)h.Bn * (float)h.A);
  int n_wp = 2 * h.HW * h.A, n_bp = h.B * h.A, n_w1 = h.HW * h.FC, n_b1 = h.B * h.FC, n_w2 = h.FC, n_b2 = h.B;
  int n_dy = h.B * 3 * h.HW;
  if (idx < n_wp) {  // dWp[i][j] = sum_b yp[b][i] * dl[b][j]
    int i = idx / h.A, j = idx - i * h.A;
    float s = 0.f;
    for (int b = 0; b < h.B; b++) s += h.yh[(size_t)b * 3 * h.HW + i] * (AZ ? h.az_dz[(size_t)b * h.A + j] : (1.f - 2.f * h.Pi[(size_t)b * h.A + j]) * sc);
    h.dWp[idx] = s;
    return;
  }
  idx -= n_wp;
  if (idx < n_bp) { h.dbp[idx] = AZ ? h.az_dz[idx] : (1.f - 2.f * h.Pi[idx]) * sc; return; }
  idx -= n_bp;
  if (idx < n_w1) {  // dW1[i][j] = sum_b yv[b][i] * dh[b][j]
    int i = idx / h.FC, j = idx - i * h.FC;
    float s = 0.f;
    for (int b = 0; b < h.B; b++) {
      float dob = AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn;
      float dh = h.hpre[(size_t)b * h.FC + j] > 0.f ? dob * h.W2[j] : 0.f;
      s += h.yh[((size_t)b * 3 + 2) * h.HW + i] * dh;
    }
    h.dW1[idx] = s;
    return;
  }
  idx -= n_w1;
  if (idx < n_b1) {
    int b = idx / h.FC, j = idx - b * h.FC;
    float dob = AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn;
    h.db1[idx] = h.hpre[idx] > 0.f ? dob * h.W2[j] : 0.f;
    return;
  }
  idx -= n_b1;
  if (idx < n_w2) {
    float s = 0.f;
    for (int b = 0; b < h.B; b++) { float hv = h.hpre[(size_t)b * h.FC + idx]; s += (AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn) * (hv > 0.f ? hv : 0.f); }
    h.dW2[idx] = s;
    return;
  }
  idx -= n_w2;
  if (idx < n_b2) { h.db2[idx] = AZ ? h.az_do[idx] : 2.f * (h.o[idx] - h.V[idx]) / (float)h.Bn; return; }
  idx -= n_b2;
  if (idx < n_dy) {  // d(yh)[b][j][p]
    int b = idx / (3 * h.HW), q = idx - b * 3 * h.HW;
    float s = 0.f;
    if (q < 2 * h.HW) {
      for (int j = 0; j < h.A; j++) s += (AZ ? h.az_dz[(size_t)b * h.A + j] : (1.f - 2.f * h.Pi[(size_t)b * h.A + j]) * sc) * h.Wp[(size_t)q * h.A + j];
    } else {
      int i = q - 2 * h.HW;
      float dob = AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn;
      for (int j = 0; j < h.FC; j++) if (h.hpre[(size_t)b * h.FC + j] > 0.f) s += dob * h.W2[j] * h.W1[(size_t)i * h.FC + j];
    }
    h.dyh[idx] = s;
  }
}
// head BN backward (3 channels, one block each): dzh[r][j], dgamma/dbeta [B][3][HW]
// TIED: hg is the shared [3][HW] tensor; dhg / dhb stay per board (a scratch of the untied shape, summed over the boards by k_rows_sum)
template <bool TIED>
__global__ void k_head_bn_bwd(TGeo g, const float* __restrict__ zh, const float* __restrict__ yh, const float* __restrict__ dyh,
                              const float* __restrict__ hg, const float* __restrict__ mean, const float* __restrict__ inv,
                              float* __restrict__ dhg, float* __restrict__ dhb, float* __restrict__ dzh) {
  __shared__ double r1[256], r2[256];
  {
    const int j = blockIdx.x;
    double a1 = 0, a2 = 0;
    for (int r = threadIdx.x; r < g.M; r += 256) {
      int b = r / g.HW, p = r - b * g.HW;
      size_t o = ((size_t)b * 3 + j) * g.HW + p;
      float gg = yh[o] > 0.f ? dyh[o] : 0.f;
      float xh = (zh[r * 3 + j] - mean[j]) * inv[j];
      dhg[o] = gg * xh; dhb[o] = gg;
      float dxh = gg * hg[TIED ? (size_t)j * g.HW + p : o];
      dzh[r * 3 + j] = dxh;
      a1 += dxh; a2 += (double)dxh * xh;
    }
    r1[threadIdx.x] = a1; r2[threadIdx.x] = a2; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; } __syncthreads(); }
    float s1 = (float)r1[0], s2 = (float)r2[0], m = (float)g.M; __syncthreads();
    for (int r = threadIdx.x; r < g.M; r += 256) {
      float xh = (zh[r * 3 + j] - mean[j]) * inv[j];
      dzh[r * 3 + j] = inv[j] * (dzh[r * 3 + j] - s1 / m - xh * (s2 / m));
    }
    __syncthreads();
  }
}
// head conv backward: dhc[j][c] = sum_r dzh[r][j]*x[pix(r)][c] ; dx[pix(r)][c] = sum_j dzh[r][j]*hc[j][c]
__global__ void k_head_conv_bwd_w(TGeo g, const float* __restrict__ x, const float* __restrict__ dzh, float* __restrict__ dhc, int Kp,
                                  int rows_per_block) {
  int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  for (int e = threadIdx.x; e < 3 * Kp; e += blockDim.x) {
    int j = e / Kp, c = e - j * Kp;
    float s = 0.f;
    for (int r = r0; r < r1; r++) s += dzh[r * 3 + j] * x[pix_off(g, r) * Kp + c];
    atomicAdd(&dhc[e], s);
  }
}
__global__ void k_head_conv_bwd_x(TGeo g, const float* __restrict__ dzh, const float* __restrict__ hc, float* __restrict__ dx, int Kp) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)g.M * Kp) return;
  int r = (int)(idx / Kp), c = (int)(idx - (size_t)r * Kp);
  dx[pix_off(g, r) * Kp + c] = dzh[r * 3] * hc[c] + dzh[r * 3 + 1] * hc[Kp + c] + dzh[r * 3 + 2] * hc[2 * Kp + c];
}


// ---- heads, second form (round 5): the same arithmetic with the memory behaviour fixed.  The nine kernels above cost 1.85 ms of a 47 ms
// G19 step, serially between the forward and the backward pass: three-block BatchNorm passes over 92 416 rows, a single-block cost sum,
// one thread per output walking strided operands.  Below: wave-per-row reductions, multi-block partial sums (double atomics), and FC
// kernels that load each weight once for eight batch rows (resp. eight weight rows) from LDS tiles.  Wherever an output is a sequential sum
// over i / b / j the ORDER is the old kernel's (bit-identical outputs: the FC forward, dWp, dW1, d(yh)); the BatchNorm sums, the head
// convolution and the cost are now tree / atomic sums (differences at 1e-7 of the value).
__global__ __launch_bounds__(256) void k_head_conv2(TGeo g, const float* __restrict__ x, const float* __restrict__ hc, float* __restrict__ zh, int Kp) {
  const int lane = threadIdx.x & 63, wv = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), nw = (int)(gridDim.x * 4u);
  for (int r = wv; r < g.M; r += nw) {
    const float* xp = x + pix_off(g, r) * Kp;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int c = lane * 4; c < Kp; c += 256) {
      const float4 v = *reinterpret_cast<const float4*>(xp + c);
      const float4 a = *reinterpret_cast<const float4*>(hc + c), b = *reinterpret_cast<const float4*>(hc + Kp + c), d = *reinterpret_cast<const float4*>(hc + 2 * Kp + c);
      s0 += v.x * a.x + v.y * a.y + v.z * a.z + v.w * a.w;
      s1 += v.x * b.x + v.y * b.y + v.z * b.z + v.w * b.w;
      s2 += v.x * d.x + v.y * d.y + v.z * d.z + v.w * d.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (lane == 0) { zh[(size_t)r * 3] = s0; zh[(size_t)r * 3 + 1] = s1; zh[(size_t)r * 3 + 2] = s2; }
  }
}
// sums [3] and sums of squares [3] of zh's channels -> hacc[0..5] (zeroed by the caller), then mean / inv
__global__ __launch_bounds__(256) void k_head_stats_part(TGeo g, const float* __restrict__ zh, double* __restrict__ hacc) {
  __shared__ double red[6][4];
  double s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
  for (int r = blockIdx.x * 256 + threadIdx.x; r < g.M; r += gridDim.x * 256) {
#pragma unroll
    for (int j = 0; j < 3; j++) { const double v = zh[(size_t)r * 3 + j]; s[j] += v; q[j] += v * v; }
  }
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s[j] += __shfl_xor(s[j], o, 64); q[j] += __shfl_xor(q[j], o, 64); }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { for (int j = 0; j < 3; j++) { red[j][w] = s[j]; red[3 + j][w] = q[j]; } }
  __syncthreads();
  if (threadIdx.x < 6) atomicAdd(&hacc[threadIdx.x], red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}
template <bool TRACK>
__global__ void k_head_stats_fin(TGeo g, const double* __restrict__ hacc, float eps, float* __restrict__ mean, float* __restrict__ inv, double m, BnTrack tr) {
  const int j = threadIdx.x;
  if (j >= 3) return;
  const double mu = hacc[j] / m;
  double var = hacc[3 + j] / m - mu * mu;
  if (var < 0) var = 0;
  mean[j] = (float)mu;
  inv[j] = 1.0f / sqrtf((float)var + eps);
  if (TRACK) { bn_track_mean(tr, j, mu); bn_track_var(tr, j, var); }
}
// out[b][j] = sum_i y[b][i] * Wt[i][j] + bias[b][j] for eight batch rows per block: grid (ceil(N / 256), ceil(B / 8), 2); z = 0: the policy
// logits (y = channels 0, 1 of yh flattened, K = 2 HW), z = 1: the value head's hidden layer (y = channel 2, K = HW)
template <bool TIED>
__global__ __launch_bounds__(256) void k_fc_fwd2(HeadT h) {
  extern __shared__ float ys[];                      // [8][K]
  const bool pol = blockIdx.z == 0;
  const int N = pol ? h.A : h.FC, K = pol ? 2 * h.HW : h.HW;
  const int j = blockIdx.x * 256 + threadIdx.x, b0 = blockIdx.y * 8;
  if (blockIdx.x * 256 >= N) return;
  const float* W = pol ? h.Wp : h.W1;
  for (int e = threadIdx.x; e < 8 * K; e += 256) {
    const int t = e / K, i = e - t * K, b = b0 + t;
    ys[e] = b < h.B ? h.yh[((size_t)b * 3 + (pol ? 0 : 2)) * h.HW + i] : 0.f;
  }
  __syncthreads();
  if (j >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < K; i++) {
    const float w = W[(size_t)i * N + j];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] += ys[t * K + i] * w;
  }
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int b = b0 + t;
    if (b >= h.B) break;
    const size_t o = (size_t)b * N + j, ob = TIED ? (size_t)j : o;
    if (pol) h.logits[o] = acc[t] + h.bp[ob]; else h.hpre[o] = acc[t] + h.b1[ob];
  }
}
template <bool TIED>
__global__ __launch_bounds__(64) void k_value_out2(HeadT h) {   // one wave per batch row
  const int b = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int j = lane; j < h.FC; j += 64) { const float hv = h.hpre[(size_t)b * h.FC + j]; s += (hv > 0.f ? hv : 0.f) * h.W2[j]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) h.o[b] = s + h.b2[TIED ? 0 : b];
}
// cost sums -> hacc[6] (policy), hacc[7] (value), zeroed by the caller; k_cost_fin writes cost[0..1]
__global__ __launch_bounds__(256) void k_cost_part(HeadT h, double* __restrict__ hacc) {
  __shared__ double red[2][4];
  double sp = 0, sv = 0;
  const int n = h.B * h.A;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) sp += -(double)(h.Pi[i] * h.logits[i] + (1.f - h.Pi[i]) * (1.f - h.logits[i]));
  for (int b = blockIdx.x * 256 + threadIdx.x; b < h.B; b += gridDim.x * 256) { const double d = h.o[b] - h.V[b]; sv += d * d; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sv += __shfl_xor(sv, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = sv; }
  __syncthreads();
  if (threadIdx.x < 2) atomicAdd(&hacc[6 + threadIdx.x], red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}
// AZ: hacc[6] holds k_az_cost_sum's sum of the rows' cross-entropies, a mean over the rows alone
template <bool AZ>
__global__ void k_cost_fin(HeadT h, const double* __restrict__ hacc) {
  if (threadIdx.x == 0) { h.cost[0] = (float)(hacc[6] / (AZ ? (double)h.Bn : (double)h.Bn * h.A)); h.cost[1] = (float)(hacc[7] / h.Bn); }
}
// ---- the AlphaZero loss (agz_trainer_set_loss(AGZ_LOSS_ALPHAZERO); the definition: agz.h): softmax cross-entropy of the logits against Pi
// and an MSE of tanh(o) against V.  One wave per batch row, after k_value_out*: A <= 512, so a lane holds at most eight logits (column
// lane + 64 k) and the row is read once.  The row maximum is taken off before the exponentials.  Writes dz [B][A], do [B] for the
// <AZ = true> backward kernels and the row's two cost terms; the policy term is summed as sum_j Pi_j (lse - z_j) = S lse - sum_j Pi_j z_j,
// whose terms are all >= 0 where Pi >= 0.
__global__ __launch_bounds__(64) void k_az_loss(HeadT h) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* __restrict__ zp = h.logits + (size_t)b * h.A;
  const float* __restrict__ pp = h.Pi + (size_t)b * h.A;
  float z[8], pi[8];
  float m = -INFINITY, S = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int j = lane + 64 * k;
    const bool in = j < h.A;
    z[k] = in ? zp[j] : -INFINITY; pi[k] = in ? pp[j] : 0.f;
    m = fmaxf(m, z[k]); S += pi[k];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); S += __shfl_xor(S, o, 64); }
  float e[8], se = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) { e[k] = expf(z[k] - m); se += e[k]; }   // (columns past A: exp(-inf) = 0)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  const float lse = m + logf(se), inv = 1.0f / se, bn = (float)h.Bn;
  float pc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int j = lane + 64 * k;
    if (j < h.A) {
      h.az_dz[(size_t)b * h.A + j] = (S * (e[k] * inv) - pi[k]) / bn;
      pc += pi[k] * (lse - z[k]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o, 64);
  if (lane == 0) {
    const float t = tanhf(h.o[b]), d = t - h.V[b];
    h.az_do[b] = 2.f * d * (1.f - t * t) / bn;
    h.az_row[2 * b] = (double)pc;
    h.az_row[2 * b + 1] = (double)d * d;
  }
}
// the rows' cost terms summed in double in ONE fixed order (a lane's rows b = lane, lane + 64, ..., then the wave tree): no atomics, so the
// cost reproduces to the bit.  hacc != NULL (second form of the heads): the sums -> hacc[6], hacc[7], where the sharded exchange and
// k_cost_fin<true> expect them; hacc == NULL (first form): cost[0..1] directly.
__global__ __launch_bounds__(64) void k_az_cost_sum(HeadT h, double* __restrict__ hacc) {
  double sp = 0, sv = 0;
  for (int b = threadIdx.x; b < h.B; b += 64) { sp += h.az_row[2 * b]; sv += h.az_row[2 * b + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sv += __shfl_xor(sv, o, 64); }
  if (threadIdx.x == 0) {
    if (hacc) { hacc[6] = sp; hacc[7] = sv; }
    else { h.cost[0] = (float)(sp / h.Bn); h.cost[1] = (float)(sv / h.Bn); }
  }
}
// dW[i][j] = sum_b y[b][i] * d[b][j], eight rows i per block: grid (ceil(N / 256), ceil(K / 8), 2); z = 0: dWp (d = the xent gradient),
// z = 1: dW1 (d = the value head's hidden-layer gradient).  The b loop is the old kernel's.
template <bool AZ>
__global__ __launch_bounds__(256) void k_fc_bwd_w(HeadT h) {
  extern __shared__ float ys[];                      // [B][8]
  const bool pol = blockIdx.z == 0;
  const int N = pol ? h.A : h.FC, K = pol ? 2 * h.HW : h.HW;
  const int j = blockIdx.x * 256 + threadIdx.x, i0 = blockIdx.y * 8;
  if (blockIdx.x * 256 >= N || i0 >= K) return;
  for (int e = threadIdx.x; e < h.B * 8; e += 256) {
    const int b = e >> 3, t = e & 7, i = i0 + t;
    ys[e] = i < K ? h.yh[((size_t)b * 3 + (pol ? 0 : 2)) * h.HW + i] : 0.f;
  }
  __syncthreads();
  if (j >= N) return;
  const float sc = 1.0f / ((float)h.Bn * (float)h.A);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < h.B; b++) {
    float d;
    if (pol) d = AZ ? h.az_dz[(size_t)b * h.A + j] : (1.f - 2.f * h.Pi[(size_t)b * h.A + j]) * sc;
    else { const float dob = AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn; d = h.hpre[(size_t)b * h.FC + j] > 0.f ? dob * h.W2[j] : 0.f; }
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] += ys[b * 8 + t] * d;
  }
  float* dW = pol ? h.dWp : h.dW1;
#pragma unroll
  for (int t = 0; t < 8; t++) if (i0 + t < K) dW[(size_t)(i0 + t) * N + j] = acc[t];
}
// the elementwise / small parts of the FC backward: dbp, db1, dW2, db2
template <bool AZ>
__global__ void k_fc_bwd_small(HeadT h) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const float sc = 1.0f / ((float)h.Bn * (float)h.A);
  const int n_bp = h.B * h.A, n_b1 = h.B * h.FC, n_w2 = h.FC, n_b2 = h.B;
  if (idx < n_bp) { h.dbp[idx] = AZ ? h.az_dz[idx] : (1.f - 2.f * h.Pi[idx]) * sc; return; }
  idx -= n_bp;
  if (idx < n_b1) {
    const int b = idx / h.FC, j = idx - b * h.FC;
    const float dob = AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn;
    h.db1[idx] = h.hpre[idx] > 0.f ? dob * h.W2[j] : 0.f;
    return;
  }
  idx -= n_b1;
  if (idx < n_w2) {
    float s = 0.f;
    for (int b = 0; b < h.B; b++) { const float hv = h.hpre[(size_t)b * h.FC + idx]; s += (AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn) * (hv > 0.f ? hv : 0.f); }
    h.dW2[idx] = s;
    return;
  }
  idx -= n_w2;
  if (idx < n_b2) h.db2[idx] = AZ ? h.az_do[idx] : 2.f * (h.o[idx] - h.V[idx]) / (float)h.Bn;
}
// d(yh)[b][q] for eight batch rows per block: grid (ceil(Q / 256), ceil(B / 8), 2); z = 0: q < 2 HW (sum over the A logits), z = 1: the value
// channel (sum over the FC hidden units).  The j loop is the old kernel's; the per-(b, j) factor comes from an LDS tile.
template <bool AZ>
__global__ __launch_bounds__(256) void k_fc_bwd_y(HeadT h) {
  extern __shared__ float ds[];                      // [8][J]
  const bool pol = blockIdx.z == 0;
  const int J = pol ? h.A : h.FC, Q = pol ? 2 * h.HW : h.HW;
  const int q = blockIdx.x * 256 + threadIdx.x, b0 = blockIdx.y * 8;
  if (blockIdx.x * 256 >= Q) return;
  const float sc = 1.0f / ((float)h.Bn * (float)h.A);
  for (int e = threadIdx.x; e < 8 * J; e += 256) {
    const int t = e / J, j = e - t * J, b = b0 + t;
    float d = 0.f;
    if (b < h.B) {
      if (pol) d = AZ ? h.az_dz[(size_t)b * h.A + j] : (1.f - 2.f * h.Pi[(size_t)b * h.A + j]) * sc;
      else { const float dob = AZ ? h.az_do[b] : 2.f * (h.o[b] - h.V[b]) / (float)h.Bn; d = h.hpre[(size_t)b * h.FC + j] > 0.f ? dob * h.W2[j] : 0.f; }
    }
    ds[e] = d;
  }
  __syncthreads();
  if (q >= Q) return;
  const float* Wr = (pol ? h.Wp : h.W1) + (size_t)q * J;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < J; j++) {
    const float w = Wr[j];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] += ds[t * J + j] * w;
  }
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int b = b0 + t;
    if (b < h.B) h.dyh[(size_t)b * 3 * h.HW + (pol ? 0 : 2 * h.HW) + q] = acc[t];
  }
}
// head BatchNorm backward in two passes over all rows: (1) dgamma / dbeta, dxh -> dzh, the two channel sums -> hacc[8..13] (zeroed by the
// caller); (2) dzh = inv * (dxh - s1 / m - xh * s2 / m)
template <bool TIED>
__global__ __launch_bounds__(256) void k_head_bn_bwd_a(TGeo g, const float* __restrict__ zh, const float* __restrict__ yh, const float* __restrict__ dyh,
                                                       const float* __restrict__ hg, const float* __restrict__ mean, const float* __restrict__ inv,
                                                       float* __restrict__ dhg, float* __restrict__ dhb, float* __restrict__ dzh, double* __restrict__ hacc) {
  __shared__ double red[6][4];
  double a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0};
  for (int r = blockIdx.x * 256 + threadIdx.x; r < g.M; r += gridDim.x * 256) {
    const int b = r / g.HW, p = r - b * g.HW;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const size_t o = ((size_t)b * 3 + j) * g.HW + p;
      const float gg = yh[o] > 0.f ? dyh[o] : 0.f;
      const float xh = (zh[(size_t)r * 3 + j] - mean[j]) * inv[j];
      dhg[o] = gg * xh; dhb[o] = gg;
      const float dxh = gg * hg[TIED ? (size_t)j * g.HW + p : o];
      dzh[(size_t)r * 3 + j] = dxh;
      a1[j] += dxh; a2[j] += (double)dxh * xh;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a1[j] += __shfl_xor(a1[j], o, 64); a2[j] += __shfl_xor(a2[j], o, 64); }
  if ((threadIdx.x & 63) == 0) { for (int j = 0; j < 3; j++) { red[j][threadIdx.x >> 6] = a1[j]; red[3 + j][threadIdx.x >> 6] = a2[j]; } }
  __syncthreads();
  if (threadIdx.x < 6) atomicAdd(&hacc[8 + threadIdx.x], red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}
__global__ __launch_bounds__(256) void k_head_bn_bwd_b(TGeo g, const float* __restrict__ zh, const float* __restrict__ mean, const float* __restrict__ inv,
                                                       float* __restrict__ dzh, const double* __restrict__ hacc, float m) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)g.M * 3) return;
  const int j = (int)(idx % 3);
  const float s1 = (float)hacc[8 + j], s2 = (float)hacc[11 + j];
  const float xh = (zh[idx] - mean[j]) * inv[j];
  dzh[idx] = inv[j] * (dzh[idx] - s1 / m - xh * (s2 / m));
}
// dhc[j][c] += sum over the block's rows: one thread per channel, the three j at once (x read once), four rows in flight
__global__ __launch_bounds__(256) void k_head_conv_bwd_w2(TGeo g, const float* __restrict__ x, const float* __restrict__ dzh, float* __restrict__ dhc, int Kp,
                                                          int rows_per_block) {
  const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, g.M);
  for (int c = threadIdx.x; c < Kp; c += 256) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int r = r0; r < r1; r++) {
      const float xv = x[pix_off(g, r) * Kp + c];
      s0 += dzh[(size_t)r * 3] * xv; s1 += dzh[(size_t)r * 3 + 1] * xv; s2 += dzh[(size_t)r * 3 + 2] * xv;
    }
    atomicAdd(&dhc[c], s0); atomicAdd(&dhc[Kp + c], s1); atomicAdd(&dhc[2 * Kp + c], s2);
  }
}
__global__ __launch_bounds__(256) void k_head_conv_bwd_x2(TGeo g, const float* __restrict__ dzh, const float* __restrict__ hc, float* __restrict__ dx, int Kp) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;   // one float4 of one row
  const int k4 = Kp >> 2;
  if (idx >= (size_t)g.M * k4) return;
  const int r = (int)(idx / k4), c = (int)(idx - (size_t)r * k4) * 4;
  const float d0 = dzh[(size_t)r * 3], d1 = dzh[(size_t)r * 3 + 1], d2 = dzh[(size_t)r * 3 + 2];
  const float4 a = *reinterpret_cast<const float4*>(hc + c), b = *reinterpret_cast<const float4*>(hc + Kp + c), e = *reinterpret_cast<const float4*>(hc + 2 * Kp + c);
  float4 o;
  o.x = d0 * a.x + d1 * b.x + d2 * e.x; o.y = d0 * a.y + d1 * b.y + d2 * e.y; o.z = d0 * a.z + d1 * b.z + d2 * e.z; o.w = d0 * a.w + d1 * b.w + d2 * e.w;
  *reinterpret_cast<float4*>(dx + pix_off(g, r) * Kp + c) = o;
}

}  // namespace agz

using namespace agz;

// ---- forward convolution of a dual block with BOTH operands DMA'd into LDS (AGZ_COMPUTE_WINO_H2, round 5) -------------------------------
// conv_h2.hpp's conv3x3_h2w_kernel splits its fp32 activations while staging them: every element is scaled, split and written to LDS once
// per tap and column tile (18 times per layer), and that VALU + ds_write issue — not operand bytes — bounds it (0.67 ms per G19 layer; the
// same kernel on 256-row tiles, with half the weight re-reads, ran 0.665).  Measured here: 0.583 ms per G19 layer.  The layer input is
// split ONCE into hi / lo fp16 planes
// (k_split_h2p, the tensor's own power-of-two range from the BatchNorm pass that wrote it) — the very planes the weight gradient of the
// same layer reads in the backward pass, which therefore no longer splits x itself — and the convolution is a pure DMA GEMM like
// wino_gemm_h2g_kernel: 128 x 256 tile, K step = 32 channels of one tap, `buffer_load ... lds` of 16 bytes per lane for both operands
// (A rows gathered by padded pixel: one lane offset per 16-row instruction, the tap and the channel chunk in the scalar offset), single
// 48 KB stage, plain __syncthreads(), three workgroups per CU (two, without the 3 spilled registers: 0.596 against 0.583 ms).  LDS image:
// four pieces (A hi, A lo, B hi, B lo) of 64-byte rows, 16-byte
// units XOR-swizzled with (row >> 2) & 3 — on the SOURCE address, the DMA writes lane-linearly.  Products as everywhere: lo*hi, hi*lo, hi*hi.
// (conv_h2.hpp's scale rule for the weight image: s = 2^(13 - floor(log2(amax))), exact inverse)
__device__ __forceinline__ void h2_scales(unsigned amax_bits, float* s, float* inv) {
  int e = (int)((amax_bits >> 23) & 0xffu);
  if (amax_bits == 0u) { *s = 1.f; *inv = 1.f; return; }
  e = e < 30 ? 30 : (e > 230 ? 230 : e);
  *s = __uint_as_float((unsigned)(267 - e) << 23);
  *inv = __uint_as_float((unsigned)(e - 13) << 23);
}
struct ConvDmaArgs {
  const _Float16 *xh, *xl;   // [B][Hp][Wp][Cin] hi / lo planes of the layer input (zero halo)
  const _Float16* w2;        // [Cin/32][tap][piece][Ntot][32]
  float* y;                  // [B][Hp][Wp][Ntot] raw GEMM result (halo untouched)
  const unsigned* x_amax;    // bits of max|x| (the planes' scale: wg_h2_scale)
  const unsigned* w_amax;    // bits of max|w| (the weight image's scale: h2_scales of conv_h2.hpp)
  TGeo g;
  int Cin, Ntot, n_mtiles, n_ntiles;
};
__device__ __forceinline__ unsigned cd_lds_off(int row, int unit) { return cmaps::lds_off(row, unit); }   // (conv_maps.hpp: shared with the CPU check)
__global__ __launch_bounds__(256, 3) void k_conv_h2dma(ConvDmaArgs a) {
  constexpr int PA = 128 * 64, PB = 256 * 64;          // bytes of one A / B piece image
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * PA + 2 * PB];   // 48 KB

  const int nblk = a.n_mtiles * a.n_ntiles;
  const int id = blockIdx.x;
  int q = nblk >> 3, rr = nblk & 7, xcd = id & 7, slot = id >> 3;
  int tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + slot;
  const int m_tile = tile / a.n_ntiles, n_tile = tile - m_tile * a.n_ntiles;
  const int m0 = m_tile * 128, n0 = n_tile * 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;

  const size_t plane_bytes = (size_t)a.g.B * a.g.Hp * a.g.Wp * a.Cin * 2;
  const __amdgpu_buffer_rsrc_t rxh = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.xh), 0, (int)plane_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rxl = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.xl), 0, (int)plane_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.w2), 0, 0x7fffffff, 0x00020000);

  // DMA lane mapping: an instruction lands 16 rows x 64 bytes; lane l -> row 16 j + (l >> 2), LDS unit l & 3, source unit (l & 3) ^ ((l >> 4) & 3)
  const unsigned src_unit = (unsigned)((lane & 3) ^ ((lane >> 4) & 3)) << 4;
  unsigned voa[2];                                       // A: rows 32 wid + 16 j + (lane >> 2) -> padded pixel, shifted by -(Wp + 1) (the taps add 0 .. 2 Wp + 2)
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int m = m0 + 32 * wid + 16 * j + (lane >> 2);
    if (m >= a.g.M) m = a.g.M - 1;
    voa[j] = (unsigned)((pix_off(a.g, m) - (size_t)(a.g.Wp + 1)) * (size_t)a.Cin * 2) + src_unit;
  }
  int nrow = n0 + 64 * wid + (lane >> 2);                // B: rows 64 wid + 16 j + (lane >> 2): + j KB in the scalar offset
  const unsigned vob = (unsigned)(nrow < a.Ntot ? nrow : a.Ntot - 1) * 64u + src_unit;
  const unsigned piece_bytes = (unsigned)a.Ntot * 64u;
  unsigned char* const la = lds + wid * 2048;            // this wave's 32 rows of an A piece
  unsigned char* const lb = lds + 2 * PA + wid * 4096;   // this wave's 64 rows of a B piece

  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  int ra[2], rb[4];
#pragma unroll
  for (int i = 0; i < 2; i++) ra[i] = (wm * 2 + i) * 32 + (lane & 31);
  // columns of this wave inside the 256-column tile: j = 0..3 -> 32-column groups of its 128 columns (the weight image's own order)
#pragma unroll
  for (int j = 0; j < 4; j++) rb[j] = wn * 128 + j * 32 + (lane & 31);
  const int kh = lane >> 5;

  const int NC = a.Cin >> 5;
  unsigned wso = 0;                                      // weight image: K steps in [chunk][tap] order, 2 pieces each
#pragma nounroll
  for (int cc = 0; cc < NC; cc++) {
#pragma nounroll
    for (int tap = 0; tap < 9; tap++) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const unsigned aso = (unsigned)((ky * a.g.Wp + kx) * a.Cin * 2 + cc * 64);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rxh, (wg_lds_ptr_t)(la + j * 1024), 16, voa[j], aso, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rxl, (wg_lds_ptr_t)(la + PA + j * 1024), 16, voa[j], aso, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (wg_lds_ptr_t)(lb + j * 1024), 16, vob, wso + (unsigned)j * 1024u, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (wg_lds_ptr_t)(lb + PB + j * 1024), 16, vob, wso + piece_bytes + (unsigned)j * 1024u, 0, 0);
      }
      wso += 2u * piece_bytes;
      __syncthreads();                                   // (its fence waits vmcnt(0): this wave's DMA has landed; then every wave's)
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
        wg_f16x8_t A_[2][2];
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
          for (int i = 0; i < 2; i++) A_[i][p] = *reinterpret_cast<const wg_f16x8_t*>(lds + p * PA + cd_lds_off(ra[i], 2 * ks + kh));
#pragma unroll
        for (int j = 0; j < 4; j++) {                    // B fragments just in time
          const wg_f16x8_t b0 = *reinterpret_cast<const wg_f16x8_t*>(lds + 2 * PA + cd_lds_off(rb[j], 2 * ks + kh));
          const wg_f16x8_t b1 = *reinterpret_cast<const wg_f16x8_t*>(lds + 2 * PA + PB + cd_lds_off(rb[j], 2 * ks + kh));
#pragma unroll
          for (int i = 0; i < 2; i++) {                  // small terms first: lo*hi, hi*lo, hi*hi
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A_[i][1], b0, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A_[i][0], b1, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A_[i][0], b0, acc[i][j], 0, 0, 0);
          }
        }
      }
      __syncthreads();                                   // every wave has read the stage before the next DMA overwrites it
    }
  }
  // raw result, un-scaled by the two exact powers of two
  float sw_, unw_;
  h2_scales(*a.w_amax, &sw_, &unw_);
  const float un = unw_ / wg_h2_scale(*a.x_amax);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m >= a.g.M) continue;
      float* yr = a.y + pix_off(a.g, m) * (size_t)a.Ntot;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int c = n0 + rb[j];
        if (c < a.Ntot) yr[c] = acc[i][j][r] * un;
      }
    }
}

// ---- the same convolution, nine taps from ONE x image (round 5, second form) ---------------------------------------------------------------
// k_conv_h2dma above streams 48 KB through L2 -> LDS per K step of 6.3 MFLOP: 5 GB per G19 layer, which at the ~10 TB/s the L2 delivers to
// the CUs is the whole 0.56 ms (46 % of the fp16x2 MFMA roof).  Here a workgroup computes 256 output pixels x 128 output channels and
// lands, per 32-channel chunk, ONE image of its input: the padded pixels from (first output pixel) - Wp - 1 to (last output pixel) + Wp + 1,
// hi and lo plane — tap (ky, kx) of output pixel m reads image row ra(m) + ky Wp + kx, ra(m) = padded distance of m from the tile's first
// pixel (row ends and one board crossing included: <= 372 rows for 19x19) — 47 KB for nine taps; the weights stream per tap (16 KB,
// double-buffered, landing under the tap before).  21 KB per K step instead of 48.  Same products in the same order per accumulator
// (chunks ascending, taps ascending, lo*hi, hi*lo, hi*hi): results are k_conv_h2dma's bit for bit.  80 KB of LDS: two workgroups per CU;
// assembly DMA + counted waits as in k_wgrad_h2t3 (the compiler's own LDS-DMA bookkeeping would drain the weight prefetch before every tap).
// Measured: G19 step 43.1 -> 42.2 ms (forward_backward, same box; 0.565 -> ~0.52 ms per layer), far from the 2.3x fewer bytes.  Decomposition
// (MODE, scripts/train_bench.py --fb --hooks 1,65,129,193; ms per step): everything 42.2, no x image after chunk 0 41.9, no weight DMA
// 37.5, neither 36.9 — the arithmetic alone runs AT the MFMA rate (0.255 ms per layer), the image costs 17 us per layer, the weights' 16 KB
// per tap 235 us.  That cost did not move with: no look-ahead at all (+0.2 ms per step); no wait for the weights (-2.3 of the 4.7 ms, wrong
// results); an XCD per n-tile (its quarter of the weights resident in its L2); every K step landing the SAME lines; a different chunk
// order per m-tile; nor with the weights loaded straight into registers one tap ahead (lane = output channel, no LDS, no barrier inside a
// chunk: 42.1 ms, and 45.8 on every other run).  Vector-memory traffic beside 48 MFMAs + 24 fragment reads per tap slows the tap whatever
// its source, latency and path; what remains is fewer weight bytes per product (a 256 x 256 tile: one workgroup per CU, another kernel).
constexpr int CD3_IMG = cmaps::CD3_IMG;
template <int MODE>   // (decomposition runs only — WRONG results: bit 0 = the x image lands for chunk 0 only, bit 1 = no weight DMA after K step 0)
__global__ __launch_bounds__(256, 2) void k_conv_h2dma3(ConvDmaArgs a) {
  constexpr int PA = CD3_IMG * 64;          // bytes of one piece (hi or lo) of the x image
  constexpr int PB = 128 * 64, SB = 2 * PB;  // one piece of a tap's weights; a weight stage (hi, lo)
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * PA + 2 * SB];   // 47 616 + 32 768 bytes

  const int nblk = a.n_mtiles * a.n_ntiles;
  const int id = blockIdx.x;
  int q = nblk >> 3, rr = nblk & 7, xcd = id & 7, slot = id >> 3;
  int tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + slot;
  const int m_tile = tile / a.n_ntiles, n_tile = tile - m_tile * a.n_ntiles;   // (the n-tiles of an m-tile are neighbours on one XCD: one x image in its L2)
  const int m0 = m_tile * 256, n0 = n_tile * 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;

  const size_t plane_bytes = (size_t)a.g.B * a.g.Hp * a.g.Wp * a.Cin * 2;
  auto mk = [](const void* p, size_t bytes) -> wg_rsrc_t {
    const unsigned long long u = (unsigned long long)p;
    wg_rsrc_t r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)u); r[1] = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane((unsigned)bytes); r[3] = 0x00020000u;
    return r;
  };
  const wg_rsrc_t rxh = mk(a.xh, plane_bytes), rxl = mk(a.xl, plane_bytes);
  const wg_rsrc_t rw = mk(a.w2, (size_t)(a.Cin >> 5) * 9 * 2 * a.Ntot * 64);
  const unsigned lds0 = (unsigned)(size_t)(wg_lds_ptr_t)lds;

  // DMA lane mapping (both operands): an instruction lands 16 rows x 64 bytes lane-linearly; lane l -> row 16 j + (l >> 2), LDS unit l & 3,
  // SOURCE unit (l & 3) ^ ((l >> 4) & 3) (the read side's swizzle, cd_lds_off)
  const unsigned src_unit = cmaps::dma_src_unit(lane);
  const size_t pix0 = pix_off(a.g, m0);
  const int pb = cmaps::cd3_base(pix0, a.g.Wp);                             // padded pixel of image row 0 (>= 0)
  const unsigned va0 = (unsigned)(pb + cmaps::dma_row(lane, 0)) * (unsigned)(a.Cin * 2) + src_unit;
  const unsigned vb0 = (unsigned)(n0 + 32 * wid + cmaps::dma_row(lane, 0)) * 64u + src_unit;
  const unsigned piece_bytes = (unsigned)a.Ntot * 64u;
  auto issue_A = [&](int cc) {                       // instructions j = wid, wid + 4, .. < 24; rows >= CD3_IMG stay unwritten (lanes off)
#pragma unroll
    for (int jj = 0; jj < 6; jj++) {
      const int j = wid + 4 * jj;
      if (cmaps::dma_row(lane, j) < CD3_IMG) {
        const unsigned vo = va0 + (unsigned)j * (unsigned)(16 * a.Cin * 2) + (unsigned)cc * 64u;
        wg_dma16(rxh, lds0 + cmaps::dma_dst(0, j), vo);
        wg_dma16(rxl, lds0 + (unsigned)PA + cmaps::dma_dst(0, j), vo);
      }
    }
  };
  auto issue_B = [&](int kstep, int buf) {           // K step = chunk * 9 + tap: the weight image's own order, two pieces each
    const unsigned so = (unsigned)kstep * 2u * piece_bytes;
    const unsigned d = lds0 + 2u * PA + (unsigned)buf * SB + (unsigned)wid * 2048u;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      wg_dma16(rw, d + cmaps::dma_dst(0, j), vb0 + so + (unsigned)j * 1024u);
      wg_dma16(rw, d + PB + cmaps::dma_dst(0, j), vb0 + so + piece_bytes + (unsigned)j * 1024u);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  int ra[4];                                           // image row of this lane's output pixel under tap (0, 0)
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int m = m0 + (wm * 4 + i) * 32 + (lane & 31);
    if (m >= a.g.M) m = a.g.M - 1;
    ra[i] = cmaps::cd3_row0(pix_off(a.g, m), pix0);
  }
  const int kh = lane >> 5;
  unsigned ob[2][2];                                   // weight fragment offsets inside a stage piece
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) ob[j][ks] = cd_lds_off(wn * 64 + j * 32 + (lane & 31), 2 * ks + kh);

  const int NC = a.Cin >> 5, NS = NC * 9;
  issue_B(0, 0);
  int t = 0;
#pragma nounroll
  for (int cc = 0; cc < NC; cc++) {
    if (cc > 0) __builtin_amdgcn_s_barrier();          // every wave is done with the image of chunk cc - 1
    if (!(MODE & 1) || cc == 0) issue_A(cc);
#pragma nounroll
    for (int tap = 0; tap < 9; tap++) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of the tap's weights (and, at tap 0, of the image) has landed
      __builtin_amdgcn_s_barrier();                      // ... every wave's; and every wave is done with the tap before
      __builtin_amdgcn_sched_barrier(0);
      if (!(MODE & 2) && t + 1 < NS) issue_B(t + 1, (t + 1) & 1);
      const unsigned char* bs = lds + 2 * PA + (t & 1) * SB;
      const int ky = (tap * 11) >> 5;                    // tap / 3 for tap < 9
      const int toff = cmaps::cd3_tap(ky, tap - 3 * ky, a.g.Wp);
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
        wg_f16x8_t B_[2][2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          B_[j][0] = *reinterpret_cast<const wg_f16x8_t*>(bs + ob[j][ks]);
          B_[j][1] = *reinterpret_cast<const wg_f16x8_t*>(bs + PB + ob[j][ks]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int row = ra[i] + toff;
          const unsigned o = cmaps::lds_off(row, 2 * ks + kh);
          const wg_f16x8_t ah = *reinterpret_cast<const wg_f16x8_t*>(lds + o);
          const wg_f16x8_t al = *reinterpret_cast<const wg_f16x8_t*>(lds + PA + o);
#pragma unroll
          for (int j = 0; j < 2; j++) {                  // small terms first: lo*hi, hi*lo, hi*hi
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, B_[j][0], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, B_[j][1], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, B_[j][0], acc[i][j], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      t++;
    }
  }
  // raw result, un-scaled by the two exact powers of two
  float sw_, unw_;
  h2_scales(*a.w_amax, &sw_, &unw_);
  const float un = unw_ / wg_h2_scale(*a.x_amax);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + (wm * 4 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m >= a.g.M) continue;
      float* yr = a.y + pix_off(a.g, m) * (size_t)a.Ntot + n0 + wn * 64 + (lane & 31);
#pragma unroll
      for (int j = 0; j < 2; j++) yr[j * 32] = acc[i][j][r] * un;
    }
}

struct TLayer {
  int Cin_p, Cout_p, nbr;
  size_t o_wf, o_gamma, o_beta;   // offsets in the flat P / G buffers
  float *wt = nullptr, *z = nullptr, *out = nullptr, *mean = nullptr, *inv = nullptr;
  unsigned short *w3f = nullptr, *w3t = nullptr;   // bf16x3 images of the forward / transposed filter (AGZ_COMPUTE_BF16X3)
  _Float16* xh2 = nullptr;                         // AGZ_COMPUTE_WINO_H2: hi plane then lo plane of the layer INPUT (forward DMA convolution + weight gradient)
  bool x_planes = false;                           // ... and they hold this step's input (set by the forward pass, read by the backward pass)
  // weight images of the step, built on the side stream beside the forward pass (prep_weights): fw = fp16x2 image of the filter for the DMA
  // forward convolution, bw = Winograd image of the transposed filter for the data gradient
  agz::RawWeights fw, bw;
  hipEvent_t ev_fw = nullptr;
  bool fw_ready = false, bw_ready = false;         // ... built for THIS step
  // agz_trainer_last_paths (agz_debug.h): the kernels the last step launched for this layer, written at the launching branches (AGZ_PATH_*)
  int path_fwd = 0, path_wgrad = 0, path_dgrad = 0, path_bn2 = 0;
  // agz_trainer_last_rows (agz_debug.h): the row plan of the last step's batch-sized loops for this layer (AGZ_ROWS_*), copied from the
  // very values the launchers pass to the kernels
  int rows[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
struct TParamRef { std::string name; int kind; std::vector<int> shape; int layer; int sub; };  // sub: 0 filter(a) 1 gamma 2 beta, for dual +10 = branch b

struct agz_trainer {
  agz_ctx* ctx = nullptr;
  agz_net_conf conf{};
  TGeo g{};
  int K, Kp, Fp = 32, L, A, FC, B, F;
  std::vector<TLayer> layers;          // 0 = init, 1..L = blocks
  std::vector<TParamRef> prefs;        // reference Model() order
  size_t n_flat = 0;
  float *P = nullptr, *G = nullptr;    // flat learnables / gradients
  // head offsets in flat
  size_t o_hc, o_hg, o_hb, o_Wp, o_bp, o_W1, o_b1, o_W2, o_b2;
  // work buffers
  float *x0 = nullptr, *dA = nullptr, *dB = nullptr, *dz = nullptr, *dz0 = nullptr;
  double* acc = nullptr;               // [2][1024] channel sums
  float *zh = nullptr, *yh = nullptr, *dyh = nullptr, *dzh = nullptr, *hmean = nullptr, *hinv = nullptr;
  float *logits = nullptr, *hpre = nullptr, *o = nullptr, *cost = nullptr;
  float *d_planes = nullptr, *d_pi = nullptr, *d_v = nullptr;
  bool x3 = false, x3_force = false;   // agz_trainer_set_compute_mode (FORCE: also below the chip-filling threshold, tests)
  // AGZ_COMPUTE_WINO_H2: the DATA-GRADIENT convolutions of the dual blocks through conv_wino_h2.hpp; the forward convolutions are DIRECT
  // fp16x2 convolutions (use_h2_fwd / dma_layer below).  (Round 2 also ran the forward convolutions through the Winograd path: 72 instead
  // of 87 ms per G19 step, but its rounding — 2e-6 of the output rms against 2e-7 — flips a ReLU unit against the reference arithmetic on
  // every other data draw at K = 256 / 19x19, which moves that unit's gradients by percent: outside the stated tolerance, removed.)
  bool wino = false;
  WinoRawScratch wsc;
  // ... and the weight gradient with fp16x2 products: both operands split once per layer (k_wgrad_h2)
  unsigned *dz_h2 = nullptr, *x_h2 = nullptr;
  // per-layer scratch cleared ONCE per step (one memset each instead of one per layer): the backward BatchNorm channel sums
  // [L + 1][2][1024] and the fp16x2 weight gradient's range words [L + 2][2] = {max|dz| of layer l, max|x| of its input}
  double* acc_b = nullptr;
  unsigned* amax_words = nullptr;
  unsigned* board_words = nullptr;     // [2][L + 2][B] per-board ranges: [0] layer inputs (from k_bn_apply_v), [1] dz (from k_bn_bwd2_v)
  std::vector<char> x_amax_ready;      // layer l's input range was produced by the forward pass (k_bn_apply_v)
  std::vector<char> xb_ready;          // ... and its per-board ranges (board_words)
  size_t* zero_tab = nullptr;          // [2][L + 1] offsets and counts of the filter-gradient regions (k_zero_regions)
  // the weight gradient of a layer (matrix pipe / L2 bound, ~0.35 GB of HBM traffic) runs on its own stream beside the same layer's data
  // gradient and the next layer's BatchNorm backward (HBM bound): both only need dz.  Measured 50.6-50.9 -> 49.1-50.0 ms per G19 step —
  // the weight gradient's two workgroups per CU hold 496 of a SIMD's 512 registers, so little else becomes resident beside them (forcing
  // ONE workgroup per CU to make room: 49.4-50.4, no better)
  hipStream_t wg_stream = nullptr;
  hipEvent_t ev_dz = nullptr, ev_split = nullptr, ev_join = nullptr;
  size_t dz_h2_cap = 0, x_h2_cap = 0;
  std::vector<char> planes_fused;      // layer l's input planes were written by the previous layer's k_bn_apply_v this step
  bool dma_layer(int l) const {        // layer l's forward convolution runs as the DMA GEMM on pre-split planes (k_conv_h2dma)
    const TLayer& ly = layers[l];
    return dma_fwd && use_h2_fwd(ly.Cin_p, ly.Cout_p) && ly.Cin_p % 32 == 0 && ly.Cout_p % 256 == 0 && g.W >= 16 &&
           (size_t)B * g.Hp * g.Wp * ly.Cin_p * 2 < ((size_t)1 << 31);
  }
  bool use_wino(int cin, int cout) const {
    return wino && cin % 32 == 0 && cin >= 64 && conv3x3_raw_wino_h2_fits(B, g.H, g.W, cin, cout) &&
           (x3_force || (size_t)((g.M + 127) / 128) * ((cout + 127) / 128) >= (size_t)ctx->num_cus);
  }
  // AGZ_COMPUTE_WINO_H2 forward: the DIRECT convolution with fp16x2 products (conv_h2.hpp's kernel with a raw store) — no transform in
  // front of the products, so its rounding is that of fp32 accumulation (3e-7 of the output rms, the same as bf16x3), unlike the
  // Winograd forward that was removed
  bool use_h2_fwd(int cin, int cout) const {
    return wino && cin >= 64 && conv3x3_raw_h2_fits(B, g.H, g.W, cin, cout) &&
           (x3_force || (size_t)((g.M + 127) / 128) * (cout / 256) >= (size_t)ctx->num_cus);
  }
  // bf16x3 only where the 128-row tiles fill the chip (same rule as inference) and the filter has whole 16-channel chunks
  bool use_x3(const TLayer& ly, int cin, int cout) const {
    return x3 && ly.w3f && cin % 16 == 0 && cin >= 64 &&
           (x3_force || (size_t)((g.M + 127) / 128) * ((cout + 127) / 128) >= (size_t)ctx->num_cus);
  }
  std::vector<void*> allocs;
  template <typename T> int alloc(T** p, size_t n) {
    void* q = nullptr;
    AGZ_HIP_TRY(hipMalloc(&q, n * sizeof(T)));
    AGZ_HIP_TRY(hipMemsetAsync(q, 0, n * sizeof(T), ctx->stream));
    allocs.push_back(q); *p = (T*)q; return AGZ_OK;
  }
  // eval (agz_trainer_eval): the forward pass alone, normalising with the tracked estimates; touches neither G nor the tracked state
  int forward_backward_dev(const float* planes_dev, const float* pi_dev, const float* v_dev, bool eval = false);
  // data-parallel step (comm.hip, agz_trainer_forward_backward_allreduce): called once per slice of the flat gradient buffer as soon
  // as the kernels that write it have been ENQUEUED — heads first, then layer L .. 0 (the order of the backward pass, the same on
  // every rank) — with the stream whose completion means "slice written"; the slices tile [0, n_flat) exactly
  std::function<int(size_t off, size_t n, hipStream_t ready)> on_slice;
  unsigned* amax_prev = nullptr;   // [(L + 2) * 2] last step's amax_words: the range estimates k_bn_apply_v writes the next layer's planes under
  double* head_acc = nullptr;   // [16] partial sums of the head kernels' second form (statistics, cost, BatchNorm backward)
  // the loss kind (agz_trainer_set_loss; the caller's configuration like lr, in no checkpoint).  az_dz [B][A], az_do [B], az_row [B][2]
  // are allocated when the kind is first set to AGZ_LOSS_ALPHAZERO: a trainer that never asks allocates nothing
  int loss_kind = AGZ_LOSS_REFERENCE;
  float *az_dz = nullptr, *az_do = nullptr;
  double* az_row = nullptr;
  int head_rows[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // agz_trainer_last_rows(layer = L + 1): AGZ_ROWS_HEAD_*
  bool cost_valid = false;  // a forward (training or eval) has written cost[0..1] (agz_trainer_get_costs)
  bool fast_heads = true;   // agz_trainer_set_dma_forward(t, on | 2 * heads): the second form of the head kernels (A/B hook)
  bool dma_fwd = true;      // AGZ_COMPUTE_WINO_H2 forward convolutions through k_conv_h2dma (agz_trainer_set_dma_forward, agz_debug.h: A/B hook)
  bool hoist_w = true;      // ... every layer's weight images at the start of the step on the side stream (bit 3 of the same hook: per layer, in line)
  bool conv3 = true;        // bit 5 of the same hook set: k_conv_h2dma (a K step = one tap) instead of k_conv_h2dma3 (nine taps from one x image)
  int conv3_mode = 0;       // bits 6, 7 of the hook: k_conv_h2dma3<MODE> (decomposition runs: WRONG results)
  int conv3_span = -1;      // rows of k_conv_h2dma3's largest x image for this geometry (<= CD3_IMG or the kernel is not used)
  bool conv3_layer(int l) {
    const TLayer& ly = layers[l];
    if (!conv3 || !dma_layer(l) || ly.Cout_p % 128 != 0) return false;
    if (conv3_span < 0) {
      int mx = 0;
      for (int m0 = 0; m0 < g.M; m0 += 256)
        mx = std::max(mx, cmaps::cd3_rows(cmaps::pix(m0, g.HW, g.W, g.Hp, g.Wp), cmaps::pix(std::min(m0 + 255, g.M - 1), g.HW, g.W, g.Hp, g.Wp), g.Wp));
      conv3_span = mx;
    }
    return conv3_span <= CD3_IMG;
  }
  // k_wgrad_h2t3 at ONE workgroup per CU (round 6): 16 KB of unused dynamic LDS on top of its 73.7 KB make a second workgroup not fit.  Two per CU
  // hold the whole register file (243 registers x 2 waves per SIMD) and 147 of 160 KB of LDS: nothing of the main stream's chain (the data
  // gradient, the next layer's BatchNorm backward) could be resident beside it and the side stream overlapped 4 %.  One per CU runs 0.72 instead
  // of 0.53 ms on its own and leaves half of every SIMD's registers: both chains now progress together (the layer's backward 1.28 -> 1.19 ms,
  // the step 42.4 -> 41.0 ms on the same box; profiles/r06/train_overlap.md).  Bit 8 of the hook: two per CU again (A/B).
  int wg_pad_lds = 16384;
  bool wg_low_prio = false; // bit 9: the side stream at the lowest priority (set before the first step)
  bool one_stream = false;  // bit 4 of the same hook: no side stream at all (diagnostic: a kernel table without overlap shows every kernel's own duration)
  hipEvent_t ev_w0 = nullptr, ev_bw = nullptr;
  int side_stream();
  int prep_weights(bool fwd_only = false);
  // solver options (agz_trainer_set_solver; all 0 = the vanilla step, which then runs the kernels it always ran) and the first-order state:
  // V, one flat buffer laid out exactly like P / G, exists only while momentum != 0 (allocated and zeroed when it is first set, released
  // when it is set back to 0): a trainer that never asks for momentum allocates nothing more
  agz_solver_conf solver{0.f, 0.f, 0.f, 0};
  float* V = nullptr;
  bool solver_on() const { return solver.momentum != 0.f || solver.l2reg != 0.f || solver.clip != 0.f; }
  // Adam (agz_trainer_set_adam; excludes a momentum): M1 / M2, two flat buffers laid out like P / G / V, exist only while adam.on (allocated
  // and zeroed when it is turned on, released when it is turned off); adam_t counts the solver steps taken since.  agz_trainer_apply
  // advances adam_t; the fused kernels of the same step, which run before it, are given the constants of adam_t + 1.
  agz_adam_conf adam{0.9f, 0.999f, 1e-8f, 0};
  float* M1 = nullptr;
  float* M2 = nullptr;
  uint64_t adam_t = 0;
  AdamK adam_k(uint64_t step) const {
    const double b1 = adam.beta1, b2 = adam.beta2, n = (double)step;
    return AdamK{adam.beta1, (float)(1.0 - b1), adam.beta2, (float)(1.0 - b2), (float)(1.0 / (1.0 - std::pow(b1, n))),
                 (float)(1.0 / (1.0 - std::pow(b2, n))), adam.eps};
  }
  // running BatchNorm statistics (agz_trainer_set_bn_tracking; BnTrack above).  bn_st: one device allocation, made when tracking is first
  // turned on (or a state is first set / loaded): per finalize launch — tower layer 0 .. L, then the heads — S_mean[C] | S_var[C] | N[ops],
  // C the launch's (padded) channels.  bn_have[op]: N(op) > 0, known on the host without a read-back (a tracked forward makes every N >= 1).
  bool bn_on = false;
  float bn_lam = 0.997f;
  double* bn_st = nullptr;
  size_t bn_total = 0;
  std::vector<size_t> bn_base;         // [L + 2] offset of each launch's block in bn_st
  std::vector<char> bn_have;           // [2 L + 3] in the op order of agz_net_set_bn_stats
  struct BnOp { size_t mean, var, n; int C; };   // offsets into bn_st of one op's S_mean[C], S_var[C], N
  int bn_num() const { return 2 * L + 3; }
  BnOp bn_op(int i) const {
    if (i >= 2 * L + 1) {                // policy head (channels 0, 1), value head (channel 2)
      const size_t b = bn_base[L + 1]; const int v = i - (2 * L + 1);
      return BnOp{b + 2 * v, b + 3 + 2 * v, b + 6 + v, v ? 1 : 2};
    }
    const int l = (i + 1) / 2, br = i == 0 ? 0 : (i - 1) % 2, C = layers[l].Cout_p;   // Init, then L1 / L2 = branch a / b of block l
    const size_t b = bn_base[l];
    return BnOp{b + (size_t)br * Kp, b + C + (size_t)br * Kp, b + 2 * (size_t)C + br, K};
  }
  BnTrack bn_track(int launch) const {   // launch: tower layer 0 .. L, L + 1 = the heads
    const int C = launch <= L ? layers[launch].Cout_p : 3;
    return BnTrack{bn_st ? bn_st + bn_base[launch] : nullptr, C, launch <= L ? Kp : 2, (double)bn_lam};
  }
  bool bn_all() const { for (char h : bn_have) if (!h) return false; return !bn_have.empty(); }
  int bn_alloc() {
    if (bn_st) return AGZ_OK;
    bn_base.assign(L + 2, 0);
    size_t off = 0;
    for (int l = 0; l <= L; l++) { bn_base[l] = off; off += 2 * (size_t)layers[l].Cout_p + layers[l].nbr; }
    bn_base[L + 1] = off; off += 8;
    bn_total = off;
    bn_have.assign(bn_num(), 0);
    int r = alloc(&bn_st, bn_total);     // (zeroed: S = 0, N = 0)
    if (r != AGZ_OK) { bn_st = nullptr; return r; }
    AGZ_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return AGZ_OK;
  }
  // tied affine (agz_trainer_create_tied; DESIGN §2 `tied-affine`): every batch-shaped learnable is stored ONCE, at its row-0 shape (Bp = 1
  // parameter rows instead of B), in the same flat P / G / V / M1 / M2 layout.  tied_rows: the head kernels' per-row gradients of the head
  // gamma / beta and the FC biases (untied shapes: dhg, dhb [B][3][HW], dbp [B][A], db1 [B][FC], db2 [B]), summed into G by k_rows_sum;
  // tied_part [2][HW][2 Kp]: the per-pixel channel sums of k_bn_bwd1_tied.  On a tied sharded trainer (agz_trainer_bind_shard) it is followed
  // by the send buffer of a layer (s1 | s2 | dgamma | dbeta partials: tied_send()) and head_acc by the 6 HW + A + FC + 1 partials of the tied
  // head tensors.
  bool tied = false;
  int Bp = 0;               // parameter rows of a batch-shaped learnable: B, or 1 on a tied trainer
  float* tied_rows = nullptr;
  double* tied_part = nullptr;
  float fuse_lr = 0.f;      // != 0 during a fused step: k_bn_bwd1 updates gamma / beta in place, apply() skips them
  bool fused_done = false;  // the backward that just ran took the fused path
  // sharded trainer (agz_trainer_create_sharded): this rank's rows [rank * B, (rank + 1) * B) of a global batch of n_ranks * B rows.
  // B, g, P, G and every work buffer are this rank's; the BatchNorm statistics, the loss normalisation and the shared tensors' gradients
  // are the global batch's (the exchanges go through `shard`, comm.hip)
  bool sharded = false;
  int rank = 0, n_ranks = 1;
  agz_shard_hooks shard;
  double* xg = nullptr;     // [n_ranks][largest count of the exchange plan] the partial sums of one exchange, rank-major
  bool tied_sharded() const { return tied && sharded; }
  double* tied_send() const { return tied_part + (size_t)4 * g.HW * Kp; }
  size_t tied_head_n() const { return (size_t)6 * g.HW + A + FC + 1; }
  int m_glob() const { return g.M * n_ranks; }
  int exchange(int site, const double* send, size_t count) { return shard.gather(site, send, xg, count); }
  bool bn_single_pass(int C) const { return C % 4 == 0 && C <= 1024 && g.M >= 4096; }
  // forward_backward_dev, collective on a sharded trainer; pre != AGZ_OK: what filled the batch failed — nothing runs, and a sharded
  // step still enters its collectives with `pre` as this rank's status
  int step(const float* planes, const float* pi, const float* v, int pre = AGZ_OK);
  int eval_pass(const float* planes, const float* pi, const float* v);   // the forward-only pass; collective on a sharded trainer
};

static inline int nblk(size_t n, int bs = 256) { return (int)((n + bs - 1) / bs); }

// clears n regions of one buffer in a single launch (grid: x = blocks per region, y = region)
__global__ __launch_bounds__(256) void k_zero_regions(float* __restrict__ base, const size_t* __restrict__ tab, int n) {
  const size_t off = tab[blockIdx.y], cnt = tab[n + blockIdx.y];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) base[off + i] = 0.f;
}

int agz_trainer::side_stream() {
  if (wg_stream) return AGZ_OK;
  if (wg_low_prio) {
    int lo = 0, hi = 0;
    AGZ_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));   // (numerically larger = lower priority)
    AGZ_HIP_TRY(hipStreamCreateWithPriority(&wg_stream, hipStreamNonBlocking, lo));
  } else
    AGZ_HIP_TRY(hipStreamCreateWithFlags(&wg_stream, hipStreamNonBlocking));
  AGZ_HIP_TRY(hipEventCreateWithFlags(&ev_dz, hipEventDisableTiming));
  AGZ_HIP_TRY(hipEventCreateWithFlags(&ev_split, hipEventDisableTiming));
  AGZ_HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
  AGZ_HIP_TRY(hipEventCreateWithFlags(&ev_w0, hipEventDisableTiming));
  AGZ_HIP_TRY(hipEventCreateWithFlags(&ev_bw, hipEventDisableTiming));
  return AGZ_OK;
}

// AGZ_COMPUTE_WINO_H2: the filters are constant inside a step (apply() runs after the backward pass), so the per-layer weight passes — range
// word + fp16 hi / lo image for the DMA forward convolution (2 kernels), transpose + Winograd image for the data gradient (3 kernels), each a
// few MB of work that cannot fill the chip: 17 + 73 us per layer in line at G19 — are queued here on the side stream, which is otherwise
// idle until the backward pass: forward images first, in layer order with an event each, then the data gradient's with one event
int agz_trainer::prep_weights(bool fwd_only) {
  for (auto& ly : layers) { ly.fw_ready = false; ly.bw_ready = false; }
  if (!wino || !hoist_w || one_stream) return AGZ_OK;
  int r = side_stream();
  if (r != AGZ_OK) return r;
  hipStream_t s = ctx->stream, sw = wg_stream;
  AGZ_HIP_TRY(hipEventRecord(ev_w0, s));              // (the previous step's apply() and its readers of the images)
  AGZ_HIP_TRY(hipStreamWaitEvent(sw, ev_w0, 0));
  for (int l = 0; l <= L; l++) {
    TLayer& ly = layers[l];
    if (!dma_layer(l)) continue;
    if (!ly.ev_fw) AGZ_HIP_TRY(hipEventCreateWithFlags(&ly.ev_fw, hipEventDisableTiming));
    if ((r = agz::conv3x3_raw_h2_weights_to(ctx, sw, P + ly.o_wf, ly.Cin_p, ly.Cout_p, &ly.fw)) != AGZ_OK) return r;
    AGZ_HIP_TRY(hipEventRecord(ly.ev_fw, sw));
    ly.fw_ready = true;
  }
  for (int l = L; l >= 1 && !fwd_only; l--) {
    TLayer& ly = layers[l];
    const int C = ly.Cout_p;
    if (!use_wino(C, ly.Cin_p)) continue;
    hipLaunchKernelGGL(k_make_wt, dim3((unsigned)(((size_t)9 * C * ly.Cin_p + 255) / 256)), dim3(256), 0, sw, P + ly.o_wf, ly.wt, C, ly.Cin_p);
    if ((r = agz::conv3x3_raw_wino_h2_weights_to(ctx, sw, ly.wt, g.H, g.W, C, ly.Cin_p, &ly.bw)) != AGZ_OK) return r;
    ly.bw_ready = true;
  }
  AGZ_HIP_TRY(hipEventRecord(ev_bw, sw));
  return AGZ_OK;
}

int agz_trainer::forward_backward_dev(const float* planes, const float* pi, const float* v, bool eval) {
  hipStream_t s = ctx->stream;
  const int RPB = 64;
  const bool trk = bn_on && !eval;   // this forward's statistics go into the running estimates (the <true> finalize kernels)
  if (trk) std::fill(bn_have.begin(), bn_have.end(), (char)1);
  { int r0 = prep_weights(eval); if (r0 != AGZ_OK) return r0; }
  hipLaunchKernelGGL(k_pack_planes_t, dim3(nblk((size_t)g.M * Fp)), dim3(256), 0, s, planes, x0, g, F, Fp);
  if (!eval) {
  // zero the gradient regions that are ACCUMULATED into (filters: atomics; heads).  The batch-shaped gamma / beta gradients — 98 % of
  // the flat buffer — are plain stores of every element (k_bn_bwd1) and need no clearing (one 7.7 GB memset per G19 step saved)
  hipLaunchKernelGGL(k_zero_regions, dim3(64, L + 1), dim3(256), 0, s, G, zero_tab, L + 1);
  AGZ_HIP_TRY(hipMemsetAsync(G + o_hc, 0, (n_flat - o_hc) * sizeof(float), s));
  AGZ_HIP_TRY(hipMemsetAsync(acc_b, 0, (size_t)(L + 1) * 2048 * sizeof(double), s));
  }
  AGZ_HIP_TRY(hipMemcpyAsync(amax_prev, amax_words, (size_t)(L + 2) * 2 * sizeof(unsigned), hipMemcpyDeviceToDevice, s));   // (last step's ranges: estimates for the fused plane split)
  AGZ_HIP_TRY(hipMemsetAsync(amax_words, 0, (size_t)(L + 2) * 2 * sizeof(unsigned), s));
  AGZ_HIP_TRY(hipMemsetAsync(board_words, 0, (size_t)2 * (L + 2) * B * sizeof(unsigned), s));
  // ---- forward, training-mode BN
  const float* cur = x0;
  for (int l = 0; l <= L; l++) {
    TLayer& ly = layers[l];
    int r;
    ly.x_planes = false;
    const size_t n_x_fwd = (size_t)B * g.Hp * g.Wp * ly.Cin_p;
    if (dma_layer(l) && x_amax_ready[l]) {
      // planes of the layer input (its range word came out of the previous layer's BatchNorm pass, and so did the planes themselves
      // unless the range's exponent moved since the last step), then the DMA GEMM
      if (!ly.xh2) { r = alloc(&ly.xh2, 2 * n_x_fwd); if (r != AGZ_OK) return r; planes_fused[l] = 0; }
      const unsigned gs = (unsigned)std::min<size_t>(nblk(n_x_fwd / 4), (size_t)ctx->num_cus * 8);
      hipLaunchKernelGGL(k_split_h2p_cond, dim3(gs), dim3(256), 0, s, cur, ly.xh2, ly.xh2 + n_x_fwd, n_x_fwd / 4, amax_words + 2 * l + 1,
                         planes_fused[l] ? (const unsigned*)(amax_prev + 2 * l + 1) : (const unsigned*)nullptr);
      const void* w2 = nullptr; const unsigned* wmax = nullptr;
      if (ly.fw_ready) { AGZ_HIP_TRY(hipStreamWaitEvent(s, ly.ev_fw, 0)); w2 = ly.fw.img; wmax = ly.fw.words; }
      else if ((r = conv3x3_raw_h2_weights(ctx, P + ly.o_wf, ly.Cin_p, ly.Cout_p, &wsc, &w2, &wmax)) != AGZ_OK) return r;
      ConvDmaArgs ca{};
      ca.xh = ly.xh2; ca.xl = ly.xh2 + n_x_fwd; ca.w2 = (const _Float16*)w2; ca.y = ly.z; ca.x_amax = amax_words + 2 * l + 1; ca.w_amax = wmax;
      ca.g = g; ca.Cin = ly.Cin_p; ca.Ntot = ly.Cout_p;
      if (conv3_layer(l)) {
        ca.n_mtiles = ceil_div(g.M, 256); ca.n_ntiles = ly.Cout_p / 128;
        switch (conv3_mode) {
          case 1: hipLaunchKernelGGL(k_conv_h2dma3<1>, dim3(ca.n_mtiles * ca.n_ntiles), dim3(256), 0, s, ca); break;
          case 2: hipLaunchKernelGGL(k_conv_h2dma3<2>, dim3(ca.n_mtiles * ca.n_ntiles), dim3(256), 0, s, ca); break;
          case 3: hipLaunchKernelGGL(k_conv_h2dma3<3>, dim3(ca.n_mtiles * ca.n_ntiles), dim3(256), 0, s, ca); break;
          default: hipLaunchKernelGGL(k_conv_h2dma3<0>, dim3(ca.n_mtiles * ca.n_ntiles), dim3(256), 0, s, ca); break;
        }
        ly.path_fwd = AGZ_PATH_FWD_H2DMA3;
      } else {
        ca.n_mtiles = ceil_div(g.M, 128); ca.n_ntiles = ly.Cout_p / 256;
        hipLaunchKernelGGL(k_conv_h2dma, dim3(ca.n_mtiles * ca.n_ntiles), dim3(256), 0, s, ca);
        ly.path_fwd = AGZ_PATH_FWD_H2DMA;
      }
      ly.x_planes = true;
      r = AGZ_OK;
    } else if (use_h2_fwd(ly.Cin_p, ly.Cout_p)) {
      r = conv3x3_raw_h2(ctx, cur, P + ly.o_wf, ly.z, B, g.H, g.W, ly.Cin_p, ly.Cout_p, &wsc, xb_ready[l] ? board_words + (size_t)l * B : nullptr);
      ly.path_fwd = AGZ_PATH_FWD_H2W;
    } else if (use_x3(ly, ly.Cin_p, ly.Cout_p)) {
      if ((r = split_w3(ctx, P + ly.o_wf, ly.w3f, ly.Cout_p, ly.Cin_p)) != AGZ_OK) return r;
      r = conv3x3_raw_x3(ctx, cur, ly.w3f, ly.z, B, g.H, g.W, ly.Cin_p, ly.Cout_p);
      ly.path_fwd = AGZ_PATH_FWD_BF16X3;
    } else {
      r = conv3x3_raw(ctx, cur, P + ly.o_wf, ly.z, B, g.H, g.W, ly.Cin_p, ly.Cout_p);
      ly.path_fwd = AGZ_PATH_FWD_F32;
    }
    if (r != AGZ_OK) return r;
    int C = ly.Cout_p;
    const BnTrack bt = bn_track(l);
    ly.rows[AGZ_ROWS_SINGLE_PASS] = !eval && bn_single_pass(C);
    // (sharded: this rank's partial sums are gathered from every rank and k_bn_fin_ranks sums them in rank order over the global rows)
    if (eval) {   // the tracked estimates in place of this batch's statistics
      hipLaunchKernelGGL(k_bn_from_running, dim3(nblk(C)), dim3(256), 0, s, bt, conf.bn_eps, ly.mean, ly.inv);
    } else if (bn_single_pass(C)) {   // (small problems keep the two-pass form: nothing to gain, and it is the oracle's order)
      hipLaunchKernelGGL(k_bn_stats, dim3(nblk(g.M, 128)), dim3(256), 0, s, g, ly.z, C, acc, 128);   // (256 / 128 / 64 / 32 rows: 46 / 37 / 46 / 71 us at G19)
      if (sharded) {
        if ((r = exchange(l, acc, 2048)) != AGZ_OK) return r;
        hipLaunchKernelGGL(trk ? k_bn_fin_ranks<true> : k_bn_fin_ranks<false>, dim3(nblk(C)), dim3(256), 0, s, xg, n_ranks, 2048, acc, C, (double)m_glob(), conf.bn_eps, ly.mean, ly.inv, 2, bt);
      } else
        hipLaunchKernelGGL(trk ? k_bn_fin2<true> : k_bn_fin2<false>, dim3(nblk(C)), dim3(256), 0, s, acc, C, (double)g.M, conf.bn_eps, ly.mean, ly.inv, bt);
    } else {
      for (int pass = 0; pass < 2; pass++) {   // the mean over the global rows first, then the centred sums around it (the oracle's order)
        hipLaunchKernelGGL(k_bn_sum, dim3(nblk(g.M, RPB)), dim3(std::min(C, 512)), 0, s, g, ly.z, C, pass ? (const float*)ly.mean : (const float*)nullptr, acc, RPB);
        if (sharded) {
          if ((r = exchange(l, acc, 1024)) != AGZ_OK) return r;
          hipLaunchKernelGGL(trk ? k_bn_fin_ranks<true> : k_bn_fin_ranks<false>, dim3(nblk(C)), dim3(256), 0, s, xg, n_ranks, 1024, acc, C, (double)m_glob(), conf.bn_eps, ly.mean, ly.inv, pass, bt);
        } else
          hipLaunchKernelGGL(trk ? k_bn_fin<true> : k_bn_fin<false>, dim3(nblk(C)), dim3(256), 0, s, acc, C, (double)g.M, conf.bn_eps, ly.mean, ly.inv, pass, bt);
      }
    }
    x_amax_ready[l + 1] = 0; xb_ready[l + 1] = 0;
    if (wino && Kp % 4 == 0 && Kp / 4 <= 256 && 256 % (Kp / 4) == 0 && ly.nbr <= 2) {
      const int tpr = 256 / (Kp / 4), rpb = round_up(std::max(tpr, ceil_div(g.M, 2048)), tpr);
      const bool per_board = rpb <= g.HW;   // (a block's rows then lie in at most two boards)
      // the next layer's DMA convolution reads `out` as fp16 hi / lo planes: written here, under last step's range (k_split_h2p_cond checks)
      _Float16* nph = nullptr;
      if (l < L && dma_layer(l + 1) && layers[l + 1].Cin_p == Kp) {
        TLayer& nx = layers[l + 1];
        const size_t n_nx = (size_t)B * g.Hp * g.Wp * nx.Cin_p;
        if (!nx.xh2) { int r2 = alloc(&nx.xh2, 2 * n_nx); if (r2 != AGZ_OK) return r2; }
        nph = nx.xh2;
        planes_fused[l + 1] = 1;
      } else if (l < L) planes_fused[l + 1] = 0;
      hipLaunchKernelGGL(tied ? k_bn_apply_v<true> : k_bn_apply_v<false>, dim3(nblk(g.M, rpb)), dim3(256), 0, s, g, ly.z, P + ly.o_gamma, P + ly.o_beta, ly.mean, ly.inv, ly.out,
                         Kp, ly.nbr, rpb, amax_words + 2 * (l + 1) + 1, per_board ? board_words + (size_t)(l + 1) * B : nullptr,
                         nph, nph ? nph + (size_t)B * g.Hp * g.Wp * Kp : nullptr, (const unsigned*)(amax_prev + 2 * (l + 1) + 1));
      x_amax_ready[l + 1] = 1;
      xb_ready[l + 1] = per_board;
      ly.rows[AGZ_ROWS_APPLY_RPB] = rpb; ly.rows[AGZ_ROWS_APPLY_BOARD_WORDS] = per_board;
    } else {
      if (l < L) planes_fused[l + 1] = 0;
      ly.rows[AGZ_ROWS_APPLY_RPB] = 0; ly.rows[AGZ_ROWS_APPLY_BOARD_WORDS] = 0;
      hipLaunchKernelGGL(tied ? k_bn_apply<true> : k_bn_apply<false>, dim3(nblk((size_t)g.M * Kp)), dim3(256), 0, s, g, ly.z, P + ly.o_gamma, P + ly.o_beta, ly.mean,
                         ly.inv, ly.out, Kp, ly.nbr);
    }
    cur = ly.out;
  }
  // ---- heads forward
  HeadT h{};
  h.B = B; h.Bn = B * n_ranks; h.HW = g.HW; h.A = A; h.FC = FC; h.yh = yh; h.Wp = P + o_Wp; h.bp = P + o_bp; h.W1 = P + o_W1; h.b1 = P + o_b1;
  h.W2 = P + o_W2; h.b2 = P + o_b2; h.Pi = pi; h.V = v; h.logits = logits; h.hpre = hpre; h.o = o;
  h.dWp = G + o_Wp; h.dbp = G + o_bp; h.dW1 = G + o_W1; h.db1 = G + o_b1; h.dW2 = G + o_W2; h.db2 = G + o_b2; h.dyh = dyh; h.cost = cost;
  const bool az = loss_kind == AGZ_LOSS_ALPHAZERO;
  if (az) { h.az_dz = az_dz; h.az_do = az_do; h.az_row = az_row; }
  // tied: the head kernels write their per-row gradients of the batch-shaped tensors into tied_rows; k_rows_sum adds the rows into G
  float *dhg = G + o_hg, *dhb = G + o_hb;
  if (tied) {
    dhg = tied_rows; dhb = dhg + (size_t)B * 3 * g.HW;
    h.dbp = dhb + (size_t)B * 3 * g.HW; h.db1 = h.dbp + (size_t)B * A; h.db2 = h.db1 + (size_t)B * FC;
  }
  // (second form of the head kernels: see k_head_conv2 ... above; fast_heads = 0, agz_debug.h, keeps the first form for A/B)
  const int fcK = 2 * g.HW > FC ? 2 * g.HW : FC, fcJ = A > FC ? A : FC;
  const bool fh = (fast_heads || sharded) && (size_t)8 * (2 * g.HW) * 4 <= 60000 && (size_t)B * 8 * 4 <= 60000 && (size_t)8 * fcJ * 4 <= 60000 && fcK > 0;
  const BnTrack hbt = bn_track(L + 1);
  if (fh) {
    AGZ_HIP_TRY(hipMemsetAsync(head_acc, 0, 16 * sizeof(double), s));
    const int g_conv2 = std::min(nblk(g.M, 4), ctx->num_cus * 16), g_stats = std::min(nblk(g.M), ctx->num_cus), g_cost = std::min(nblk((size_t)B * A), 64);
    head_rows[AGZ_ROWS_HEAD_SECOND_FORM] = 1; head_rows[AGZ_ROWS_HEAD_CONV2_GRID] = g_conv2;
    head_rows[AGZ_ROWS_HEAD_STATS_GRID] = eval ? 0 : g_stats; head_rows[AGZ_ROWS_HEAD_COST_GRID] = az ? 0 : g_cost;
    hipLaunchKernelGGL(k_head_conv2, dim3(g_conv2), dim3(256), 0, s, g, cur, P + o_hc, zh, Kp);
    if (eval) hipLaunchKernelGGL(k_bn_from_running, dim3(1), dim3(64), 0, s, hbt, conf.bn_eps, hmean, hinv);
    else {
    hipLaunchKernelGGL(k_head_stats_part, dim3(g_stats), dim3(256), 0, s, g, zh, head_acc);
    if (sharded) {   // (head_acc [16] is gathered whole; each exchange sums the ranks' part it concerns into this rank's head_acc)
      int r = exchange(L + 1, head_acc, 16);
      if (r != AGZ_OK) return r;
      hipLaunchKernelGGL(k_sum_ranks, dim3(1), dim3(64), 0, s, xg, n_ranks, 16, head_acc, 0, 6);
    }
    hipLaunchKernelGGL(trk ? k_head_stats_fin<true> : k_head_stats_fin<false>, dim3(1), dim3(64), 0, s, g, head_acc, conf.bn_eps, hmean, hinv, (double)m_glob(), hbt);
    }
    hipLaunchKernelGGL(tied ? k_head_apply<true> : k_head_apply<false>, dim3(nblk((size_t)g.M * 3)), dim3(256), 0, s, g, zh, P + o_hg, P + o_hb, hmean, hinv, yh);
    hipLaunchKernelGGL(tied ? k_fc_fwd2<true> : k_fc_fwd2<false>, dim3(nblk(std::max(A, FC)), nblk(B, 8), 2), dim3(256), (size_t)8 * 2 * g.HW * sizeof(float), s, h);
    hipLaunchKernelGGL(tied ? k_value_out2<true> : k_value_out2<false>, dim3(B), dim3(64), 0, s, h);
    if (az) {
      hipLaunchKernelGGL(k_az_loss, dim3(B), dim3(64), 0, s, h);
      hipLaunchKernelGGL(k_az_cost_sum, dim3(1), dim3(64), 0, s, h, head_acc);
    } else
    hipLaunchKernelGGL(k_cost_part, dim3(g_cost), dim3(256), 0, s, h, head_acc);
    if (sharded) {
      int r = exchange(L + 1, head_acc, 16);
      if (r != AGZ_OK) return r;
      hipLaunchKernelGGL(k_sum_ranks, dim3(1), dim3(64), 0, s, xg, n_ranks, 16, head_acc, 6, 2);
    }
    hipLaunchKernelGGL(az ? k_cost_fin<true> : k_cost_fin<false>, dim3(1), dim3(64), 0, s, h, head_acc);
  } else {
  std::fill(head_rows, head_rows + 8, 0);
  hipLaunchKernelGGL(k_head_conv, dim3(nblk((size_t)g.M * 3)), dim3(256), 0, s, g, cur, P + o_hc, zh, Kp);
  if (eval) hipLaunchKernelGGL(k_bn_from_running, dim3(1), dim3(64), 0, s, hbt, conf.bn_eps, hmean, hinv);
  else hipLaunchKernelGGL(trk ? k_head_stats<true> : k_head_stats<false>, dim3(3), dim3(256), 0, s, g, zh, conf.bn_eps, hmean, hinv, hbt);
  hipLaunchKernelGGL(tied ? k_head_apply<true> : k_head_apply<false>, dim3(nblk((size_t)g.M * 3)), dim3(256), 0, s, g, zh, P + o_hg, P + o_hb, hmean, hinv, yh);
  hipLaunchKernelGGL(tied ? k_fc_fwd<true> : k_fc_fwd<false>, dim3(nblk((size_t)B * A + (size_t)B * FC)), dim3(256), 0, s, h);
  hipLaunchKernelGGL(tied ? k_value_out<true> : k_value_out<false>, dim3(nblk(B)), dim3(256), 0, s, h);
  if (az) {
    hipLaunchKernelGGL(k_az_loss, dim3(B), dim3(64), 0, s, h);
    hipLaunchKernelGGL(k_az_cost_sum, dim3(1), dim3(64), 0, s, h, (double*)nullptr);
  } else
  hipLaunchKernelGGL(k_cost, dim3(1), dim3(256), 0, s, h);
  }
  cost_valid = true;
  if (eval) { AGZ_HIP_TRY(hipGetLastError()); return AGZ_OK; }   // (forward only: no gradient, no state touched)
  // ---- heads backward
  size_t n_fc = (size_t)2 * g.HW * A + (size_t)B * A + (size_t)g.HW * FC + (size_t)B * FC + FC + B + (size_t)B * 3 * g.HW;
  if (fh) {
    hipLaunchKernelGGL(az ? k_fc_bwd_w<true> : k_fc_bwd_w<false>, dim3(nblk(std::max(A, FC)), nblk(2 * g.HW, 8), 2), dim3(256), (size_t)B * 8 * sizeof(float), s, h);
    hipLaunchKernelGGL(az ? k_fc_bwd_small<true> : k_fc_bwd_small<false>, dim3(nblk((size_t)B * A + (size_t)B * FC + FC + B)), dim3(256), 0, s, h);
    hipLaunchKernelGGL(az ? k_fc_bwd_y<true> : k_fc_bwd_y<false>, dim3(nblk(2 * g.HW), nblk(B, 8), 2), dim3(256), (size_t)8 * fcJ * sizeof(float), s, h);
    hipLaunchKernelGGL(tied ? k_head_bn_bwd_a<true> : k_head_bn_bwd_a<false>, dim3(std::min(nblk(g.M), ctx->num_cus)), dim3(256), 0, s, g, zh, yh, dyh, P + o_hg, hmean, hinv, dhg, dhb, dzh, head_acc);
    if (tied_sharded()) {
      // the five tied head tensors' partials over this rank's rows ride the same gather, behind the 16 words; summed in rank order into G
      const size_t nt = tied_head_n(), cnt = 16 + nt;
      RowSum rs{{dhg, dhb, h.dbp, h.db1, h.db2}, {nullptr, nullptr, nullptr, nullptr, nullptr}, {3 * g.HW, 3 * g.HW, A, FC, 1}};
      hipLaunchKernelGGL(k_rows_sum<true>, dim3(nblk(nt)), dim3(256), 0, s, rs, B, head_acc + 16);
      int r = exchange(L + 1, head_acc, cnt);
      if (r != AGZ_OK) return r;
      hipLaunchKernelGGL(k_sum_ranks, dim3(1), dim3(64), 0, s, xg, n_ranks, (int)cnt, head_acc, 8, 6);
      RowDst rd{{G + o_hg, G + o_hb, G + o_bp, G + o_b1, G + o_b2}, {3 * g.HW, 3 * g.HW, A, FC, 1}};
      hipLaunchKernelGGL(k_rows_ranks, dim3(nblk(nt)), dim3(256), 0, s, xg + 16, n_ranks, cnt, rd);
    } else if (sharded) {
      int r = exchange(L + 1, head_acc, 16);
      if (r != AGZ_OK) return r;
      hipLaunchKernelGGL(k_sum_ranks, dim3(1), dim3(64), 0, s, xg, n_ranks, 16, head_acc, 8, 6);
    }
    hipLaunchKernelGGL(k_head_bn_bwd_b, dim3(nblk((size_t)g.M * 3)), dim3(256), 0, s, g, zh, hmean, hinv, dzh, head_acc, (float)m_glob());
    hipLaunchKernelGGL(k_head_conv_bwd_w2, dim3(nblk(g.M, RPB)), dim3(256), 0, s, g, cur, dzh, G + o_hc, Kp, RPB);
  } else {
  hipLaunchKernelGGL(az ? k_fc_bwd<true> : k_fc_bwd<false>, dim3(nblk(n_fc)), dim3(256), 0, s, h);
  hipLaunchKernelGGL(tied ? k_head_bn_bwd<true> : k_head_bn_bwd<false>, dim3(3), dim3(256), 0, s, g, zh, yh, dyh, P + o_hg, hmean, hinv, dhg, dhb, dzh);
  hipLaunchKernelGGL(k_head_conv_bwd_w, dim3(nblk(g.M, RPB)), dim3(256), 0, s, g, cur, dzh, G + o_hc, Kp, RPB);
  }
  if (tied && !sharded) {
    RowSum rs{{dhg, dhb, h.dbp, h.db1, h.db2}, {G + o_hg, G + o_hb, G + o_bp, G + o_b1, G + o_b2}, {3 * g.HW, 3 * g.HW, A, FC, 1}};
    hipLaunchKernelGGL(k_rows_sum<false>, dim3(nblk((size_t)6 * g.HW + A + FC + 1)), dim3(256), 0, s, rs, B, (double*)nullptr);
  }
  float* dcur = dA;
  float* dnext = dB;
  if (fh) hipLaunchKernelGGL(k_head_conv_bwd_x2, dim3(nblk((size_t)g.M * (Kp / 4))), dim3(256), 0, s, g, dzh, P + o_hc, dcur, Kp);
  else hipLaunchKernelGGL(k_head_conv_bwd_x, dim3(nblk((size_t)g.M * Kp)), dim3(256), 0, s, g, dzh, P + o_hc, dcur, Kp);
  if (wino) {
    // the weight gradient's fp16 scratch at its largest layer, BEFORE the first slice goes to the reduction queue: an allocation failure
    // between two slices would leave the peers waiting in the collectives this rank never enters
    size_t need_dz = 0, need_x = 0;
    for (int l = 0; l <= L; l++) {
      need_dz = std::max(need_dz, (size_t)B * g.Hp * g.Wp * layers[l].Cout_p);
      need_x = std::max(need_x, (size_t)B * g.Hp * g.Wp * layers[l].Cin_p);
    }
    if (dz_h2_cap < need_dz) { if (dz_h2) hipFree(dz_h2); dz_h2 = nullptr; dz_h2_cap = 0; AGZ_HIP_TRY(hipMalloc(&dz_h2, need_dz * 4)); dz_h2_cap = need_dz; }
    if (x_h2_cap < need_x) { if (x_h2) hipFree(x_h2); x_h2 = nullptr; x_h2_cap = 0; AGZ_HIP_TRY(hipMalloc(&x_h2, need_x * 4)); x_h2_cap = need_x; }
  }
  if (on_slice) { int r = on_slice(o_hc, n_flat - o_hc, s); if (r != AGZ_OK) return r; }   // the heads' gradients are final
  // ---- tower backward
  { int r = side_stream(); if (r != AGZ_OK) return r; }
  hipStream_t sw = one_stream ? s : wg_stream;
  if (wino && hoist_w && !one_stream) AGZ_HIP_TRY(hipStreamWaitEvent(s, ev_bw, 0));   // the data gradient's weight images (prep_weights; long done)
  for (int l = L; l >= 0; l--) {
    TLayer& ly = layers[l];
    int C = ly.Cout_p;
    const float* xin = l == 0 ? x0 : layers[l - 1].out;
    double* s1 = acc_b + (size_t)l * 2048; double* s2 = s1 + 1024;
    unsigned* wg_amax = amax_words + 2 * l;
    float* dz = l == 0 ? this->dz0 : this->dz;  // (different pixel strides: keep the [pix][2Kp] buffer's zero halo intact)
    if (sw != s && l < L) AGZ_HIP_TRY(hipStreamWaitEvent(s, ev_split, 0));   // the previous layer's weight gradient has taken its copy of dz
    {
      // (the solver variants only on a fused step with an option set: everything else launches the instantiation without them)
      const bool sv_adam = fuse_lr != 0.f && adam.on, sv_on = fuse_lr != 0.f && solver_on(), sv_mom = sv_on && solver.momentum != 0.f;
      SolverDev sd{solver.momentum, solver.l2reg, solver.clip, sv_mom ? V + ly.o_gamma : nullptr, sv_mom ? V + ly.o_beta : nullptr,
                   AdamK{}, nullptr, nullptr, nullptr, nullptr};
      if (sv_adam) {   // (the step agz_trainer_apply is about to count: adam_t + 1)
        sd.ak = adam_k(adam_t + 1);
        sd.m1gamma = M1 + ly.o_gamma; sd.m1beta = M1 + ly.o_beta; sd.m2gamma = M2 + ly.o_gamma; sd.m2beta = M2 + ly.o_beta;
      }
      if (tied_sharded()) {   // this rank's double partials and channel sums into the layer's send buffer (nothing rounded, nothing stepped)
        hipLaunchKernelGGL((k_bn_bwd1_tied<SK_VANILLA, true>), dim3(g.HW * ceil_div(C, 64)), dim3(256), 0, s, g, ly.z, P + ly.o_gamma, P + ly.o_beta, ly.mean,
                           ly.inv, ly.out, dcur, G + ly.o_gamma, G + ly.o_beta, dz, tied_part, Kp, ly.nbr, 0.f, sd);
        hipLaunchKernelGGL(k_bn_tied_sums, dim3(nblk((size_t)2 * C, 16)), dim3(256), 0, s, tied_part, g.HW, C, tied_send(), tied_send() + 1024);
      } else if (tied) {   // one workgroup per (pixel, 64 channels) owns the element for all B boards; then the channel sums in a fixed pixel order
        auto* bwd1t = sv_adam ? k_bn_bwd1_tied<SK_ADAM> : sv_mom ? k_bn_bwd1_tied<SK_MOMENTUM> : sv_on ? k_bn_bwd1_tied<SK_OPTIONS> : k_bn_bwd1_tied<SK_VANILLA>;
        hipLaunchKernelGGL(bwd1t, dim3(g.HW * ceil_div(C, 64)), dim3(256), 0, s, g, ly.z, P + ly.o_gamma, P + ly.o_beta, ly.mean, ly.inv,
                           ly.out, dcur, G + ly.o_gamma, G + ly.o_beta, dz, tied_part, Kp, ly.nbr, fuse_lr, sd);
        hipLaunchKernelGGL(k_bn_tied_sums, dim3(nblk((size_t)2 * C, 16)), dim3(256), 0, s, tied_part, g.HW, C, s1, s2);
      } else {
      auto* bwd1 = sv_adam ? k_bn_bwd1<SK_ADAM> : sv_mom ? k_bn_bwd1<SK_MOMENTUM> : sv_on ? k_bn_bwd1<SK_OPTIONS> : k_bn_bwd1<SK_VANILLA>;
      hipLaunchKernelGGL(bwd1, dim3(nblk(g.M, RPB)), dim3(std::min(C, 512)), 0, s, g, ly.z, P + ly.o_gamma, P + ly.o_beta, ly.mean, ly.inv,
                         ly.out, dcur, G + ly.o_gamma, G + ly.o_beta, dz, s1, s2, Kp, ly.nbr, RPB, fuse_lr, sd);
      }
    }
    if (tied_sharded()) {
      // ONE gather of s1 | s2 | dgamma | dbeta partials; the channel sums into acc_b of this layer, where step 2 reads them, and the tied
      // gradient in rank order: stored (two-pass) or stepped in place with the solver of the fused step (the constants of adam_t + 1)
      const size_t nt = (size_t)2 * g.HW * C, cnt = 2048 + nt;
      int r = exchange(l, tied_send(), cnt);
      if (r != AGZ_OK) return r;
      // (k_bn_tied_sums wrote words [0, C) of each half of the send buffer; the rest of the 2 x 1024 is whatever a wider layer left there,
      // summed into acc_b as well and never read: step 2 reads channels < C, and acc_b is cleared at the start of a step)
      hipLaunchKernelGGL(k_sum_ranks, dim3(nblk(2048)), dim3(256), 0, s, xg, n_ranks, (int)cnt, s1, 0, 2048);
      const bool sv_adam = fuse_lr != 0.f && adam.on, sv_on = fuse_lr != 0.f && solver_on(), sv_mom = sv_on && solver.momentum != 0.f;
      const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(nblk(nt), (size_t)ctx->num_cus * 8));
      const size_t og = ly.o_gamma;   // [gamma | beta], contiguous
      if (sv_adam) hipLaunchKernelGGL(k_tied_ranks<SK_ADAM>, dim3(grid), dim3(256), 0, s, xg + 2048, n_ranks, cnt, nt, P + og, G + og, M1 + og, M2 + og, fuse_lr, 0.f, solver.l2reg, solver.clip, adam_k(adam_t + 1));
      else if (sv_mom) hipLaunchKernelGGL(k_tied_ranks<SK_MOMENTUM>, dim3(grid), dim3(256), 0, s, xg + 2048, n_ranks, cnt, nt, P + og, G + og, V + og, (float*)nullptr, fuse_lr, solver.momentum, solver.l2reg, solver.clip, AdamK{});
      else if (sv_on) hipLaunchKernelGGL(k_tied_ranks<SK_OPTIONS>, dim3(grid), dim3(256), 0, s, xg + 2048, n_ranks, cnt, nt, P + og, G + og, (float*)nullptr, (float*)nullptr, fuse_lr, solver.momentum, solver.l2reg, solver.clip, AdamK{});
      else hipLaunchKernelGGL(k_tied_ranks<SK_VANILLA>, dim3(grid), dim3(256), 0, s, xg + 2048, n_ranks, cnt, nt, P + og, G + og, (float*)nullptr, (float*)nullptr, fuse_lr, 0.f, 0.f, 0.f, AdamK{});
    } else if (sharded) {   // the two channel sums over the global batch (in place: acc_b of this layer holds the ranks' sum afterwards)
      int r = exchange(l, s1, 2048);
      if (r != AGZ_OK) return r;
      hipLaunchKernelGGL(k_sum_ranks, dim3(nblk(2048)), dim3(256), 0, s, xg, n_ranks, 2048, s1, 0, 2048);
    }
    bool dz_amax_ready = false, dzb_ready = false;
    if (wino && C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0) {
      const int tpr = 256 / (C / 4), rpb = round_up(std::max(tpr, ceil_div(g.M, 2048)), tpr);
      dzb_ready = rpb <= g.HW;
      hipLaunchKernelGGL(k_bn_bwd2_v, dim3(nblk(g.M, rpb)), dim3(256), 0, s, g, ly.z, ly.mean, ly.inv, dz, s1, s2, C, rpb, wg_amax,
                         dzb_ready ? board_words + (size_t)(L + 2 + l) * B : nullptr, (float)m_glob());
      dz_amax_ready = true;
      ly.path_bn2 = AGZ_PATH_BN2_V;
      ly.rows[AGZ_ROWS_BWD2_RPB] = rpb; ly.rows[AGZ_ROWS_BWD2_BOARD_WORDS] = dzb_ready;
    } else {
      ly.rows[AGZ_ROWS_BWD2_RPB] = 0; ly.rows[AGZ_ROWS_BWD2_BOARD_WORDS] = 0;
      hipLaunchKernelGGL(k_bn_bwd2, dim3(nblk((size_t)g.M * C)), dim3(256), 0, s, g, ly.z, ly.mean, ly.inv, dz, s1, s2, C, (float)m_glob());
      ly.path_bn2 = AGZ_PATH_BN2_SCALAR;
    }
    // weight gradient (on its own stream from here)
    if (sw != s) { AGZ_HIP_TRY(hipEventRecord(ev_dz, s)); AGZ_HIP_TRY(hipStreamWaitEvent(sw, ev_dz, 0)); }
    bool split_recorded = false;
    WgArgs wa{};
    wa.dz = dz; wa.x = xin; wa.dw = G + ly.o_wf; wa.g = g; wa.N = C; wa.Cin = ly.Cin_p; wa.rows_per_block = 2048;   // rows of the reduction per workgroup
    wa.n_tiles = ceil_div(C, 128); wa.c_tiles = ceil_div(ly.Cin_p, 128);
    int chunks = ceil_div(g.M, wa.rows_per_block);
    wa.n_chunks = chunks;
    const unsigned wg_grid = (unsigned)(wa.n_tiles * wa.c_tiles * 9 * round_up(chunks, 8));   // k_wgrad_x3 / _h2: XCD-aware order
    const bool chip_full = x3_force || (size_t)wa.n_tiles * wa.c_tiles * 9 * chunks >= (size_t)ctx->num_cus;
    const bool off31 = (size_t)B * g.Hp * g.Wp * (size_t)std::max(C, ly.Cin_p) * 4 < ((size_t)1 << 31);   // byte offsets of the buffer loads
    ly.rows[AGZ_ROWS_WGRAD_CHUNKS] = chunks; ly.rows[AGZ_ROWS_SPLIT_BLOCKS] = 0; ly.rows[AGZ_ROWS_SPLIT_NEED] = 0;
    if (wino && chip_full && off31 && C % 4 == 0 && ly.Cin_p % 4 == 0) {
      // fp16x2 products: range + split pass over dz and x (once per layer, not once per tap workgroup), then the GEMM
      const size_t n_dz = (size_t)B * g.Hp * g.Wp * C, n_x = (size_t)B * g.Hp * g.Wp * ly.Cin_p;
      if (dz_h2_cap < n_dz) { if (dz_h2) hipFree(dz_h2); dz_h2 = nullptr; dz_h2_cap = 0; AGZ_HIP_TRY(hipMalloc(&dz_h2, n_dz * 4)); dz_h2_cap = n_dz; }
      if (x_h2_cap < n_x) { if (x_h2) hipFree(x_h2); x_h2 = nullptr; x_h2_cap = 0; AGZ_HIP_TRY(hipMalloc(&x_h2, n_x * 4)); x_h2_cap = n_x; }
      const unsigned gs = (unsigned)std::min<size_t>(nblk(n_dz / 4), (size_t)ctx->num_cus * 8);
      ly.rows[AGZ_ROWS_SPLIT_BLOCKS] = (int)gs; ly.rows[AGZ_ROWS_SPLIT_NEED] = nblk(n_dz / 4);
      if (!dz_amax_ready) hipLaunchKernelGGL(k_absmax, dim3(gs), dim3(256), 0, sw, dz, n_dz / 4, wg_amax);
      if (!x_amax_ready[l]) hipLaunchKernelGGL(k_absmax, dim3(gs), dim3(256), 0, sw, xin, n_x / 4, wg_amax + 1);
      if (g.W >= 16 && C % 8 == 0 && ly.Cin_p % 8 == 0) {
        // three taps per workgroup from hi / lo fp16 planes (k_wgrad_h2t3)
        _Float16* dzh = (_Float16*)dz_h2; _Float16* dzl = dzh + n_dz;
        _Float16* xh = ly.x_planes ? ly.xh2 : (_Float16*)x_h2; _Float16* xl = xh + n_x;   // (the forward pass's planes of this input, if it made them)
        hipLaunchKernelGGL(k_split_h2p, dim3(gs), dim3(256), 0, sw, dz, dzh, dzl, n_dz / 4, wg_amax);
        if (sw != s) { AGZ_HIP_TRY(hipEventRecord(ev_split, sw)); split_recorded = true; }
        if (!ly.x_planes) hipLaunchKernelGGL(k_split_h2p, dim3(gs), dim3(256), 0, sw, xin, xh, xl, n_x / 4, wg_amax + 1);
        WgH2t3Args w3{};
        w3.dzh = dzh; w3.dzl = dzl; w3.xh = xh; w3.xl = xl; w3.amax = wg_amax; w3.dw = wa.dw; w3.g = g; w3.N = wa.N; w3.Cin = wa.Cin;
        w3.n_tiles = wa.n_tiles; w3.c_tiles = wa.c_tiles; w3.steps_per_board = ceil_div(g.HW, 32);
        const int per_chunk3 = wa.n_tiles * wa.c_tiles * 3;
        // chunks of boards: a chunk's workgroups share an XCD (its L2 holds the chunk's rows), an XCD runs 2 workgroups on each of its
        // CUs; about two rounds of them (5 chunks x 24 workgroups on 64 slots at K = 256; 4 to 8 chunks per XCD measured within 5 %)
        const int slots = ctx->num_cus / 8 * 2;
        w3.n_chunks = std::min(B, 8 * std::max(1, 2 * slots / per_chunk3));
        hipLaunchKernelGGL(k_wgrad_h2t3, dim3((unsigned)(per_chunk3 * round_up(w3.n_chunks, 8))), dim3(256), (size_t)wg_pad_lds, sw, w3);
        ly.path_wgrad = AGZ_PATH_WGRAD_H2T3;
        ly.rows[AGZ_ROWS_WGRAD_CHUNKS] = w3.n_chunks;
      } else {
        hipLaunchKernelGGL(k_split_h2, dim3(gs), dim3(256), 0, sw, dz, dz_h2, n_dz / 4, wg_amax);
        if (sw != s) { AGZ_HIP_TRY(hipEventRecord(ev_split, sw)); split_recorded = true; }
        hipLaunchKernelGGL(k_split_h2, dim3(gs), dim3(256), 0, sw, xin, x_h2, n_x / 4, wg_amax + 1);
        WgH2Args wh{};
        wh.dz2 = dz_h2; wh.x2 = x_h2; wh.amax = wg_amax; wh.dw = wa.dw; wh.g = g; wh.N = wa.N; wh.Cin = wa.Cin;
        wh.rows_per_block = wa.rows_per_block; wh.n_tiles = wa.n_tiles; wh.c_tiles = wa.c_tiles; wh.n_chunks = chunks;
        hipLaunchKernelGGL(k_wgrad_h2, dim3(wg_grid), dim3(256), 0, sw, wh);
        ly.path_wgrad = AGZ_PATH_WGRAD_H2;
      }
    }
    // bf16x3 mode: the weight gradient runs on the bf16 pipe as well
    else if (x3 && off31 && chip_full) {
      hipLaunchKernelGGL(k_wgrad_x3, dim3(wg_grid), dim3(256), 0, sw, wa);
      ly.path_wgrad = AGZ_PATH_WGRAD_X3;
    } else {
      hipLaunchKernelGGL(k_wgrad, dim3(wa.n_tiles * wa.c_tiles * 9 * chunks), dim3(256), 0, sw, wa);
      ly.path_wgrad = AGZ_PATH_WGRAD_F32;
    }
    if (sw != s && !split_recorded) AGZ_HIP_TRY(hipEventRecord(ev_split, sw));   // (kernels that read dz itself: after the weight gradient)
    // layer l's slice [filter | gamma | beta] is final once its weight gradient has run (sw: it started after this layer's BatchNorm backward)
    if (on_slice) { int r = on_slice(ly.o_wf, (l < L ? layers[l + 1].o_wf : o_hc) - ly.o_wf, sw); if (r != AGZ_OK) return r; }
    if (l > 0) {  // data gradient: the forward GEMM with flipped/transposed weights over the [a|b] channels of dz
      if (!ly.bw_ready) hipLaunchKernelGGL(k_make_wt, dim3(nblk((size_t)9 * C * ly.Cin_p)), dim3(256), 0, s, P + ly.o_wf, ly.wt, C, ly.Cin_p);
      int r;
      if (use_wino(C, ly.Cin_p)) {
        r = conv3x3_raw_wino_h2(ctx, dz, ly.wt, dnext, B, g.H, g.W, C, ly.Cin_p, &wsc, dzb_ready ? board_words + (size_t)(L + 2 + l) * B : nullptr,
                                ly.bw_ready ? &ly.bw : nullptr);
        ly.path_dgrad = AGZ_PATH_DGRAD_WINO_H2;
      } else if (use_x3(ly, C, ly.Cin_p)) {
        if ((r = split_w3(ctx, ly.wt, ly.w3t, ly.Cin_p, C)) != AGZ_OK) return r;
        r = conv3x3_raw_x3(ctx, dz, ly.w3t, dnext, B, g.H, g.W, C, ly.Cin_p);
        ly.path_dgrad = AGZ_PATH_DGRAD_X3;
      } else {
        r = conv3x3_raw(ctx, dz, ly.wt, dnext, B, g.H, g.W, C, ly.Cin_p);
        ly.path_dgrad = AGZ_PATH_DGRAD_RAW;
      }
      if (r != AGZ_OK) return r;
      std::swap(dcur, dnext);
    }
  }
  if (sw != s) { AGZ_HIP_TRY(hipEventRecord(ev_join, sw)); AGZ_HIP_TRY(hipStreamWaitEvent(s, ev_join, 0)); }   // the step's stream carries everything again
  AGZ_HIP_TRY(hipGetLastError());
  return AGZ_OK;
}

// (comm.hip) the context a trainer was created on
agz_ctx* agz_trainer_ctx(const agz_trainer* t) { return t ? t->ctx : nullptr; }
void agz_trainer_set_slice_hook(agz_trainer* t, std::function<int(size_t, size_t, hipStream_t)> f) { t->on_slice = std::move(f); }
// the slices forward_backward_dev hands to on_slice, in the order it issues them: the heads, then layer L .. 0 ([filter | gamma | beta])
void agz_trainer_slices(const agz_trainer* t, std::vector<std::pair<size_t, size_t>>& out) {
  out.clear();
  out.emplace_back(t->o_hc, t->n_flat - t->o_hc);
  const int L = (int)t->layers.size() - 1;
  for (int l = L; l >= 0; l--) out.emplace_back(t->layers[l].o_wf, (l < L ? t->layers[l + 1].o_wf : t->o_hc) - t->layers[l].o_wf);
}

// one training step's forward / backward; on a sharded trainer a COLLECTIVE step (the communicator enters whatever exchanges a failure
// skipped, sums the shared tensors' gradients and agrees on the status: comm.hip)
int agz_trainer::step(const float* planes, const float* pi, const float* v, int pre) {
  if (!sharded) return pre != AGZ_OK ? pre : forward_backward_dev(planes, pi, v);
  return shard.step([&]() -> int {
    if (pre != AGZ_OK) return pre;
    const int r = forward_backward_dev(planes, pi, v);
    if (r != AGZ_OK) {
      // a step that failed part-way may have left work on the side stream: join it, so that the next step starts on a quiet trainer; and
      // the forward statistics' sums of the layer it stopped at were never finalized (which clears them): clear them here
      if (wg_stream && hipEventRecord(ev_join, wg_stream) == hipSuccess) hipStreamWaitEvent(ctx->stream, ev_join, 0);
      hipMemsetAsync(acc, 0, 2048 * sizeof(double), ctx->stream);
    }
    return r;
  });
}

int agz_trainer::eval_pass(const float* planes, const float* pi, const float* v) {
  if (!sharded) return forward_backward_dev(planes, pi, v, true);
  return shard.eval_step([&]() -> int { return forward_backward_dev(planes, pi, v, true); });
}

int agz_trainer_bind_shard(agz_trainer* t, int rank, int n, agz_shard_hooks hooks) {
  AGZ_REQUIRE(t && n >= 1 && rank >= 0 && rank < n, AGZ_E_INVALID, "agz_trainer_bind_shard: rank %d of %d", rank, n);
  // the sharded step exchanges the partial sums of the second form of the head kernels (forward_backward_dev: fh)
  const int fcJ = std::max(t->A, t->FC);
  AGZ_REQUIRE((size_t)8 * (2 * t->g.HW) * 4 <= 60000 && (size_t)t->B * 8 * 4 <= 60000 && (size_t)8 * fcJ * 4 <= 60000, AGZ_E_UNSUPPORTED,
              "sharded trainer: board, batch or action space too large for the head kernels it runs");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  // Everything is allocated first and the handle changed last: a failure leaves it the unbound trainer it was.
  // The gather buffer holds n slices of the largest exchange of the plan: 2048 doubles, or on a tied trainer the largest backward gather,
  // which carries the tied tensors' partials as well (agz_trainer_exchange_plan).  A gather that a failed step never issued is entered
  // in place from slice `rank` of it (comm.hip).  A tied trainer's tied_part and head_acc are replaced by ones with room for the send
  // buffers behind them (tied_send(); the head partials): agz_trainer_create_tied itself allocates what it always did.
  size_t mx = 2048;
  double *xg = nullptr, *part = nullptr, *hacc = nullptr;
  int r = AGZ_OK;
  if (t->tied) {
    for (const auto& ly : t->layers) mx = std::max(mx, 2048 + (size_t)2 * t->g.HW * ly.Cout_p);
    mx = std::max(mx, 16 + t->tied_head_n());
    if ((r = t->alloc(&part, (size_t)4 * t->g.HW * 2 * t->Kp + 2048)) != AGZ_OK || (r = t->alloc(&hacc, 16 + t->tied_head_n())) != AGZ_OK) return r;
  }
  if ((r = t->alloc(&xg, (size_t)n * mx)) != AGZ_OK) return r;
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  if (t->tied) {
    for (void* old : {(void*)t->tied_part, (void*)t->head_acc}) {
      t->allocs.erase(std::find(t->allocs.begin(), t->allocs.end(), old));
      hipFree(old);
    }
    t->tied_part = part; t->head_acc = hacc;
  }
  t->xg = xg;
  t->sharded = true; t->rank = rank; t->n_ranks = n; t->shard = std::move(hooks);
  return AGZ_OK;
}
bool agz_trainer_is_sharded(const agz_trainer* t) { return t && t->sharded; }
// the gathers of forward_backward_dev in issue order: per tower layer 0 .. L one (single-pass statistics) or two (two-pass), the heads'
// statistics, cost and BatchNorm backward, then the backward BatchNorm sums of layer L .. 0
void agz_trainer_exchange_plan(const agz_trainer* t, std::vector<size_t>& out, bool eval) {
  out.clear();
  if (eval) { out.push_back(16); return; }   // agz_trainer_eval: the cost words alone
  for (const auto& ly : t->layers) {
    if (t->bn_single_pass(ly.Cout_p)) out.push_back(2048);
    else { out.push_back(1024); out.push_back(1024); }
  }
  // (tied: the heads' backward gather and every layer's carry the double partials of the tied tensors' gradients behind the sums)
  const bool ts = t->tied && t->sharded;
  for (int k = 0; k < 3; k++) out.push_back(k == 2 && ts ? 16 + t->tied_head_n() : 16);
  for (int l = t->L; l >= 0; l--) out.push_back(2048 + (ts ? (size_t)2 * t->g.HW * t->layers[l].Cout_p : 0));
}
double* agz_trainer_gather_buf(agz_trainer* t) { return t->xg; }
void agz_trainer_shared_ranges(const agz_trainer* t, std::vector<std::pair<size_t, size_t>>& out) {
  out.clear();
  for (const auto& ly : t->layers) out.emplace_back(ly.o_wf, (size_t)9 * ly.Cout_p * ly.Cin_p);
  out.emplace_back(t->o_hc, (size_t)3 * t->Kp);
  out.emplace_back(t->o_Wp, (size_t)2 * t->g.HW * t->A);
  out.emplace_back(t->o_W1, (size_t)t->g.HW * t->FC);
  out.emplace_back(t->o_W2, (size_t)t->FC);
}

// batch-shaped learnables (gamma / beta of every BatchNorm, the FC biases): dimension 0 is the batch, a sharded trainer holds its rows
static bool pref_batch_shaped(const TParamRef& p) { return p.kind == 1 || p.kind == 3; }

extern "C" {

int agz_trainer_shard(const agz_trainer* t, int* row0, int* rows, int* n_ranks) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_shard: NULL trainer");
  if (row0) *row0 = t->rank * t->B;
  if (rows) *rows = t->B;
  if (n_ranks) *n_ranks = t->n_ranks;
  return AGZ_OK;
}

static int trainer_create(agz_ctx* ctx, const agz_net_conf* c, agz_trainer** out, bool tied);
int agz_trainer_create(agz_ctx* ctx, const agz_net_conf* c, agz_trainer** out) { return trainer_create(ctx, c, out, false); }
// every batch-shaped learnable at its row-0 shape, shared by the BatchSize rows of a step (include/agz.h; DESIGN §2 `tied-affine`)
int agz_trainer_create_tied(agz_ctx* ctx, const agz_net_conf* c, agz_trainer** out) { return trainer_create(ctx, c, out, true); }
int agz_trainer_is_tied(const agz_trainer* t, int* tied) {
  AGZ_REQUIRE(t && tied, AGZ_E_INVALID, "agz_trainer_is_tied: NULL argument");
  *tied = t->tied ? 1 : 0;
  return AGZ_OK;
}
static int trainer_create(agz_ctx* ctx, const agz_net_conf* c, agz_trainer** out, bool tied) {
  AGZ_REQUIRE(ctx && c && out, AGZ_E_INVALID, "agz_trainer_create: NULL argument");
  AGZ_REQUIRE(c->K >= 1 && c->ActionSpace >= 3 && c->SharedLayers >= 0 && c->FC > 1 && c->BatchSize >= 1 && c->Features > 0,
              AGZ_E_INVALID, "agz_trainer_create: NNConf is not valid");
  AGZ_REQUIRE(c->Features <= 32, AGZ_E_UNSUPPORTED, "Features > 32 unsupported");
  AGZ_HIP_TRY(hipSetDevice(ctx->device));
  agz_trainer* t = new agz_trainer();
  t->ctx = ctx; t->conf = *c; t->tied = tied; t->Bp = tied ? 1 : c->BatchSize;
  t->K = c->K; t->Kp = round_up(c->K, 32); t->L = c->SharedLayers; t->A = c->ActionSpace; t->FC = c->FC; t->B = c->BatchSize; t->F = c->Features;
  AGZ_REQUIRE(2 * t->Kp <= 1024, AGZ_E_UNSUPPORTED, "K > 512 unsupported by the trainer");
  TGeo& g = t->g;
  g.B = t->B; g.H = c->Height; g.W = c->Width; g.HW = g.H * g.W; g.Hp = g.H + 2; g.Wp = g.W + 2; g.M = g.B * g.HW;
  const int K = t->K, Kp = t->Kp, HW = g.HW, B = t->B, H = g.H, W = g.W, A = t->A, FCn = t->FC, F = t->F;
  const int Bp = t->Bp;   // rows of the batch-shaped learnables (1 on a tied trainer: the shapes below are then the inference net's)
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += (n + 3) & ~(size_t)3; return o; };
  t->layers.resize(t->L + 1);
  for (int l = 0; l <= t->L; l++) {
    TLayer& ly = t->layers[l];
    ly.nbr = l == 0 ? 1 : 2; ly.Cin_p = l == 0 ? t->Fp : Kp; ly.Cout_p = ly.nbr * Kp;
    ly.o_wf = take((size_t)9 * ly.Cout_p * ly.Cin_p);
    ly.o_gamma = take((size_t)Bp * HW * ly.Cout_p);
    ly.o_beta = take((size_t)Bp * HW * ly.Cout_p);
  }
  t->o_hc = take((size_t)3 * Kp); t->o_hg = take((size_t)Bp * 3 * HW); t->o_hb = take((size_t)Bp * 3 * HW);
  t->o_Wp = take((size_t)2 * HW * A); t->o_bp = take((size_t)Bp * A); t->o_W1 = take((size_t)HW * FCn); t->o_b1 = take((size_t)Bp * FCn);
  t->o_W2 = take(FCn); t->o_b2 = take(Bp);
  t->n_flat = off;
  // reference Model() order (include/agz.h)
  auto pr = [&](const std::string& nm, int kind, std::vector<int> shp, int layer, int sub) { t->prefs.push_back(TParamRef{nm, kind, shp, layer, sub}); };
  pr("FilterInit", 0, {K, F, 3, 3}, 0, 0); pr("Init_gamma", 1, {Bp, K, H, W}, 0, 1); pr("Init_beta", 1, {Bp, K, H, W}, 0, 2);
  for (int i = 0; i < t->L; i++) {
    std::string s = std::to_string(i);
    pr("FilterLayer1 of Shared Layer " + s, 0, {K, K, 3, 3}, i + 1, 0); pr("L1_" + s + "_gamma", 1, {Bp, K, H, W}, i + 1, 1); pr("L1_" + s + "_beta", 1, {Bp, K, H, W}, i + 1, 2);
    pr("FilterLayer2 of Shared Layer " + s, 0, {K, K, 3, 3}, i + 1, 10); pr("L2_" + s + "_gamma", 1, {Bp, K, H, W}, i + 1, 11); pr("L2_" + s + "_beta", 1, {Bp, K, H, W}, i + 1, 12);
  }
  pr("FilterPolicyHead", 0, {2, K, 1, 1}, -1, 0); pr("PolicyHead_gamma", 1, {Bp, 2, H, W}, -1, 1); pr("PolicyHead_beta", 1, {Bp, 2, H, W}, -1, 2);
  pr("Policy_w", 2, {2 * HW, A}, -1, 3); pr("Policy_b", 3, {Bp, A}, -1, 4);
  pr("FilterValueHead", 0, {1, K, 1, 1}, -2, 0); pr("ValueHead_gamma", 1, {Bp, 1, H, W}, -2, 1); pr("ValueHead_beta", 1, {Bp, 1, H, W}, -2, 2);
  pr("Value_w", 2, {HW, FCn}, -2, 3); pr("Value_b", 3, {Bp, FCn}, -2, 4);
  pr("ValueOutput_w", 2, {FCn, 1}, -2, 5); pr("ValueOutput_b", 3, {Bp, 1}, -2, 6);
  int r = AGZ_OK;
#define TAL(p, n) if ((r = t->alloc(&t->p, (size_t)(n))) != AGZ_OK) { agz_trainer_destroy(t); return r; }
  TAL(P, t->n_flat) TAL(G, t->n_flat)
  size_t px = (size_t)B * g.Hp * g.Wp;
  TAL(x0, px * t->Fp) TAL(dA, px * Kp) TAL(dB, px * Kp) TAL(dz, px * 2 * Kp) TAL(dz0, px * Kp) TAL(acc, 2048)   /* [2][1024] channel sums of the forward BatchNorm (self-clearing) */
  TAL(acc_b, (size_t)(t->L + 1) * 2048) TAL(amax_words, (size_t)(t->L + 2) * 2) TAL(zero_tab, (size_t)(t->L + 1) * 2)
  TAL(board_words, (size_t)2 * (t->L + 2) * B)
  t->x_amax_ready.assign(t->L + 2, 0); t->xb_ready.assign(t->L + 2, 0); t->planes_fused.assign(t->L + 2, 0);
  {
    std::vector<size_t> tab((size_t)(t->L + 1) * 2);
    for (int l = 0; l <= t->L; l++) {
      tab[l] = t->layers[l].o_wf;
      tab[t->L + 1 + l] = (size_t)9 * t->layers[l].Cout_p * t->layers[l].Cin_p;
    }
    AGZ_HIP_TRY(hipMemcpyAsync(t->zero_tab, tab.data(), tab.size() * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));   // (after alloc()'s clear, same stream)
    AGZ_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  for (int l = 0; l <= t->L; l++) {
    TLayer& ly = t->layers[l];
    if ((r = t->alloc(&ly.z, px * ly.Cout_p)) != AGZ_OK || (r = t->alloc(&ly.out, px * Kp)) != AGZ_OK ||
        (r = t->alloc(&ly.mean, (size_t)ly.Cout_p)) != AGZ_OK || (r = t->alloc(&ly.inv, (size_t)ly.Cout_p)) != AGZ_OK ||
        (r = t->alloc(&ly.wt, (size_t)9 * ly.Cout_p * ly.Cin_p)) != AGZ_OK) { agz_trainer_destroy(t); return r; }
  }
  TAL(zh, (size_t)g.M * 3) TAL(yh, (size_t)g.M * 3) TAL(dyh, (size_t)g.M * 3) TAL(dzh, (size_t)g.M * 3) TAL(hmean, 4) TAL(hinv, 4)
  TAL(logits, (size_t)B * A) TAL(hpre, (size_t)B * FCn) TAL(o, B) TAL(cost, 2) TAL(head_acc, 16) TAL(amax_prev, (size_t)(t->L + 2) * 2)
  TAL(d_planes, (size_t)B * F * HW) TAL(d_pi, (size_t)B * A) TAL(d_v, B)
  if (tied) { TAL(tied_rows, (size_t)B * (6 * HW + A + FCn + 1)) TAL(tied_part, (size_t)2 * HW * 2 * Kp) }
#undef TAL
  AGZ_HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out = t;
  return AGZ_OK;
}

void agz_trainer_destroy(agz_trainer* t) {
  if (!t) return;
  hipSetDevice(t->ctx->device);
  hipStreamSynchronize(t->ctx->stream);
  if (t->wg_stream) { hipStreamSynchronize(t->wg_stream); hipStreamDestroy(t->wg_stream); }
  for (auto& ly : t->layers) { agz::raw_weights_free(&ly.fw); agz::raw_weights_free(&ly.bw); if (ly.ev_fw) hipEventDestroy(ly.ev_fw); }
  if (t->ev_w0) hipEventDestroy(t->ev_w0);
  if (t->ev_bw) hipEventDestroy(t->ev_bw);
  if (t->ev_dz) hipEventDestroy(t->ev_dz);
  if (t->ev_split) hipEventDestroy(t->ev_split);
  if (t->ev_join) hipEventDestroy(t->ev_join);
  for (void* p : t->allocs) hipFree(p);
  wino_raw_scratch_free(&t->wsc);
  if (t->dz_h2) hipFree(t->dz_h2);
  if (t->x_h2) hipFree(t->x_h2);
  if (t->V) hipFree(t->V);
  if (t->M1) hipFree(t->M1);
  if (t->M2) hipFree(t->M2);
  delete t;
}

int agz_trainer_num_params(const agz_trainer* t) { return t ? (int)t->prefs.size() : 0; }

static size_t pref_size(const TParamRef& p) { size_t n = 1; for (int d : p.shape) n *= (size_t)d; return n; }

int agz_trainer_param_info(const agz_trainer* t, int i, char* name, size_t cap, size_t* n) {
  AGZ_REQUIRE(t && i >= 0 && i < (int)t->prefs.size(), AGZ_E_INVALID, "agz_trainer_param_info: bad index");
  if (name && cap) { strncpy(name, t->prefs[i].name.c_str(), cap - 1); name[cap - 1] = 0; }
  if (n) *n = pref_size(t->prefs[i]);
  return AGZ_OK;
}

// reference layout <-> device layout for parameter i of flat buffer `buf` (P or G). dir 0: host -> device, 1: device -> host
// nb_sel > 0: only the first nb_sel batch rows of a conv-layer gamma/beta (agz_trainer_export needs row 0 only)
// (B below is the number of PARAMETER rows: a tied trainer's batch-shaped tensors have one, and a tied tensor is its own row 0)
static int xfer_param(const agz_trainer* t, float* buf, int i, float* host, int dir, int nb_sel = 0) {
  const TParamRef& p = t->prefs[i];
  const int K = t->K, Kp = t->Kp, HW = t->g.HW, B = (nb_sel > 0 && nb_sel < t->Bp && t->prefs[i].layer >= 0 && (t->prefs[i].sub % 10) != 0) ? nb_sel : t->Bp, A = t->A, FCn = t->FC, F = t->F, Fp = t->Fp;
  hipStream_t s = t->ctx->stream;
  auto dev_rw = [&](size_t off, std::vector<float>& tmp) -> int {
    if (dir == 0) AGZ_HIP_TRY(hipMemcpyAsync(buf + off, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice, s));
    else AGZ_HIP_TRY(hipMemcpyAsync(tmp.data(), buf + off, tmp.size() * 4, hipMemcpyDeviceToHost, s));
    AGZ_HIP_TRY(hipStreamSynchronize(s));
    return AGZ_OK;
  };
  if (p.layer >= 0) {
    const TLayer& ly = t->layers[p.layer];
    int br = p.sub >= 10 ? 1 : 0, sub = p.sub % 10;
    int Cin = p.layer == 0 ? F : K, Cin_p = ly.Cin_p, C = ly.Cout_p;
    if (sub == 0) {  // filter [K][Cin][3][3] <-> wf[tap][br*Kp + o][ci]
      std::vector<float> tmp((size_t)9 * C * Cin_p);
      if (hipMemcpy(tmp.data(), buf + ly.o_wf, tmp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { agz::set_error("xfer: D2H failed"); return AGZ_E_HIP; }
      for (int o = 0; o < K; o++) for (int ci = 0; ci < Cin; ci++) for (int tp = 0; tp < 9; tp++) {
        size_t di = ((size_t)tp * C + br * Kp + o) * Cin_p + ci, hi = ((size_t)o * Cin + ci) * 9 + tp;
        if (dir == 0) tmp[di] = host[hi]; else host[hi] = tmp[di];
      }
      if (dir == 0) return dev_rw(ly.o_wf, tmp);
      return AGZ_OK;
    }
    // gamma/beta [B][K][H][W] <-> [r = b*HW+p][br*Kp + c]: only this tensor's Kp-wide column block moves (strided 2-D
    // copy), the host-side transpose runs on all cores — a 19x19 / K=256 / B=256 trainer has 82 such tensors of 94 MB
    size_t off = sub == 1 ? ly.o_gamma : ly.o_beta;
    const size_t M = (size_t)B * HW;   // (B is nb_sel when only the leading rows are wanted)
    std::vector<float> tmp(M * Kp, 0.f);
    float* dcol = buf + off + (size_t)br * Kp;
    if (dir == 1 && hipMemcpy2D(tmp.data(), (size_t)Kp * 4, dcol, (size_t)C * 4, (size_t)Kp * 4, M, hipMemcpyDeviceToHost) != hipSuccess) {
      agz::set_error("xfer: D2H failed"); return AGZ_E_HIP;
    }
    auto work = [&](int b_lo, int b_hi) {
      for (int b = b_lo; b < b_hi; b++)
        for (int q = 0; q < HW; q++) {
          float* trow = tmp.data() + ((size_t)b * HW + q) * Kp;
          for (int c = 0; c < K; c++) {
            size_t hi = ((size_t)b * K + c) * HW + q;
            if (dir == 0) trow[c] = host[hi]; else host[hi] = trow[c];
          }
        }
    };
    unsigned nthr = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    if ((size_t)B * K * HW < (1u << 16) || nthr == 1) work(0, B);
    else {
      std::vector<std::thread> th;
      int per = (B + (int)nthr - 1) / (int)nthr;
      for (int lo = 0; lo < B; lo += per) th.emplace_back(work, lo, std::min(B, lo + per));
      for (auto& x : th) x.join();
    }
    if (dir == 0 && hipMemcpy2D(dcol, (size_t)C * 4, tmp.data(), (size_t)Kp * 4, (size_t)Kp * 4, M, hipMemcpyHostToDevice) != hipSuccess) {
      agz::set_error("xfer: H2D failed"); return AGZ_E_HIP;
    }
    return AGZ_OK;
  }
  // heads
  const bool pol = p.layer == -1;
  auto plain = [&](size_t off, size_t n) -> int {
    if (dir == 0) AGZ_HIP_TRY(hipMemcpy(buf + off, host, n * 4, hipMemcpyHostToDevice));
    else AGZ_HIP_TRY(hipMemcpy(host, buf + off, n * 4, hipMemcpyDeviceToHost));
    return AGZ_OK;
  };
  if (p.sub == 0) {  // 1x1 filter [nc][K] <-> hc[j][Kp]
    int nc = pol ? 2 : 1, j0 = pol ? 0 : 2;
    std::vector<float> tmp((size_t)3 * Kp);
    AGZ_HIP_TRY(hipMemcpy(tmp.data(), buf + t->o_hc, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int j = 0; j < nc; j++) for (int c = 0; c < K; c++) { if (dir == 0) tmp[(size_t)(j0 + j) * Kp + c] = host[(size_t)j * K + c]; else host[(size_t)j * K + c] = tmp[(size_t)(j0 + j) * Kp + c]; }
    if (dir == 0) AGZ_HIP_TRY(hipMemcpy(buf + t->o_hc, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    return AGZ_OK;
  }
  if (p.sub == 1 || p.sub == 2) {  // head gamma/beta [B][nc][HW] <-> [B][3][HW]
    int nc = pol ? 2 : 1, j0 = pol ? 0 : 2;
    size_t off = p.sub == 1 ? t->o_hg : t->o_hb;
    std::vector<float> tmp((size_t)B * 3 * HW);
    AGZ_HIP_TRY(hipMemcpy(tmp.data(), buf + off, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++) for (int j = 0; j < nc; j++) for (int q = 0; q < HW; q++) {
      size_t di = ((size_t)b * 3 + j0 + j) * HW + q, hi = ((size_t)b * nc + j) * HW + q;
      if (dir == 0) tmp[di] = host[hi]; else host[hi] = tmp[di];
    }
    if (dir == 0) AGZ_HIP_TRY(hipMemcpy(buf + off, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    return AGZ_OK;
  }
  if (pol) return p.sub == 3 ? plain(t->o_Wp, (size_t)2 * HW * A) : plain(t->o_bp, (size_t)B * A);
  switch (p.sub) {
    case 3: return plain(t->o_W1, (size_t)HW * FCn);
    case 4: return plain(t->o_b1, (size_t)B * FCn);
    case 5: return plain(t->o_W2, FCn);
    default: return plain(t->o_b2, B);
  }
  (void)Fp;
}

int agz_trainer_set_param(agz_trainer* t, int i, const float* host, size_t n) {
  AGZ_REQUIRE(t && host && i >= 0 && i < (int)t->prefs.size(), AGZ_E_INVALID, "agz_trainer_set_param: bad argument");
  AGZ_REQUIRE(n == pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_set_param(%s): need %zu floats, got %zu", t->prefs[i].name.c_str(), pref_size(t->prefs[i]), n);
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return xfer_param(t, t->P, i, const_cast<float*>(host), 0);
}
int agz_trainer_get_param(const agz_trainer* t, int i, float* host, size_t n) {
  AGZ_REQUIRE(t && host && i >= 0 && i < (int)t->prefs.size() && n >= pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_get_param: bad argument");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return xfer_param(t, t->P, i, host, 1);
}
int agz_trainer_get_grad(const agz_trainer* t, int i, float* host, size_t n) {
  AGZ_REQUIRE(t && host && i >= 0 && i < (int)t->prefs.size() && n >= pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_get_grad: bad argument");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return xfer_param(t, t->G, i, host, 1);
}

// ---- solver options (gorgonia's solver constructor options, dualnet/meta.go:20) ---------------------------------------------------------
using agz::ckpt::solver_conf_valid;   // (the options' validity rules: ckpt.hpp, which applies them to a checkpoint as well)
// momentum != 0 for the first time: the velocity buffer, zeroed; momentum back to 0: released (v has no meaning without it).  The options
// change only if the call succeeds.  (Sharded: a local call; every rank sets the same options, as every rank passes the same lr.)
int agz_trainer_set_solver(agz_trainer* t, const agz_solver_conf* c) {
  AGZ_REQUIRE(t && c, AGZ_E_INVALID, "agz_trainer_set_solver: NULL argument");
  AGZ_REQUIRE(solver_conf_valid(c), AGZ_E_INVALID,
              "agz_trainer_set_solver: need 0 <= momentum < 1, l2reg >= 0, clip >= 0, all finite, reserved = 0 (got %g, %g, %g, %d)",
              (double)c->momentum, (double)c->l2reg, (double)c->clip, (int)c->reserved);
  AGZ_REQUIRE(!(c->momentum != 0.f && t->adam.on), AGZ_E_STATE,
              "agz_trainer_set_solver: a momentum and Adam exclude each other (turn Adam off first: agz_trainer_set_adam)");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  if (c->momentum != 0.f && !t->V) {
    float* v = nullptr;
    if (hipMalloc(&v, t->n_flat * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      agz::set_error("agz_trainer_set_solver: out of device memory for the velocity (%zu bytes)", t->n_flat * sizeof(float));
      return AGZ_E_NOMEM;
    }
    if (hipMemsetAsync(v, 0, t->n_flat * sizeof(float), t->ctx->stream) != hipSuccess || hipStreamSynchronize(t->ctx->stream) != hipSuccess) {
      hipFree(v);
      agz::set_error("agz_trainer_set_solver: clearing the velocity failed");
      return AGZ_E_HIP;
    }
    t->V = v;
  } else if (c->momentum == 0.f && t->V) {
    AGZ_HIP_TRY(hipFree(t->V));
    t->V = nullptr;
  }
  t->solver = *c;
  return AGZ_OK;
}
int agz_trainer_get_solver(const agz_trainer* t, agz_solver_conf* out) {
  AGZ_REQUIRE(t && out, AGZ_E_INVALID, "agz_trainer_get_solver: NULL argument");
  *out = t->solver;
  return AGZ_OK;
}
int agz_trainer_get_velocity(const agz_trainer* t, int i, float* host, size_t n) {
  AGZ_REQUIRE(t && host && i >= 0 && i < (int)t->prefs.size() && n >= pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_get_velocity: bad argument");
  if (!t->V) { std::fill(host, host + pref_size(t->prefs[i]), 0.f); return AGZ_OK; }   // (no momentum: no velocity)
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return xfer_param(t, t->V, i, host, 1);
}
int agz_trainer_set_velocity(agz_trainer* t, int i, const float* host, size_t n) {
  AGZ_REQUIRE(t && host && i >= 0 && i < (int)t->prefs.size(), AGZ_E_INVALID, "agz_trainer_set_velocity: bad argument");
  AGZ_REQUIRE(n == pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_set_velocity(%s): need %zu floats, got %zu", t->prefs[i].name.c_str(), pref_size(t->prefs[i]), n);
  AGZ_REQUIRE(t->V, AGZ_E_STATE, "agz_trainer_set_velocity: the trainer has no velocity (set a momentum != 0 first: agz_trainer_set_solver)");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return xfer_param(t, t->V, i, const_cast<float*>(host), 0);
}
int agz_trainer_reset_solver(agz_trainer* t) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_reset_solver: NULL trainer");
  t->adam_t = 0;
  if (!t->V && !t->M1) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  if (t->V) AGZ_HIP_TRY(hipMemsetAsync(t->V, 0, t->n_flat * sizeof(float), t->ctx->stream));
  if (t->M1) {
    AGZ_HIP_TRY(hipMemsetAsync(t->M1, 0, t->n_flat * sizeof(float), t->ctx->stream));
    AGZ_HIP_TRY(hipMemsetAsync(t->M2, 0, t->n_flat * sizeof(float), t->ctx->stream));
  }
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return AGZ_OK;
}

// ---- Adam (gorgonia.NewAdamSolver on the solver line, dualnet/meta.go:20; the definition: include/agz.h, DESIGN §2 `solver-adam`) ------
using agz::ckpt::adam_conf_valid;
// on for the first time: the two moment buffers, zeroed, and t = 0; off: both released, t = 0.  The settings change only if the call
// succeeds.  (Sharded: a local call; every rank makes it alike.)
int agz_trainer_set_adam(agz_trainer* t, const agz_adam_conf* c) {
  AGZ_REQUIRE(t && c, AGZ_E_INVALID, "agz_trainer_set_adam: NULL argument");
  AGZ_REQUIRE(adam_conf_valid(c), AGZ_E_INVALID, "agz_trainer_set_adam: need 0 <= beta1 < 1, 0 <= beta2 < 1, eps > 0, all finite, on = 0 / 1 (got %g, %g, %g, %d)",
              (double)c->beta1, (double)c->beta2, (double)c->eps, (int)c->on);
  AGZ_REQUIRE(!(c->on && t->solver.momentum != 0.f), AGZ_E_STATE,
              "agz_trainer_set_adam: Adam and a momentum exclude each other (set the momentum to 0 first: agz_trainer_set_solver)");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  if (c->on && !t->M1) {
    const size_t bytes = t->n_flat * sizeof(float);
    float* m1 = nullptr; float* m2 = nullptr;
    if (hipMalloc(&m1, bytes) != hipSuccess || hipMalloc(&m2, bytes) != hipSuccess) {
      (void)hipGetLastError();
      if (m1) hipFree(m1);
      agz::set_error("agz_trainer_set_adam: out of device memory for the moments (2 x %zu bytes)", bytes);
      return AGZ_E_NOMEM;
    }
    if (hipMemsetAsync(m1, 0, bytes, t->ctx->stream) != hipSuccess || hipMemsetAsync(m2, 0, bytes, t->ctx->stream) != hipSuccess ||
        hipStreamSynchronize(t->ctx->stream) != hipSuccess) {
      hipFree(m1); hipFree(m2);
      agz::set_error("agz_trainer_set_adam: clearing the moments failed");
      return AGZ_E_HIP;
    }
    t->M1 = m1; t->M2 = m2; t->adam_t = 0;
  } else if (!c->on && t->M1) {
    AGZ_HIP_TRY(hipFree(t->M1)); t->M1 = nullptr;
    AGZ_HIP_TRY(hipFree(t->M2)); t->M2 = nullptr;
    t->adam_t = 0;
  }
  t->adam = *c;
  return AGZ_OK;
}
int agz_trainer_get_adam(const agz_trainer* t, agz_adam_conf* out, uint64_t* step) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_get_adam: NULL trainer");
  if (out) *out = t->adam;
  if (step) *step = t->adam_t;
  return AGZ_OK;
}
int agz_trainer_get_moments(const agz_trainer* t, int i, float* m, float* v, size_t n) {
  AGZ_REQUIRE(t && m && v, AGZ_E_INVALID, "agz_trainer_get_moments: NULL argument");
  AGZ_REQUIRE(i >= 0 && i < (int)t->prefs.size() && n >= pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_get_moments: bad argument");
  if (!t->M1) {   // (Adam off: no moments)
    std::fill(m, m + pref_size(t->prefs[i]), 0.f); std::fill(v, v + pref_size(t->prefs[i]), 0.f);
    return AGZ_OK;
  }
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  int r = xfer_param(t, t->M1, i, m, 1);
  return r != AGZ_OK ? r : xfer_param(t, t->M2, i, v, 1);
}
int agz_trainer_set_moments(agz_trainer* t, int i, const float* m, const float* v, size_t n) {
  AGZ_REQUIRE(t && m && v, AGZ_E_INVALID, "agz_trainer_set_moments: NULL argument");
  AGZ_REQUIRE(i >= 0 && i < (int)t->prefs.size(), AGZ_E_INVALID, "agz_trainer_set_moments: bad index");
  AGZ_REQUIRE(n == pref_size(t->prefs[i]), AGZ_E_INVALID, "agz_trainer_set_moments(%s): need %zu floats, got %zu", t->prefs[i].name.c_str(), pref_size(t->prefs[i]), n);
  AGZ_REQUIRE(t->M1, AGZ_E_STATE, "agz_trainer_set_moments: the trainer has no moments (turn Adam on first: agz_trainer_set_adam)");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  int r = xfer_param(t, t->M1, i, const_cast<float*>(m), 0);
  return r != AGZ_OK ? r : xfer_param(t, t->M2, i, const_cast<float*>(v), 0);
}

// A sharded trainer draws its rows' slice of the GLOBAL tensors: the stream position of its first element, the Glorot deviation of the
// global shape — bit for bit those rows of a plain trainer's init_random(seed) at the global batch.
int agz_trainer_init_random(agz_trainer* t, uint64_t seed) {  // same recipe as agz_net_init_random over the FULL shapes
  AGZ_REQUIRE(t, AGZ_E_INVALID, "trainer is NULL");
  // SplitMix64 is counter based (state_n = seed + n * golden), so the sequential stream of the oracle's initialiser can be
  // generated in parallel: the batch-shaped gamma/beta of a 19x19, K=256, B=256 trainer are 1.9 G normals (37 s on one core).
  const uint64_t GOLD = 0x9E3779B97F4A7C15ull;
  uint64_t draws = 0;   // draws consumed so far
  unsigned nthr = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
  for (int i = 0; i < (int)t->prefs.size(); i++) {
    const TParamRef& p = t->prefs[i];
    std::vector<float> v(pref_size(p));
    // this rank's slice: elements [g0, g0 + v.size()) of a tensor of n elements.  A tied trainer draws row 0 of the BatchSize rows a plain
    // trainer draws (the same stream positions, the Glorot deviation of the batch-shaped tensor): the slice of "rank 0 of B"
    // (a tied sharded trainer draws that row at the GLOBAL batch, whole and the same on every rank)
    const int nr = pref_batch_shaped(p) ? (t->tied ? t->B * t->n_ranks : t->n_ranks) : 1;
    double field = 1; for (size_t k = 2; k < p.shape.size(); k++) field *= p.shape[k];
    const double stdev = std::sqrt(2.0 / ((double)(p.shape[0] * nr + p.shape[1]) * field));
    const size_t n = v.size() * nr, g0 = v.size() * (nr > 1 && !t->tied ? t->rank : 0);
    const uint64_t d0 = draws;
    if (p.kind == 0) {           // GlorotU: one draw per element
      const double lim = stdev * std::sqrt(3.0);
      auto work = [&](size_t lo, size_t hi) {
        SplitMix64 r(seed + (d0 + g0 + lo) * GOLD);
        for (size_t k = lo; k < hi; k++) v[k] = (float)((r.float64() * 2.0 - 1.0) * lim);
      };
      if (n < (1u << 16)) work(0, n);   // (filters are shared: n = v.size())
      else {
        std::vector<std::thread> th;
        size_t per = (n + nthr - 1) / nthr;
        for (unsigned q = 0; q < nthr; q++) { size_t lo = q * per, hi = std::min(n, lo + per); if (lo < hi) th.emplace_back(work, lo, hi); }
        for (auto& x : th) x.join();
      }
      draws += n;
    } else if (p.kind == 1 || p.kind == 2) {   // GlorotN by Box-Muller: two draws per PAIR of elements
      const size_t pairs = (n + 1) / 2, e1 = g0 + v.size();
      const size_t p0 = g0 / 2, p1 = (e1 + 1) / 2;   // the pairs this rank's elements fall in (a slice may start or end mid-pair)
      auto work = [&](size_t lo, size_t hi) {   // pair indices, relative to p0
        SplitMix64 r(seed + (d0 + 2 * (p0 + lo)) * GOLD);
        for (size_t q = p0 + lo; q < p0 + hi; q++) {
          double u1 = 1.0 - r.float64(), u2 = r.float64();
          double rad = std::sqrt(-2.0 * std::log(u1)), th = 6.283185307179586476925 * u2;
          if (2 * q >= g0) v[2 * q - g0] = (float)(rad * std::cos(th) * stdev);
          if (2 * q + 1 < e1) v[2 * q + 1 - g0] = (float)(rad * std::sin(th) * stdev);
        }
      };
      const size_t np = p1 - p0;
      if (np < (1u << 15)) work(0, np);
      else {
        std::vector<std::thread> th;
        size_t per = (np + nthr - 1) / nthr;
        for (unsigned q = 0; q < nthr; q++) { size_t lo = q * per, hi = std::min(np, lo + per); if (lo < hi) th.emplace_back(work, lo, hi); }
        for (auto& x : th) x.join();
      }
      draws += 2 * pairs;
    }
    int rc = agz_trainer_set_param(t, i, v.data(), v.size());
    if (rc != AGZ_OK) return rc;
  }
  return AGZ_OK;
}

int agz_trainer_forward_backward(agz_trainer* t, const float* planes, const float* pi, const float* v, float* cost) {
  AGZ_REQUIRE(t && planes && pi && v, AGZ_E_INVALID, "agz_trainer_forward_backward: NULL argument");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  hipStream_t s = t->ctx->stream;
  AGZ_HIP_TRY(hipMemcpyAsync(t->d_planes, planes, (size_t)t->B * t->F * t->g.HW * 4, hipMemcpyHostToDevice, s));
  AGZ_HIP_TRY(hipMemcpyAsync(t->d_pi, pi, (size_t)t->B * t->A * 4, hipMemcpyHostToDevice, s));
  AGZ_HIP_TRY(hipMemcpyAsync(t->d_v, v, (size_t)t->B * 4, hipMemcpyHostToDevice, s));
  int r = t->step(t->d_planes, t->d_pi, t->d_v);
  if (r != AGZ_OK) return r;
  float c[2] = {0, 0};
  AGZ_HIP_TRY(hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, s));
  AGZ_HIP_TRY(hipStreamSynchronize(s));
  if (cost) *cost = c[0] + c[1];
  return AGZ_OK;
}

// forward_backward on DEVICE buffers (a batch sliced out of agz_examples_tensors_dev): no staging copy
int agz_trainer_forward_backward_dev(agz_trainer* t, const float* planes_dev, const float* pi_dev, const float* v_dev, float* cost) {
  AGZ_REQUIRE(t && planes_dev && pi_dev && v_dev, AGZ_E_INVALID, "agz_trainer_forward_backward_dev: NULL argument");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  int r = t->step(planes_dev, pi_dev, v_dev);
  if (r != AGZ_OK) return r;
  if (cost) {
    float c[2] = {0, 0};
    AGZ_HIP_TRY(hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, t->ctx->stream));
    AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    *cost = c[0] + c[1];
  }
  return AGZ_OK;
}

// solver.Step with options (agz_trainer_set_solver): the regions the vanilla step sweeps with k_axpy, through k_solver_sweep
static int apply_solver(agz_trainer* t, float lr, float grad_scale) {
  const agz_solver_conf& sc = t->solver;
  const bool mom = sc.momentum != 0.f, adam = t->adam.on != 0;
  if (adam) t->adam_t++;   // one count per solver step: the fused kernels of this step were given the same value
  const AdamK ak = adam ? t->adam_k(t->adam_t) : AdamK{};
  hipStream_t s = t->ctx->stream;
  auto sweep = [&](size_t off, size_t n) {   // (every region starts and ends on a multiple of four floats: take() in agz_trainer_create)
    const size_t n4 = n / 4;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(nblk(n4), (size_t)t->ctx->num_cus * 8));
    if (adam) hipLaunchKernelGGL(k_solver_sweep<SK_ADAM>, dim3(grid), dim3(256), 0, s, t->P + off, t->G + off, t->M1 + off, n4, lr, grad_scale, 0.f, sc.l2reg, sc.clip, t->M2 + off, ak);
    else if (mom) hipLaunchKernelGGL(k_solver_sweep<SK_MOMENTUM>, dim3(grid), dim3(256), 0, s, t->P + off, t->G + off, t->V + off, n4, lr, grad_scale, sc.momentum, sc.l2reg, sc.clip, (float*)nullptr, ak);
    else hipLaunchKernelGGL(k_solver_sweep<SK_OPTIONS>, dim3(grid), dim3(256), 0, s, t->P + off, t->G + off, (float*)nullptr, n4, lr, grad_scale, sc.momentum, sc.l2reg, sc.clip, (float*)nullptr, ak);
  };
  if (t->fused_done) {   // k_bn_bwd1<SK_OPTIONS / SK_MOMENTUM / SK_ADAM> stepped the tower's gamma / beta and their velocity: the filters and the head region remain
    AGZ_REQUIRE(grad_scale == 1.0f, AGZ_E_STATE, "agz_trainer_apply: a fused step takes no gradient scale");
    for (const auto& ly : t->layers) sweep(ly.o_wf, (size_t)9 * ly.Cout_p * ly.Cin_p);
    sweep(t->o_hc, t->n_flat - t->o_hc);
    t->fused_done = false;
  } else if (t->tied) {
    // the tower's tied gamma / beta through tied_step, the code the fused owner runs (k_bn_bwd1_tied): both paths give the same bits
    auto tsweep = [&](size_t off, size_t n) {
      const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(nblk(n), (size_t)t->ctx->num_cus * 8));
      if (adam) hipLaunchKernelGGL(k_tied_sweep<SK_ADAM>, dim3(grid), dim3(256), 0, s, t->P + off, t->G + off, t->M1 + off, t->M2 + off, n, lr, grad_scale, 0.f, sc.l2reg, sc.clip, ak);
      else if (mom) hipLaunchKernelGGL(k_tied_sweep<SK_MOMENTUM>, dim3(grid), dim3(256), 0, s, t->P + off, t->G + off, t->V + off, (float*)nullptr, n, lr, grad_scale, sc.momentum, sc.l2reg, sc.clip, ak);
      else hipLaunchKernelGGL(k_tied_sweep<SK_OPTIONS>, dim3(grid), dim3(256), 0, s, t->P + off, t->G + off, (float*)nullptr, (float*)nullptr, n, lr, grad_scale, sc.momentum, sc.l2reg, sc.clip, ak);
    };
    const int L = (int)t->layers.size() - 1;
    for (int l = 0; l <= L; l++) {
      const TLayer& ly = t->layers[l];
      sweep(ly.o_wf, (size_t)9 * ly.Cout_p * ly.Cin_p);
      tsweep(ly.o_gamma, (l < L ? t->layers[l + 1].o_wf : t->o_hc) - ly.o_gamma);   // [gamma | beta], contiguous
    }
    sweep(t->o_hc, t->n_flat - t->o_hc);
  } else
    sweep(0, t->n_flat);
  AGZ_HIP_TRY(hipGetLastError());
  return AGZ_OK;
}

int agz_trainer_apply(agz_trainer* t, float lr, float grad_scale) {  // solver.Step (meta.go:40): w -= lr * grad
  AGZ_REQUIRE(t, AGZ_E_INVALID, "trainer is NULL");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  if (t->solver_on() || t->adam.on) return apply_solver(t, lr, grad_scale);
  if (t->fused_done) {
    // the backward that just ran stepped the tower's gamma / beta itself (k_bn_bwd1): the filters of every layer and the head region remain
    AGZ_REQUIRE(grad_scale == 1.0f, AGZ_E_STATE, "agz_trainer_apply: a fused step takes no gradient scale");
    for (const auto& ly : t->layers) {
      const size_t n = (size_t)9 * ly.Cout_p * ly.Cin_p;
      hipLaunchKernelGGL(k_axpy, dim3(nblk(n)), dim3(256), 0, t->ctx->stream, t->P + ly.o_wf, t->G + ly.o_wf, -lr, n);
    }
    const size_t nh = t->n_flat - t->o_hc;
    hipLaunchKernelGGL(k_axpy, dim3(nblk(nh)), dim3(256), 0, t->ctx->stream, t->P + t->o_hc, t->G + t->o_hc, -lr, nh);
    t->fused_done = false;
  } else {
    hipLaunchKernelGGL(k_axpy, dim3(nblk(t->n_flat)), dim3(256), 0, t->ctx->stream, t->P, t->G, -lr * grad_scale, t->n_flat);
  }
  AGZ_HIP_TRY(hipGetLastError());
  return AGZ_OK;
}

int agz_trainer_batch(agz_trainer* t, const float* planes, const float* pi, const float* v, float lr, float* cost) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "trainer is NULL");
  t->fuse_lr = lr;                                   // lr = 0 (a dry step): the plain path, gradients materialised
  int r = agz_trainer_forward_backward(t, planes, pi, v, cost);
  t->fused_done = r == AGZ_OK && t->fuse_lr != 0.f;
  t->fuse_lr = 0.f;
  if (r != AGZ_OK) return r;
  r = agz_trainer_apply(t, lr, 1.0f);
  if (r != AGZ_OK) return r;
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  return AGZ_OK;
}

// AGZ_COMPUTE_F32_MFMA (default); AGZ_COMPUTE_BF16X3: forward, data-gradient and weight-gradient GEMMs on the bf16 pipe;
// AGZ_COMPUTE_WINO_H2: the data-gradient convolutions of the dual blocks through the Winograd fp16x2 path (weights transformed on
// the device every step), everything else as in BF16X3.  Same gradient tolerance against the oracle in all modes.
int agz_trainer_set_compute_mode(agz_trainer* t, int mode) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "trainer is NULL");
  const bool force = (mode & AGZ_COMPUTE_FORCE) != 0;
  mode &= ~AGZ_COMPUTE_FORCE;
  AGZ_REQUIRE(mode == AGZ_COMPUTE_F32_MFMA || mode == AGZ_COMPUTE_BF16X3 || mode == AGZ_COMPUTE_WINO_H2, AGZ_E_INVALID, "agz_trainer_set_compute_mode: mode %d not available for training", mode);
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  t->x3_force = force;
  if (mode == AGZ_COMPUTE_BF16X3 || mode == AGZ_COMPUTE_WINO_H2)
    for (auto& ly : t->layers)
      if (!ly.w3f) {
        int r = t->alloc(&ly.w3f, w3_elems(ly.Cout_p, ly.Cin_p));
        if (r == AGZ_OK) r = t->alloc(&ly.w3t, w3_elems(ly.Cin_p, ly.Cout_p));
        if (r != AGZ_OK) return r;
      }
  t->x3 = mode == AGZ_COMPUTE_BF16X3 || mode == AGZ_COMPUTE_WINO_H2;
  t->wino = mode == AGZ_COMPUTE_WINO_H2;
  return AGZ_OK;
}

int agz_trainer_set_dma_forward(agz_trainer* t, int on) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "trainer is NULL");
  t->dma_fwd = (on & 1) != 0;
  t->fast_heads = (on & 4) == 0;      // bit 2: the FIRST form of the head kernels (A/B)
  t->conv3_mode = (on >> 6) & 3;
  t->conv3 = (on & 32) == 0;          // bit 5: the forward DMA convolution with one tap per K step (k_conv_h2dma) (A/B)
  t->one_stream = (on & 16) != 0;     // bit 4: everything on the step's stream (diagnostic)
  t->hoist_w = (on & 8) == 0;         // bit 3: weight images per layer in line, not at the start of the step on the side stream (A/B)
  t->wg_pad_lds = (on & 256) ? 0 : 16384;   // bit 8: k_wgrad_h2t3 at two workgroups per CU as in round 5 (default: one, 73.7 KB static + 16 KB dynamic LDS)
  t->wg_low_prio = (on & 512) != 0;     // bit 9: the side stream at the lowest priority (before the first step)
  return AGZ_OK;
}

// The loss kind (agz.h).  Local on a sharded handle: every rank sets the same.
int agz_trainer_set_loss(agz_trainer* t, int kind) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_set_loss: NULL trainer");
  AGZ_REQUIRE(kind == AGZ_LOSS_REFERENCE || kind == AGZ_LOSS_ALPHAZERO, AGZ_E_INVALID, "agz_trainer_set_loss: unknown loss kind %d", kind);
  if (kind == AGZ_LOSS_ALPHAZERO && !t->az_row) {
    AGZ_REQUIRE(t->A <= 512, AGZ_E_UNSUPPORTED, "agz_trainer_set_loss: the loss kernel holds a row of at most 512 logits (ActionSpace %d)", t->A);
    AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
    int r = AGZ_OK;
    if (!t->az_dz) r = t->alloc(&t->az_dz, (size_t)t->B * t->A);
    if (r == AGZ_OK && !t->az_do) r = t->alloc(&t->az_do, (size_t)t->B);
    if (r == AGZ_OK) r = t->alloc(&t->az_row, (size_t)t->B * 2);
    if (r != AGZ_OK) return r;
    AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  }
  t->loss_kind = kind;
  return AGZ_OK;
}
int agz_trainer_get_loss(const agz_trainer* t, int* kind) {
  AGZ_REQUIRE(t && kind, AGZ_E_INVALID, "agz_trainer_get_loss: NULL argument");
  *kind = t->loss_kind;
  return AGZ_OK;
}
int agz_trainer_get_costs(agz_trainer* t, float* policy, float* value) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_get_costs: NULL trainer");
  AGZ_REQUIRE(t->cost_valid, AGZ_E_STATE, "agz_trainer_get_costs: no forward pass has run yet");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  float c[2] = {0, 0};
  AGZ_HIP_TRY(hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, t->ctx->stream));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  if (policy) *policy = c[0];
  if (value) *value = c[1];
  return AGZ_OK;
}

int agz_trainer_last_paths(agz_trainer* t, int layer, int* fwd, int* wgrad, int* dgrad, int* bn_bwd2) {
  AGZ_REQUIRE(t && fwd && wgrad && dgrad && bn_bwd2, AGZ_E_INVALID, "agz_trainer_last_paths: NULL argument");
  AGZ_REQUIRE(layer >= 0 && layer <= t->L, AGZ_E_INVALID, "agz_trainer_last_paths: layer %d of 0..%d", layer, t->L);
  const TLayer& ly = t->layers[layer];
  *fwd = ly.path_fwd; *wgrad = ly.path_wgrad; *dgrad = ly.path_dgrad; *bn_bwd2 = ly.path_bn2;
  return AGZ_OK;
}

int agz_trainer_last_rows(agz_trainer* t, int layer, int32_t out[8]) {
  AGZ_REQUIRE(t && out, AGZ_E_INVALID, "agz_trainer_last_rows: NULL argument");
  AGZ_REQUIRE(layer >= 0 && layer <= t->L + 1, AGZ_E_INVALID, "agz_trainer_last_rows: layer %d of 0..%d", layer, t->L + 1);
  const int* src = layer <= t->L ? t->layers[layer].rows : t->head_rows;
  for (int i = 0; i < 8; i++) out[i] = src[i];
  return AGZ_OK;
}

int agz_trainer_last_planes(agz_trainer* t, int layer, int* fused, uint32_t* est_bits, uint32_t* range_bits) {
  AGZ_REQUIRE(t && fused && est_bits && range_bits, AGZ_E_INVALID, "agz_trainer_last_planes: NULL argument");
  AGZ_REQUIRE(layer >= 0 && layer <= t->L, AGZ_E_INVALID, "agz_trainer_last_planes: layer %d of 0..%d", layer, t->L);
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // (the step's last kernels; the side stream was joined into it by the step)
  if (t->wg_stream) AGZ_HIP_TRY(hipStreamSynchronize(t->wg_stream));
  unsigned w[2] = {0u, 0u};
  AGZ_HIP_TRY(hipMemcpy(&w[0], t->amax_prev + 2 * layer + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  AGZ_HIP_TRY(hipMemcpy(&w[1], t->amax_words + 2 * layer + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  *fused = t->planes_fused[layer] && t->layers[layer].x_planes ? 1 : 0;
  *est_bits = w[0]; *range_bits = w[1];
  return AGZ_OK;
}

int agz_trainer_grads_dev(agz_trainer* t, float** dev_ptr, size_t* n_floats) {
  AGZ_REQUIRE(t && dev_ptr && n_floats, AGZ_E_INVALID, "NULL argument");
  *dev_ptr = t->G; *n_floats = t->n_flat;
  return AGZ_OK;
}

// the learn rate dual.Train builds its solver with: gorgonia.NewVanillaSolver(gorgonia.WithLearnRate(0.1)) (dualnet/meta.go:22)
static constexpr float DUAL_TRAIN_LR = 0.1f;

// dual.Train (dualnet/meta.go:16-54): iterations x batches of BatchSize rows; shuffleBatch (meta.go:57-102) after every
// iteration with the build's SplitMix64 (Fisher-Yates j = r.Intn(i+1) pattern).  Xs/policies/values are shuffled IN PLACE
// like the reference does.
int agz_train(agz_trainer* t, float* Xs, float* policies, float* values, int batches, int iterations, uint64_t seed, float* last_cost) {
  AGZ_REQUIRE(t && Xs && policies && values && batches >= 1 && iterations >= 0, AGZ_E_INVALID, "agz_train: bad argument");
  // (sharded: the tensors are the GLOBAL examples, the same on every rank; batch b is rows [b * Bg, (b + 1) * Bg), this rank trains its
  // own rows of it, and every rank shuffles the whole set with the same stream)
  const size_t xs = (size_t)t->F * t->g.HW, ps = (size_t)t->A, Bg = (size_t)t->B * t->n_ranks;
  const size_t n = (size_t)batches * Bg;
  SplitMix64 rng(seed);
  std::vector<float> tmp(std::max(xs, ps));
  float c = 0;
  for (int it = 0; it < iterations; it++) {
    for (int b = 0; b < batches; b++) {
      size_t s0 = (size_t)b * Bg + (size_t)t->rank * t->B;
      int r = agz_trainer_batch(t, Xs + s0 * xs, policies + s0 * ps, values + s0, DUAL_TRAIN_LR, &c);
      if (r != AGZ_OK) return r;
    }
    for (size_t i = 0; i < n; i++) {
      size_t j = (size_t)(rng.next() % (uint64_t)(i + 1));
      if (j == i) continue;
      memcpy(tmp.data(), Xs + i * xs, xs * 4); memcpy(Xs + i * xs, Xs + j * xs, xs * 4); memcpy(Xs + j * xs, tmp.data(), xs * 4);
      memcpy(tmp.data(), policies + i * ps, ps * 4); memcpy(policies + i * ps, policies + j * ps, ps * 4); memcpy(policies + j * ps, tmp.data(), ps * 4);
      std::swap(values[i], values[j]);
    }
  }
  if (last_cost) *last_cost = c;
  return AGZ_OK;
}

// one batch of dual.Train's loop (meta.go:33-40) on the trainer's own batch buffers, already filled on its stream: the fused step at
// dual.Train's learn rate, then the solver on what the backward did not step itself.  Nothing is synchronised.  `filled`: the status of
// what filled the buffers (agz_trainer::step's `pre`).
static int train_step_on_batch(agz_trainer* t, int filled = AGZ_OK) {
  t->fuse_lr = DUAL_TRAIN_LR;
  int rc = t->step(t->d_planes, t->d_pi, t->d_v, filled);
  t->fused_done = rc == AGZ_OK;
  t->fuse_lr = 0.f;
  if (rc == AGZ_OK) rc = agz_trainer_apply(t, DUAL_TRAIN_LR, 1.0f);
  return rc;
}

// dual.Train over DEVICE tensors (Xs [rows,F,H,W], policies [rows,A], values [rows], rows = batches*BatchSize — e.g.
// agz_examples_tensors_dev).  Same loop and the same shuffleBatch stream as agz_train, but the shuffle permutes a row
// index (4 B/row) instead of swapping rows, each batch is gathered device to device, and the cost is read back once at
// the end — no host round trip of the examples and no per-batch synchronisation.  The device tensors are left unchanged.
int agz_train_dev(agz_trainer* t, const float* Xs_dev, const float* policies_dev, const float* values_dev, int batches, int iterations,
                  uint64_t seed, float* last_cost) {
  AGZ_REQUIRE(t && Xs_dev && policies_dev && values_dev && batches >= 1 && iterations >= 0, AGZ_E_INVALID, "agz_train_dev: bad argument");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  hipStream_t s = t->ctx->stream;
  const size_t xs = (size_t)t->F * t->g.HW, ps = (size_t)t->A, Bg = (size_t)t->B * t->n_ranks;   // (sharded: as agz_train)
  const size_t n = (size_t)batches * Bg;
  std::vector<int32_t> perm(n);
  for (size_t i = 0; i < n; i++) perm[i] = (int32_t)i;
  int32_t* d_perm = nullptr;
  const hipError_t em = hipMalloc(&d_perm, n * 4);
  if (t->sharded) {   // (every rank agrees before the first collective step: none may stay out of a step its peers enter)
    if (em != hipSuccess) agz::set_error("agz_train_dev: %s", hipGetErrorString(em));
    const int a = t->shard.agree(em == hipSuccess ? AGZ_OK : AGZ_E_NOMEM);
    if (a != AGZ_OK) { if (em == hipSuccess) hipFree(d_perm); return a; }
  } else
    AGZ_HIP_TRY(em);
  SplitMix64 rng(seed);
  int rc = AGZ_OK;
  for (int it = 0; it < iterations && rc == AGZ_OK; it++) {
    hipError_t e = hipMemcpyAsync(d_perm, perm.data(), n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // perm is reshuffled on the host below
    if (e != hipSuccess) { agz::set_error("agz_train_dev: %s", hipGetErrorString(e)); rc = AGZ_E_HIP; break; }
    for (int b = 0; b < batches && rc == AGZ_OK; b++) {
      const int32_t* ib = d_perm + (size_t)b * Bg + (size_t)t->rank * t->B;
      hipLaunchKernelGGL(k_gather_rows_t, dim3(nblk((size_t)t->B * xs)), dim3(256), 0, s, Xs_dev, ib, t->d_planes, (int)xs, (size_t)t->B * xs);
      hipLaunchKernelGGL(k_gather_rows_t, dim3(nblk((size_t)t->B * ps)), dim3(256), 0, s, policies_dev, ib, t->d_pi, (int)ps, (size_t)t->B * ps);
      hipLaunchKernelGGL(k_gather_rows_t, dim3(nblk((size_t)t->B)), dim3(256), 0, s, values_dev, ib, t->d_v, 1, (size_t)t->B);
      rc = train_step_on_batch(t);
    }
    for (size_t i = 0; i < n; i++) {  // shuffleBatch (meta.go:57-102) on the row index
      size_t j = (size_t)(rng.next() % (uint64_t)(i + 1));
      std::swap(perm[i], perm[j]);
    }
  }
  float c[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d_perm);
  if (rc != AGZ_OK) return rc;
  AGZ_HIP_TRY(e);
  if (last_cost) *last_cost = iterations > 0 ? c[0] + c[1] : 0.f;
  return AGZ_OK;
}

// dual.Train's loop over minibatches SAMPLED from a replay window (replay.hip; BUILD EXTENSION, DESIGN.md §2 replay-window): step s of the
// run draws the trainer's BatchSize rows with replay::draw(seed, s, BatchSize, r, n, symmetric) straight into the trainer's batch buffers
// (one k_replay_sample launch where agz_train_dev has three gathers) and takes the step agz_train_dev takes per batch.  n is read once, at
// entry; nothing is uploaded and nothing waited for between steps; the cost is read back once at the end.
int agz_train_replay(agz_trainer* t, agz_replay* rp, int steps, uint64_t seed, int symmetric, float* last_cost) {
  AGZ_REQUIRE(t && rp && steps >= 0, AGZ_E_INVALID, "agz_train_replay: bad argument");
  AGZ_REQUIRE(!t->sharded, AGZ_E_UNSUPPORTED,
              "agz_train_replay: a sharded trainer trains from a replay window through the collective agz_train_replay_sharded");
  const agz::ReplayInfo w = agz::replay_info(rp);
  AGZ_REQUIRE(w.ctx == t->ctx, AGZ_E_INVALID, "agz_train_replay: the trainer and the window belong to different contexts");
  AGZ_REQUIRE(w.F == t->conf.Features && w.H == t->conf.Height && w.W == t->conf.Width && w.A1 == t->conf.ActionSpace, AGZ_E_INVALID,
              "agz_train_replay: the window's rows are [%d, %d, %d] + %d, the trainer's [%d, %d, %d] + %d", w.F, w.H, w.W, w.A1,
              t->conf.Features, t->conf.Height, t->conf.Width, t->conf.ActionSpace);
  int rc = agz::replay_check_symmetric(rp, symmetric, "agz_train_replay");
  if (rc != AGZ_OK) return rc;
  AGZ_REQUIRE(w.ring_total > 0, AGZ_E_STATE, "agz_train_replay: the window is empty");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  hipStream_t s = t->ctx->stream;
  const uint64_t n = w.ring_total < w.cap ? w.ring_total : w.cap;
  for (int st = 0; st < steps && rc == AGZ_OK; st++) {
    rc = agz::replay_sample_launch(rp, t->B, 0, t->B, seed, (uint64_t)st, symmetric, n, w.ring_total, t->d_planes, t->d_pi, t->d_v);
    if (rc == AGZ_OK) rc = train_step_on_batch(t);
  }
  float c[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (rc != AGZ_OK) return rc;
  AGZ_HIP_TRY(e);
  if (last_cost) *last_cost = steps > 0 ? c[0] + c[1] : 0.f;
  return AGZ_OK;
}

// agz_train_replay on a SHARDED trainer (DESIGN.md §2 replay-sharded): collective.  Every rank holds a replica of the window; step s trains
// on minibatch s of n_ranks * B rows, of which this rank draws rows [rank * B, (rank + 1) * B) itself — replay::draw is a pure function of
// the global row index, so nothing is exchanged for the draw and the step's collectives are those of agz_train_dev's step.  Entry: the local
// checks, shard.agree on them, then ONE all-gather of {total, capacity, live, packed, digest} (digest: agz_replay_digest if verify, else
// 0); any difference from rank 0's tuple is AGZ_E_STATE on every rank and nothing is changed.
int agz_train_replay_sharded(agz_trainer* t, agz_replay* rp, int steps, uint64_t seed, int symmetric, int verify, float* last_cost) {
  AGZ_REQUIRE(t && rp && steps >= 0, AGZ_E_INVALID, "agz_train_replay_sharded: bad argument");
  AGZ_REQUIRE(t->sharded, AGZ_E_STATE,
              "agz_train_replay_sharded: not a sharded trainer (agz_trainer_create_sharded / _sharded_tied); agz_train_replay trains this one");
  const agz::ReplayInfo w = agz::replay_info(rp);
  const uint64_t n = w.ring_total < w.cap ? w.ring_total : w.cap;
  // the local checks of agz_train_replay, then the window's digest; whatever they give, this rank enters the two exchanges below
  auto local = [&]() -> int {
    AGZ_REQUIRE(w.ctx == t->ctx, AGZ_E_INVALID, "agz_train_replay_sharded: the trainer and the window belong to different contexts");
    AGZ_REQUIRE(w.F == t->conf.Features && w.H == t->conf.Height && w.W == t->conf.Width && w.A1 == t->conf.ActionSpace, AGZ_E_INVALID,
                "agz_train_replay_sharded: the window's rows are [%d, %d, %d] + %d, the trainer's [%d, %d, %d] + %d", w.F, w.H, w.W, w.A1,
                t->conf.Features, t->conf.Height, t->conf.Width, t->conf.ActionSpace);
    const int r = agz::replay_check_symmetric(rp, symmetric, "agz_train_replay_sharded");
    if (r != AGZ_OK) return r;
    AGZ_REQUIRE(w.ring_total > 0, AGZ_E_STATE, "agz_train_replay_sharded: the window is empty");
    AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
    return AGZ_OK;
  };
  uint64_t mine[5] = {w.ring_total, w.cap, n, w.packed ? 1u : 0u, 0};
  int rc = local();
  if (rc == AGZ_OK && verify) rc = agz_replay_digest(rp, &mine[4]);
  uint64_t* d = nullptr;   // [n_ranks][5] gathered tuples, then this rank's
  const size_t nr = (size_t)t->n_ranks;
  if (rc == AGZ_OK && hipMalloc(&d, (nr + 1) * sizeof(mine)) != hipSuccess) {
    (void)hipGetLastError();
    d = nullptr;
    agz::set_error("agz_train_replay_sharded: out of device memory for the window check");
    rc = AGZ_E_NOMEM;
  }
  rc = t->shard.agree(rc);
  if (rc != AGZ_OK) { if (d) hipFree(d); return rc; }
  std::vector<uint64_t> all(nr * 5);
  if (hipMemcpy(d + nr * 5, mine, sizeof(mine), hipMemcpyHostToDevice) != hipSuccess) rc = AGZ_E_HIP;
  const int g = t->shard.allgather_bytes(d + nr * 5, d, sizeof(mine));
  if (rc == AGZ_OK) rc = g;
  if (rc == AGZ_OK && hipMemcpy(all.data(), d, all.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = AGZ_E_HIP;
  hipFree(d);
  if (rc == AGZ_E_HIP) agz::set_error("agz_train_replay_sharded: the exchange of the window check failed");
  rc = t->shard.agree(rc);
  if (rc != AGZ_OK) return rc;
  // (every rank holds the same gathered tuples, so every rank takes the same branch here)
  static const char* const FIELD[5] = {"total", "capacity", "live", "the packed flag", "the digest"};
  for (size_t r = 1; r < nr; r++)
    for (int f = 0; f < 5; f++)
      AGZ_REQUIRE(all[r * 5 + f] == all[f], AGZ_E_STATE,
                  "agz_train_replay_sharded: the windows differ: rank %zu holds %s %llu (0x%llx), rank 0 holds %llu (0x%llx); nothing was trained",
                  r, FIELD[f], (unsigned long long)all[r * 5 + f], (unsigned long long)all[r * 5 + f], (unsigned long long)all[f],
                  (unsigned long long)all[f]);
  hipStream_t s = t->ctx->stream;
  const int Bg = t->B * t->n_ranks, row0 = t->rank * t->B;
  for (int st = 0; st < steps && rc == AGZ_OK; st++) {
    // (a rank whose sampler launch fails still enters the step's collectives: its error travels in the step's status word)
    const int filled = agz::replay_sample_launch(rp, Bg, row0, t->B, seed, (uint64_t)st, symmetric, n, w.ring_total, t->d_planes, t->d_pi, t->d_v);
    rc = train_step_on_batch(t, filled);
  }
  float c[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (rc != AGZ_OK) return rc;
  AGZ_HIP_TRY(e);
  if (last_cost) *last_cost = steps > 0 ? c[0] + c[1] : 0.f;
  return AGZ_OK;
}

// ---- running BatchNorm statistics (BnTrack above; include/agz.h) --------------------------------------------------------------------------
using agz::ckpt::bn_momentum_valid;
// the whole state on the host (a few KB to a few hundred KB); empty while none exists
static int bn_download(const agz_trainer* t, std::vector<double>& h) {
  h.assign(t->bn_total, 0.0);
  if (!t->bn_st) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  AGZ_HIP_TRY(hipMemcpy(h.data(), t->bn_st, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  return AGZ_OK;
}
static int bn_upload(agz_trainer* t, const std::vector<double>& h) {
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  AGZ_HIP_TRY(hipMemcpy(t->bn_st, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return AGZ_OK;
}
static void bn_estimates(const agz_trainer* t, const std::vector<double>& h, int i, float* mean, float* var) {
  const agz_trainer::BnOp op = t->bn_op(i);
  const double n = h[op.n];
  for (int c = 0; c < op.C; c++) { mean[c] = (float)(h[op.mean + c] / n); var[c] = (float)(h[op.var + c] / n); }
}

int agz_trainer_set_bn_tracking(agz_trainer* t, int on, float momentum) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_set_bn_tracking: NULL trainer");
  AGZ_REQUIRE((on == 0 || on == 1) && bn_momentum_valid(momentum), AGZ_E_INVALID,
              "agz_trainer_set_bn_tracking: need on = 0 / 1 and a finite 0 <= momentum < 1 (got %d, %g)", on, (double)momentum);
  if (on) {
    AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
    int r = t->bn_alloc();
    if (r != AGZ_OK) return r;
  }
  t->bn_on = on != 0; t->bn_lam = momentum;
  return AGZ_OK;
}
int agz_trainer_get_bn_tracking(const agz_trainer* t, int* on, float* momentum, double* weight) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_get_bn_tracking: NULL trainer");
  if (on) *on = t->bn_on ? 1 : 0;
  if (momentum) *momentum = t->bn_lam;
  if (weight) {
    *weight = 0.0;
    if (t->bn_st) {   // N of the first op (every op's N is the same unless agz_trainer_set_bn_stats gave them different weights)
      AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
      AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
      AGZ_HIP_TRY(hipMemcpy(weight, t->bn_st + t->bn_op(0).n, sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return AGZ_OK;
}
int agz_trainer_num_bn(const agz_trainer* t) { return t ? t->bn_num() : 0; }
int agz_trainer_get_bn_stats(const agz_trainer* t, int bi, float* mean, float* var, size_t C) {
  AGZ_REQUIRE(t && mean && var && bi >= 0 && bi < t->bn_num(), AGZ_E_INVALID, "agz_trainer_get_bn_stats: bad argument");
  AGZ_REQUIRE(t->bn_st && t->bn_have[bi], AGZ_E_STATE, "agz_trainer_get_bn_stats: no statistics tracked yet (N = 0)");
  AGZ_REQUIRE(C == (size_t)t->bn_op(bi).C, AGZ_E_INVALID, "agz_trainer_get_bn_stats: op %d has %d channels, got %zu", bi, t->bn_op(bi).C, C);
  std::vector<double> h;
  int r = bn_download(t, h);
  if (r != AGZ_OK) return r;
  bn_estimates(t, h, bi, mean, var);
  return AGZ_OK;
}
int agz_trainer_set_bn_stats(agz_trainer* t, int bi, const float* mean, const float* var, size_t C, double weight) {
  AGZ_REQUIRE(t && mean && var && bi >= 0 && bi < t->bn_num(), AGZ_E_INVALID, "agz_trainer_set_bn_stats: bad argument");
  AGZ_REQUIRE(std::isfinite(weight) && weight > 0, AGZ_E_INVALID, "agz_trainer_set_bn_stats: the weight must be finite and > 0 (got %g)", weight);
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  int r = t->bn_alloc();
  if (r != AGZ_OK) return r;
  const agz_trainer::BnOp op = t->bn_op(bi);
  AGZ_REQUIRE(C == (size_t)op.C, AGZ_E_INVALID, "agz_trainer_set_bn_stats: op %d has %d channels, got %zu", bi, op.C, C);
  std::vector<double> sm(C), sv(C);
  for (size_t c = 0; c < C; c++) { sm[c] = weight * (double)mean[c]; sv[c] = weight * (double)var[c]; }
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  AGZ_HIP_TRY(hipMemcpy(t->bn_st + op.mean, sm.data(), C * sizeof(double), hipMemcpyHostToDevice));
  AGZ_HIP_TRY(hipMemcpy(t->bn_st + op.var, sv.data(), C * sizeof(double), hipMemcpyHostToDevice));
  AGZ_HIP_TRY(hipMemcpy(t->bn_st + op.n, &weight, sizeof(double), hipMemcpyHostToDevice));
  t->bn_have[bi] = 1;
  return AGZ_OK;
}
int agz_trainer_reset_bn_stats(agz_trainer* t) {
  AGZ_REQUIRE(t, AGZ_E_INVALID, "agz_trainer_reset_bn_stats: NULL trainer");
  if (!t->bn_st) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipMemsetAsync(t->bn_st, 0, t->bn_total * sizeof(double), t->ctx->stream));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  std::fill(t->bn_have.begin(), t->bn_have.end(), (char)0);
  return AGZ_OK;
}

// The forward pass alone under the tracked estimates: a held-out loss.  Sharded: collective, the cost words alone are exchanged.
int agz_trainer_eval_dev(agz_trainer* t, const float* planes_dev, const float* pi_dev, const float* v_dev, float* cost) {
  AGZ_REQUIRE(t && planes_dev && pi_dev && v_dev, AGZ_E_INVALID, "agz_trainer_eval_dev: NULL argument");
  AGZ_REQUIRE(t->bn_all(), AGZ_E_STATE, "agz_trainer_eval: no running statistics yet (N = 0): track a training forward or set them first");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  int r = t->eval_pass(planes_dev, pi_dev, v_dev);
  if (r != AGZ_OK) return r;
  if (cost) {
    float c[2] = {0, 0};
    AGZ_HIP_TRY(hipMemcpyAsync(c, t->cost, 8, hipMemcpyDeviceToHost, t->ctx->stream));
    AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    *cost = c[0] + c[1];
  }
  return AGZ_OK;
}
int agz_trainer_eval(agz_trainer* t, const float* planes, const float* pi, const float* v, float* cost) {
  AGZ_REQUIRE(t && planes && pi && v, AGZ_E_INVALID, "agz_trainer_eval: NULL argument");
  AGZ_REQUIRE(t->bn_all(), AGZ_E_STATE, "agz_trainer_eval: no running statistics yet (N = 0): track a training forward or set them first");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  hipStream_t s = t->ctx->stream;
  AGZ_HIP_TRY(hipMemcpyAsync(t->d_planes, planes, (size_t)t->B * t->F * t->g.HW * 4, hipMemcpyHostToDevice, s));
  AGZ_HIP_TRY(hipMemcpyAsync(t->d_pi, pi, (size_t)t->B * t->A * 4, hipMemcpyHostToDevice, s));
  AGZ_HIP_TRY(hipMemcpyAsync(t->d_v, v, (size_t)t->B * 4, hipMemcpyHostToDevice, s));
  float c = 0.f;
  int r = agz_trainer_eval_dev(t, t->d_planes, t->d_pi, t->d_v, &c);
  if (r != AGZ_OK) return r;
  if (cost) *cost = c;
  return AGZ_OK;
}

// ---- checkpoints.  The file's format and what each form does to the trainer that loads it: ckpt.hpp, which also checks a whole file
// before anything here is changed.  This side describes the trainer (ckpt_layout), fetches and delivers tensors, and applies what a file
// carries.
namespace ckpt = agz::ckpt;

// BatchSize and the batch-shaped tensors are the GLOBAL batch's on a sharded trainer: its file is the plain trainer's at that batch size.
// A tied sharded trainer holds every tied tensor whole on every rank: its file is the tied trainer's at the global batch size
static ckpt::Layout ckpt_layout(const agz_trainer* t) {
  ckpt::Layout lay{t->conf, t->tied, {}, {}};
  lay.conf.BatchSize = t->B * t->n_ranks;
  for (const auto& p : t->prefs) {
    const bool split = pref_batch_shaped(p) && !t->tied;   // its rows are spread over the ranks
    lay.tensors.push_back({(uint64_t)pref_size(p) * (split ? t->n_ranks : 1), split});
  }
  for (int i = 0; i < t->bn_num(); i++) lay.bn_C.push_back((uint64_t)(i >= 2 * t->L + 1 ? (i == 2 * t->L + 1 ? 2 : 1) : t->K));
  return lay;
}
// the running statistics (the trainer holds some: bn_all()) as a checkpoint's BatchNorm block, and back
static int bn_block_get(const agz_trainer* t, ckpt::BnBlock& b) {
  std::vector<double> h;
  int r = bn_download(t, h);
  if (r != AGZ_OK) return r;
  b = ckpt::BnBlock{t->bn_lam, t->bn_on ? 1u : 0u, {}, {}, {}};
  for (int i = 0; i < t->bn_num(); i++) {
    const agz_trainer::BnOp op = t->bn_op(i);
    b.n.push_back(h[op.n]);
    b.sm.emplace_back(h.begin() + op.mean, h.begin() + op.mean + op.C);
    b.sv.emplace_back(h.begin() + op.var, h.begin() + op.var + op.C);
  }
  return AGZ_OK;
}
static int bn_block_apply(agz_trainer* t, const ckpt::BnBlock& b) {
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  int r = t->bn_alloc();
  if (r != AGZ_OK) return r;
  std::vector<double> h(t->bn_total, 0.0);
  for (int i = 0; i < t->bn_num(); i++) {
    const agz_trainer::BnOp op = t->bn_op(i);
    h[op.n] = b.n[i];
    for (int c = 0; c < op.C; c++) { h[op.mean + c] = b.sm[i][c]; h[op.var + c] = b.sv[i][c]; }
  }
  if ((r = bn_upload(t, h)) != AGZ_OK) return r;
  std::fill(t->bn_have.begin(), t->bn_have.end(), (char)1);
  t->bn_on = b.on != 0; t->bn_lam = b.lam;
  return AGZ_OK;
}
// the options an Adam checkpoint carries, into the trainer: momentum 0 releases a velocity, Adam on allocates the moments if there are none
static int adam_head_apply(agz_trainer* t, const ckpt::Options& o) {
  int r = agz_trainer_set_solver(t, &o.solver);
  if (r == AGZ_OK) r = agz_trainer_set_adam(t, &o.adam);
  if (r == AGZ_OK) t->adam_t = o.step;
  return r;
}
// a file with a velocity, loaded into a trainer with Adam on: the file's solver is taken and Adam turned off
static int adam_off(agz_trainer* t) {
  if (!t->adam.on) return AGZ_OK;
  agz_adam_conf c = t->adam;
  c.on = 0;
  return agz_trainer_set_adam(t, &c);
}
// group 0 / 1 / 2 of a checkpoint's tensor blocks: the learnables, then the velocity or (Adam) the first moments, then the second moments
static float* group_buf(const agz_trainer* t, int group) { return group == 0 ? t->P : t->M1 ? (group == 1 ? t->M1 : t->M2) : t->V; }

// Sharded (collective): rank 0 writes the plain trainer's file at the global batch.  Tensor by tensor, batch-shaped ones are gathered from
// every rank (rows in rank order = the global tensor) through one device buffer of n slices; nothing larger than one global tensor is ever
// staged on the host.  Every rank enters every gather whatever failed locally, and the call ends with the status exchange.  The options,
// and so the form, are the same on every rank; so are the running statistics rank 0 writes.
int agz_trainer_save(const agz_trainer* t, const char* path) {
  AGZ_REQUIRE(t && path, AGZ_E_INVALID, "agz_trainer_save: NULL argument");
  const int n = t->n_ranks;
  auto agree = [&](int rc) { return t->sharded ? t->shard.agree(rc) : rc; };
  int rc = hipSetDevice(t->ctx->device) == hipSuccess && hipStreamSynchronize(t->ctx->stream) == hipSuccess ? AGZ_OK : AGZ_E_HIP;
  FILE* f = nullptr;
  if (t->rank == 0 && !(f = fopen(path, "wb"))) { agz::set_error("agz_trainer_save: cannot open %s", path); rc = AGZ_E_INVALID; }
  size_t mx = 0;
  const bool split = t->sharded && !t->tied;   // (tied sharded: rank 0 holds every tensor whole and writes the tied trainer's file; the call stays collective)
  for (const auto& p : t->prefs) if (split && pref_batch_shaped(p)) mx = std::max(mx, pref_size(p));
  float* d = nullptr;   // (sharded) [n][mx] gathered slices, then this rank's slice
  if (mx && hipMalloc(&d, (size_t)(n + 1) * mx * 4) != hipSuccess) { d = nullptr; if (rc == AGZ_OK) { agz::set_error("agz_trainer_save: out of device memory for the gather"); rc = AGZ_E_NOMEM; } }
  const int a = agree(rc);
  if (a != AGZ_OK) { if (f) fclose(f); if (d) hipFree(d); return a; }
  const ckpt::Form form{t->tied, t->M1 ? ckpt::ADAM : t->V ? ckpt::VELOCITY : ckpt::NONE, t->bn_all()};
  ckpt::BnBlock bn;
  if (f && form.bn && bn_block_get(t, bn) != AGZ_OK) rc = AGZ_E_HIP;
  std::vector<float> v, all;
  const bool ok = ckpt::write(f, ckpt_layout(t), form, ckpt::Options{t->solver, t->adam, t->adam_t}, bn, [&](int g, size_t i) {
    const TParamRef& p = t->prefs[i];
    v.assign(pref_size(p), 0.f);
    if (xfer_param(t, group_buf(t, g), (int)i, v.data(), 1) != AGZ_OK && rc == AGZ_OK) rc = AGZ_E_HIP;
    if (!split || !pref_batch_shaped(p)) return std::make_pair((const float*)v.data(), (uint64_t)v.size());
    float* mine = d + (size_t)n * mx;
    if (hipMemcpy(mine, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess && rc == AGZ_OK) rc = AGZ_E_HIP;
    const int r = t->shard.allgather_bytes(mine, d, v.size() * 4);
    if (r != AGZ_OK && rc == AGZ_OK) rc = r;
    all.resize(f ? v.size() * n : 0);
    if (f && hipMemcpy(all.data(), d, all.size() * 4, hipMemcpyDeviceToHost) != hipSuccess && rc == AGZ_OK) rc = AGZ_E_HIP;
    return std::make_pair((const float*)all.data(), (uint64_t)all.size());
  });
  const bool closed = !f || fclose(f) == 0;
  if (d) hipFree(d);
  if (f && !(ok && closed) && rc == AGZ_OK) { agz::set_error("agz_trainer_save: write to %s failed", path); rc = AGZ_E_INVALID; }
  return agree(rc);
}

// Local also on a sharded trainer: a checkpoint of the GLOBAL configuration, of which this rank reads its rows of every batch-shaped tensor.
// Nothing is changed unless ckpt::scan accepts the whole file; after a failure further down (a device error) the state is undefined.
int agz_trainer_load(agz_trainer* t, const char* path) {
  AGZ_REQUIRE(t && path, AGZ_E_INVALID, "agz_trainer_load: NULL argument");
  FILE* f = fopen(path, "rb");
  AGZ_REQUIRE(f, AGZ_E_INVALID, "agz_trainer_load: cannot open %s", path);
  const ckpt::Layout lay = ckpt_layout(t);
  ckpt::Scan sc;
  const ckpt::Status st = ckpt::scan(f, lay, &sc);
  if (st != ckpt::OK) {
    fclose(f);
    if (st == ckpt::KIND)   // (sharded handles alike: a tied file loads into agz_trainer_create_sharded_tied, a plain one into agz_trainer_create_sharded)
      agz::set_error("agz_trainer_load: %s is the checkpoint of a %s trainer, this trainer is %s", path,
                     sc.form.tied ? "tied (agz_trainer_create_tied / agz_trainer_create_sharded_tied)" : "plain (agz_trainer_create / agz_trainer_create_sharded)",
                     t->tied ? "tied" : "plain");
    else if (st == ckpt::NOT_THIS) agz::set_error("agz_trainer_load: %s is not a checkpoint of this trainer configuration (batch size %d)", path, lay.conf.BatchSize);
    else agz::set_error("agz_trainer_load: %s is truncated or mismatched", path);
    return AGZ_E_INVALID;
  }
  auto apply_group = [&](int g) -> int {   // every tensor of the group (of a batch-shaped one: this rank's rows) into the group's buffer
    std::vector<float> v;
    for (size_t i = 0; i < t->prefs.size(); i++) {
      const std::pair<long, uint64_t> rows = ckpt::rows(lay.tensors[i], sc.off[g][i], t->rank, t->n_ranks);
      v.resize(rows.second);
      if (fseek(f, rows.first, SEEK_SET) != 0 || fread(v.data(), 4, v.size(), f) != v.size()) { agz::set_error("agz_trainer_load: reading %s failed", path); return AGZ_E_INVALID; }
      if (xfer_param(t, group_buf(t, g), (int)i, v.data(), 0) != AGZ_OK) return AGZ_E_HIP;
    }
    return AGZ_OK;
  };
  const ckpt::State state = sc.form.state;
  int r = hipSetDevice(t->ctx->device) == hipSuccess && hipStreamSynchronize(t->ctx->stream) == hipSuccess ? AGZ_OK : AGZ_E_HIP;
  if (r == AGZ_OK) r = apply_group(0);
  if (r == AGZ_OK && state == ckpt::ADAM) r = adam_head_apply(t, sc.opt);
  if (r == AGZ_OK && state == ckpt::VELOCITY && (r = adam_off(t)) == AGZ_OK) r = agz_trainer_set_solver(t, &sc.opt.solver);
  for (int g = 1; r == AGZ_OK && g < ckpt::groups(state); g++) r = apply_group(g);
  fclose(f);
  if (r == AGZ_OK) r = sc.form.bn ? bn_block_apply(t, sc.bn) : agz_trainer_reset_bn_stats(t);
  if (r == AGZ_OK && state == ckpt::NONE) r = agz_trainer_reset_solver(t);   // v := 0 (Adam: the moments and t := 0), the options stay
  return r;
}

// the running statistics, if the trainer holds any (N > 0), as the net's AGZ_BN_RUNNING statistics; nothing otherwise
static int export_bn(const agz_trainer* t, agz_net* net) {
  if (!t->bn_all()) return AGZ_OK;
  std::vector<double> h;
  int r = bn_download(t, h);
  if (r != AGZ_OK) return r;
  for (int i = 0; i < t->bn_num(); i++) {
    const int C = t->bn_op(i).C;
    std::vector<float> m(C), v(C);
    bn_estimates(t, h, i, m.data(), v.data());
    if ((r = agz_net_set_bn_stats(net, i, m.data(), v.data(), (size_t)C)) != AGZ_OK) return r;
  }
  return AGZ_OK;
}

// row 0 of every learnable as rank 0 holds it (a plain trainer's export), broadcast to every rank: the nets are bit-identical everywhere
static int export_sharded(const agz_trainer* t, agz_net* net) {
  int rc = AGZ_OK;
  size_t mx = 0;
  for (int i = 0; i < (int)t->prefs.size(); i++) {
    size_t want = 0;
    if (agz_net_param_info(net, i, nullptr, 0, &want) != AGZ_OK || want > pref_size(t->prefs[i])) { rc = AGZ_E_INVALID; want = 0; }
    mx = std::max(mx, want);
  }
  if (rc != AGZ_OK) agz::set_error("agz_trainer_export: network shapes differ");
  float* d = nullptr;
  if (hipMalloc(&d, std::max<size_t>(mx, 1) * 4) != hipSuccess) { d = nullptr; if (rc == AGZ_OK) { agz::set_error("agz_trainer_export: out of device memory"); rc = AGZ_E_NOMEM; } }
  int a = t->shard.agree(rc);
  if (a != AGZ_OK) { if (d) hipFree(d); return a; }
  std::vector<float> v;
  for (int i = 0; i < (int)t->prefs.size(); i++) {
    size_t want = 0;
    agz_net_param_info(net, i, nullptr, 0, &want);
    const TParamRef& p = t->prefs[i];
    const bool conv_bn = p.layer >= 0 && (p.sub % 10) != 0;   // as agz_trainer_export: row 0 only of the tower's gamma / beta
    if (t->rank == 0) {
      v.assign(conv_bn ? want : pref_size(p), 0.f);
      if (xfer_param(t, t->P, i, v.data(), 1, conv_bn ? 1 : 0) != AGZ_OK && rc == AGZ_OK) rc = AGZ_E_HIP;
      if (hipMemcpy(d, v.data(), want * 4, hipMemcpyHostToDevice) != hipSuccess && rc == AGZ_OK) rc = AGZ_E_HIP;
    }
    int r = t->shard.bcast0(d, want * 4);
    if (r != AGZ_OK && rc == AGZ_OK) rc = r;
    v.assign(want, 0.f);
    if (hipMemcpy(v.data(), d, want * 4, hipMemcpyDeviceToHost) != hipSuccess && rc == AGZ_OK) rc = AGZ_E_HIP;
    if (rc == AGZ_OK && (r = agz_net_set_param(net, i, v.data(), want)) != AGZ_OK) rc = r;
  }
  hipFree(d);
  if (rc == AGZ_OK) rc = export_bn(t, net);   // (every rank holds the same bits and exports its own)
  rc = t->shard.agree(rc);
  return rc == AGZ_OK ? agz_net_commit(net) : rc;
}

// the copy loop of dual.Infer (meta.go:141-146): row 0 of every learnable -> the inference net, then commit
int agz_trainer_export(const agz_trainer* t, agz_net* net) {
  AGZ_REQUIRE(t && net, AGZ_E_INVALID, "NULL argument");
  AGZ_REQUIRE((int)t->prefs.size() == agz_net_num_params(net), AGZ_E_INVALID, "agz_trainer_export: network shapes differ");
  AGZ_HIP_TRY(hipSetDevice(t->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  if (t->sharded) return export_sharded(t, net);
  for (int i = 0; i < (int)t->prefs.size(); i++) {
    size_t want = 0;
    int r = agz_net_param_info(net, i, nullptr, 0, &want);
    if (r != AGZ_OK) return r;
    const TParamRef& p = t->prefs[i];
    const bool conv_bn = p.layer >= 0 && (p.sub % 10) != 0;   // batch-shaped [B][K][H][W]: only row 0 is transferred
    std::vector<float> v(conv_bn ? want : pref_size(p));
    r = xfer_param(t, t->P, i, v.data(), 1, conv_bn ? 1 : 0);
    if (r != AGZ_OK) return r;
    AGZ_REQUIRE(v.size() >= want, AGZ_E_INVALID, "agz_trainer_export: parameter %d too small", i);
    r = agz_net_set_param(net, i, v.data(), v.size());  // takes row 0 of batch-shaped tensors
    if (r != AGZ_OK) return r;
  }
  { int r = export_bn(t, net); if (r != AGZ_OK) return r; }
  return agz_net_commit(net);
}

}  // extern "C"
