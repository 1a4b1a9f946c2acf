// Dual-block 3x3 convolution with ONE bf16 product per multiply (AGZ_COMPUTE_BF16) — NOT fp32-grade.
//
// Declared arithmetic (`bf16-tower`): every fp32 filter value is rounded once to bf16 (round to nearest even) when
// the weight image is built; every fp32 input activation is rounded the same way on its way into LDS (v_cvt_pk_bf16_f32: NaN stays a
// quiet NaN, Inf stays Inf, finite values past the bf16 range round to Inf — nothing beyond what RNE gives); products of two 8-bit
// significands are exact in fp32; accumulation is the MFMA's fp32; the epilogue is the fp32 relu(relu(bn a) + relu(bn b)) of the other
// modes on the same d_ep_dual[l].  One v_mfma_f32_32x32x16_bf16 per product: 436 GFLOP per block at 19x19 / K=256 / 512 boards.
//
// Work split.  A workgroup owns ONE board (boards of more than 384 pixels: a run of at most 384 of its pixels, `rows_tile`) and one
// 128-column tile [64 branch-a | 64 branch-b] — the interleave of d_ep_dual / the other dual kernels.  No workgroup ever holds rows of
// two boards and K is never split: the summation order of an output element is (64-channel chunk, tap, 16-channel step) whatever the
// batch is and wherever the board sits in it, so the block is bit-identical per board at every batch size.
// 4 waves, one per SIMD; wave w owns rows [96 w, 96 w + 96) x all 128 columns: 3 x 4 MFMA tiles, 192 accumulator registers (the
// unified 512-register file of a single-wave SIMD holds them; 0 spills).  361 rows = 11.3 row blocks: rows past the board (or past the
// workgroup's run) clamp to its last pixel for the LDS reads and are never stored.
//
// Activations go into LDS once per 64-channel chunk, not once per tap.  The workgroup stages the haloed slice of its board —
// (lines + 2) x (W + 2) pixels, 21 x 21 at 19x19, the zero halo comes with the padded NHWC layout — as bf16, 128 bytes per pixel
// (56 KB at 19x19), two stages (chunk c+1 is fetched, converted and written while chunk c is multiplied: two 32-byte units per
// thread and tap).  The nine taps are nine SHIFTED fragment reads of that one image: row m = (line, col) reads pixel
// (line + ky) (W + 2) + col + kx.  Weights: the [128 columns][64 channels] bf16 tile of one (chunk, tap), 16 KB, two stages, copied
// 16 bytes per lane from an image that is already in LDS byte order (build_bf16_weights: wq[n_tile][chunk][tap][16 KB], the kernel's
// K loop — chunk outer, tap inner — front to back).  LDS: 2 x 56 KB + 2 x 16 KB = 144 KB static, one workgroup per CU.
//
// Bank argument (LDS: 64 banks = a 256-byte window of sixteen 16-byte slots; a ds_read_b128 / ds_write_b128 is served 16 lanes at a
// time and is conflict-free when those 16 lanes touch 16 different slots):
//   image address of (pixel p, 16-byte unit u of its 8)  =  128 p + 16 (u ^ f),   f = ((p - 2 line(p)) >> 1) & 7
//   so the slot is 8 (p & 1) + (u ^ f).  p - 2 line = line W + col counts the pixels as the GEMM rows do (the two halo columns
//   between board lines taken out), and stepping a tap adds the constant kx + W ky to it.  The 16 lanes of a fragment read hold 16
//   CONSECUTIVE rows and one u: their pixels are consecutive but for the jump of two at a line end, which keeps the parity pattern,
//   so 8 are even and 8 odd, and within either parity (p - 2 line) >> 1 runs through 8 consecutive integers: 8 different f, 16
//   different slots — for all nine shifts.  (Clamped rows repeat one address: a broadcast.)  The staging write puts the 8 units of
//   one pixel on 8 consecutive lanes: 16 lanes = an even and an odd pixel x 8 units = 16 slots.  The weight tile is the same image
//   with f = (n >> 1) & 7 (rows are consecutive columns n), written lane-linearly.
//
// Cost model (19x19, K=256, 512 boards: 2048 workgroups of 36 (chunk, tap) steps x 4 channel steps):
//   LDS reads per MFMA   a channel step of a wave reads 3 A + 4 B fragments of 1 KB for 12 MFMAs: 0.58 KB per MFMA
//                        (the 64x64 wave tile of conv_x3.hpp at one MFMA per product would read 1 KB per MFMA)
//   L2 -> CU, per launch activations 2048 x 441 x 256 x 4 B = 0.92 GB (a board's slice once per n-tile, not once per tap; the four
//                        n-tiles of a board are adjacent workgroups of one XCD, so three of the four reads are L2 hits),
//                        weights 2048 x 576 KB = 1.21 GB, epilogue parameters 2048 x 361 x 64 x 16 B = 0.76 GB
//   registers            DESIGN.md section 4f quotes the compiler's resource-usage remarks
// Batch-1 speed is out of scope here: one board is four workgroups on 256 CUs (the small-batch form of the bf16-activation tower: conv_bf16s.hpp).
//
// Element type.  The kernel is a template over the 16-bit element E of its two operands: Bf16El (the arithmetic above) or Fp16El
// (AGZ_COMPUTE_FP16, DESIGN.md section 2 `fp16-tower`, section 4j: IEEE half, every activation clamped to [-65504, 65504] and rounded
// to nearest even, every filter rounded at its own power-of-two scale by agz_net::build_fp16_weights, which folds the scale back into the
// epilogue image the kernel is handed as `ep`).  Three things differ under E: the pack-and-round helper (E::pack2), the MFMA (E::mfma:
// v_mfma_f32_32x32x16_f16 runs at the bf16 instruction's rate on the same operand registers) and the fragment vector type (E::frag).
// The element is 16 bits either way, so everything else above carries over byte for byte — the LDS images and their swizzle, the bank
// argument, the XCD order, the accumulation order, the byte model — and the Bf16El instantiation compiles to the code the
// untemplated kernel compiled to.
#pragma once
// (included by net.hip INSIDE namespace agz, after conv_x3.hpp: bf16x8_t, u32x4_t, f32x16)

constexpr int BF16_ROWS = 384;                 // GEMM rows of a workgroup: 4 waves x 3 row blocks of 32
constexpr int BF16_SP_MAX = 448;               // haloed pixels of a staged slice (19x19: 441)
constexpr int BF16_A_STAGE = BF16_SP_MAX * 128;
constexpr int BF16_B_STAGE = 128 * 128;        // [128 columns][64 channels] bf16

// The kernel and its helpers are compiled without the packed-fp32 instructions (v_pk_fma_f32 and kin, which hipcc would pick for the
// epilogue): plain v_fma_f32 there.  Inlining needs caller and callee to agree on the feature, so the helpers carry the attribute too
// and the kernel calls nothing else (clang vector types instead of float4, no library min).
#define BF16_FN __attribute__((target("no-packed-fp32-ops")))

struct Bf16Args {
  const float* x;            // padded NHWC [B][Hp][Wp][Kp]
  float* y;
  const f32x4* ep;           // {sa, ta, sb, tb} [HW][Kp]
  const unsigned short* wq;  // agz_net::build_bf16_weights image (Fp16El: build_fp16_weights, with its folded ep)
  int HW, W, Wp, HpWp, Kp;
  int n_ntiles, m_per_board, rows_tile, ncc;   // ncc = Kp / 64 channel chunks
};

// two fp32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32), a in the low half
BF16_FN __device__ __forceinline__ unsigned bf16_pack2(float a, float b) {
  typedef float bf16_f2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16_b2 __attribute__((ext_vector_type(2)));
  bf16_f2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16_b2));
}

// two fp32 -> packed IEEE half pair, a in the low half: clamp to [-65504, 65504], then round to nearest even (the convert follows the
// mode register's default, RNE; v_cvt_pkrtz would truncate).  The compares are false for a NaN, which so reaches the convert and stays a
// NaN; +-Inf and every finite value past the half range become +-65504: no Inf ever comes out.  Subnormal halves are produced, not flushed.
BF16_FN __device__ __forceinline__ unsigned fp16_pack2(float a, float b) {
  typedef float fp16_f2 __attribute__((ext_vector_type(2)));
  typedef _Float16 fp16_h2 __attribute__((ext_vector_type(2)));
  a = a > 65504.f ? 65504.f : a;
  a = a < -65504.f ? -65504.f : a;
  b = b > 65504.f ? 65504.f : b;
  b = b < -65504.f ? -65504.f : b;
  fp16_f2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, fp16_h2));
}

// The element types of the single-product tower (conv_bf16.hpp, conv_bf16a.hpp, conv_bf16s.hpp, conv_bf16p.hpp)
struct Bf16El {
  typedef bf16x8_t frag;
  BF16_FN static __device__ __forceinline__ unsigned pack2(float a, float b) { return bf16_pack2(a, b); }
  BF16_FN static __device__ __forceinline__ f32x16 mfma(frag A, frag B, f32x16 C) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, C, 0, 0, 0); }
};
struct Fp16El {
  typedef _Float16 frag __attribute__((ext_vector_type(8)));
  BF16_FN static __device__ __forceinline__ unsigned pack2(float a, float b) { return fp16_pack2(a, b); }
  BF16_FN static __device__ __forceinline__ f32x16 mfma(frag A, frag B, f32x16 C) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B, C, 0, 0, 0); }
};

// __syncthreads() spelled out (the library's is a function without the attribute: it would stay a call)
BF16_FN __device__ __forceinline__ void bf16_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// staging unit `idx` of a slice (pixel idx / 8, 16-byte unit idx % 8): byte offset of its 32 fp32 bytes from the slice's first
// pixel (channel chunk 0) and byte offset of its bf16 unit in the LDS image (the bank argument above)
BF16_FN __device__ __forceinline__ void bf16_unit(int idx, int pbase, int Wp, int Kp, unsigned& goff, unsigned& loff) {
  const int q = idx >> 3, u = idx & 7;
  const int p = pbase + q, line = p / Wp;
  goff = ((unsigned)q * (unsigned)Kp + (unsigned)u * 8u) * 4u;
  loff = (unsigned)q * 128u + (unsigned)((u ^ (((p - 2 * line) >> 1) & 7)) << 4);
}

template <typename E>
BF16_FN __global__ __launch_bounds__(256, 1) void conv3x3_bf16_dual_kernel(Bf16Args a) {
  typedef typename E::frag frag_t;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BF16_A_STAGE + 2 * BF16_B_STAGE];
  unsigned char* const ldsA = lds;
  unsigned char* const ldsB = lds + 2 * BF16_A_STAGE;

  // XCD-aware order (as conv3x3_x3_kernel): consecutive tiles — the n-tiles of one board, then the next board — share an XCD's L2
  const int nblk = gridDim.x, id = blockIdx.x;
  const int xq = nblk >> 3, xr = nblk & 7, xcd = id & 7, slot = id >> 3;
  const int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + slot;
  const int n_tile = tile % a.n_ntiles, bm = tile / a.n_ntiles;
  const int b = bm / a.m_per_board, mt = bm - b * a.m_per_board;
  const int m0 = mt * a.rows_tile;
  const int mend = m0 + a.rows_tile < a.HW ? m0 + a.rows_tile : a.HW;           // rows [m0, mend) of board b
  const int line0 = m0 / a.W, line1 = (mend - 1) / a.W;
  const int SP = (line1 - line0 + 3) * a.Wp;               // haloed pixels staged (<= BF16_SP_MAX, checked by the launcher)
  const int pbase = line0 * a.Wp;                          // first of them in the board's padded image

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5;
  const char* xb = reinterpret_cast<const char*>(a.x + ((size_t)b * a.HpWp + pbase) * a.Kp);
  const char* wb = reinterpret_cast<const char*>(a.wq) + (size_t)n_tile * a.ncc * 9 * BF16_B_STAGE + tid * 16;
  const int nit = a.ncc * 9;

  // fragment rows of this lane: row block 3 wid + i, row lane & 31 -> top-left pixel of its 3x3 window inside the slice
  int prel[3], mrow[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int m = m0 + (3 * wid + i) * 32 + (lane & 31);
    if (m >= mend) m = mend - 1;
    const int line = m / a.W, col = m - line * a.W;
    prel[i] = (line - line0) * a.Wp + col;
    mrow[i] = m;
  }
  const unsigned bsw = (unsigned)((lane & 31) >> 1) & 7u;
  const unsigned brow = (unsigned)(lane & 31) * 128u;

  f32x16 acc[3][2][2];   // [row block][32-channel group][branch]
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int br = 0; br < 2; br++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][j][br][r] = 0.f;

  f32x4 ra[2][2];      // two staging units of the next chunk's activations
  u32x4_t rb[4];       // the next step's weight tile: four 16-byte runs per lane
  bool av[2];
  unsigned ag[2], al[2];

#define BF16_LOAD_A(T, CC)                                                                       \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; s_++) {                                             \
    const int idx_ = tid + 256 * (2 * (T) + s_);                                                 \
    av[s_] = idx_ < SP * 8;                                                                      \
    bf16_unit(av[s_] ? idx_ : 0, pbase, a.Wp, a.Kp, ag[s_], al[s_]);                             \
    if (av[s_]) {                                                                                \
      const char* g_ = xb + ag[s_] + (unsigned)(CC) * 256u;                                      \
      ra[s_][0] = *reinterpret_cast<const f32x4*>(g_);                                          \
      ra[s_][1] = *reinterpret_cast<const f32x4*>(g_ + 16);                                     \
    }                                                                                            \
  }
#define BF16_STORE_A(DST)                                                                        \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; s_++)                                               \
    if (av[s_]) {                                                                                \
      u32x4_t v_ = {E::pack2(ra[s_][0].x, ra[s_][0].y), E::pack2(ra[s_][0].z, ra[s_][0].w),      \
                    E::pack2(ra[s_][1].x, ra[s_][1].y), E::pack2(ra[s_][1].z, ra[s_][1].w)};     \
      *reinterpret_cast<u32x4_t*>((DST) + al[s_]) = v_;                                          \
    }
#define BF16_LOAD_B(IT)                                                                          \
  _Pragma("unroll") for (int j_ = 0; j_ < 4; j_++)                                               \
    rb[j_] = *reinterpret_cast<const u32x4_t*>(wb + (size_t)(IT) * BF16_B_STAGE + j_ * 4096);
#define BF16_STORE_B(DST)                                                                        \
  _Pragma("unroll") for (int j_ = 0; j_ < 4; j_++)                                               \
    *reinterpret_cast<u32x4_t*>((DST) + tid * 16 + j_ * 4096) = rb[j_];

  // prologue: chunk 0 of the slice and the first weight tile
  BF16_LOAD_B(0)
  BF16_STORE_B(ldsB)
  // (nothing to hide this fetch behind: nine units per thread in flight at a time, two rounds, instead of nine rounds of two)
#pragma unroll 1
  for (int h9 = 0; h9 < 2; h9++) {
    f32x4 pa[9][2];
    unsigned pl[9];
    bool pv[9];
#pragma unroll
    for (int t = 0; t < 9; t++) {
      const int idx = tid + 256 * (9 * h9 + t);
      unsigned pg;
      pv[t] = idx < SP * 8;
      bf16_unit(pv[t] ? idx : 0, pbase, a.Wp, a.Kp, pg, pl[t]);
      if (pv[t]) {
        pa[t][0] = *reinterpret_cast<const f32x4*>(xb + pg);
        pa[t][1] = *reinterpret_cast<const f32x4*>(xb + pg + 16);
      }
    }
#pragma unroll
    for (int t = 0; t < 9; t++)
      if (pv[t]) {
        u32x4_t v = {E::pack2(pa[t][0].x, pa[t][0].y), E::pack2(pa[t][0].z, pa[t][0].w),
                     E::pack2(pa[t][1].x, pa[t][1].y), E::pack2(pa[t][1].z, pa[t][1].w)};
        *reinterpret_cast<u32x4_t*>(ldsA + pl[t]) = v;
      }
  }
  bf16_sync();

  for (int cc = 0; cc < a.ncc; cc++) {
    const unsigned char* Ac = ldsA + (cc & 1) * BF16_A_STAGE;
    unsigned char* An = ldsA + ((cc & 1) ^ 1) * BF16_A_STAGE;
    const bool more_a = cc + 1 < a.ncc;
    int kx = 0, tapoff = 0, tapsw = 0;   // ky Wp + kx and kx + W ky of the tap
#pragma unroll 1
    for (int tap = 0; tap < 9; tap++) {
      const int it = cc * 9 + tap;
      const bool more_b = it + 1 < nit;
      // the next step's operands leave for the registers before this step's MFMAs ...
      if (more_b) { BF16_LOAD_B(it + 1) }
      if (more_a) { BF16_LOAD_A(tap, cc + 1) }
      const unsigned char* Bc = ldsB + (it & 1) * BF16_B_STAGE;
      unsigned aoff[3], asw[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        aoff[i] = (unsigned)(prel[i] + tapoff) * 128u;
        asw[i] = (unsigned)((mrow[i] + tapsw) >> 1) & 7u;
      }
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const unsigned u = (unsigned)(2 * ks + half);
        frag_t A_[3], B_[4];
#pragma unroll
        for (int i = 0; i < 3; i++) A_[i] = *reinterpret_cast<const frag_t*>(Ac + aoff[i] + ((u ^ asw[i]) << 4));
#pragma unroll
        for (int jb = 0; jb < 4; jb++) B_[jb] = *reinterpret_cast<const frag_t*>(Bc + jb * 4096 + brow + ((u ^ bsw) << 4));
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 2; j++)
#pragma unroll
            for (int br = 0; br < 2; br++)
              acc[i][j][br] = E::mfma(A_[i], B_[br * 2 + j], acc[i][j][br]);
      }
      // ... and go to the other stages behind them (last read a whole step / chunk ago, before the barrier that ended it)
      if (more_b) { BF16_STORE_B(ldsB + ((it + 1) & 1) * BF16_B_STAGE) }
      if (more_a) { BF16_STORE_A(An) }
      bf16_sync();
      if (kx < 2) { kx++; tapoff++; tapsw++; }
      else { kx = 0; tapoff += a.Wp - 2; tapsw += a.W - 2; }
    }
  }
#undef BF16_LOAD_A
#undef BF16_STORE_A
#undef BF16_LOAD_B
#undef BF16_STORE_B
#undef BF16_FN

  // epilogue: BN(scale, shift) + ReLU per branch, add, ReLU; interior of the padded NHWC output
  float* yb = a.y + (size_t)b * a.HpWp * a.Kp;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int rh = 0; rh < 2; rh++) {
      // the parameters of eight rows leave together (rows past the end load the last row's: no branch around a load, one wait
      // per sixteen loads — a wave alone on its SIMD has nobody to hide a load-use chain per row behind)
      f32x4 e[8][2];
#pragma unroll
      for (int rr = 0; rr < 8; rr++) {
        const int r = rh * 8 + rr;
        const int m = m0 + (3 * wid + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int mc = m < mend ? m : mend - 1;
#pragma unroll
        for (int j = 0; j < 2; j++) e[rr][j] = a.ep[(unsigned)mc * (unsigned)a.Kp + (unsigned)(n_tile * 64 + j * 32 + (lane & 31))];
      }
#pragma unroll
      for (int rr = 0; rr < 8; rr++) {
        const int r = rh * 8 + rr;
        const int m = m0 + (3 * wid + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < mend) {
          const int h = m / a.W, w = m - h * a.W;
          const unsigned obase = (unsigned)((h + 1) * a.Wp + (w + 1)) * (unsigned)a.Kp;
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const int c = n_tile * 64 + j * 32 + (lane & 31);
            float va = acc[i][j][0][r] * e[rr][j].x + e[rr][j].y;
            float vb = acc[i][j][1][r] * e[rr][j].z + e[rr][j].w;
            va = va > 0.f ? va : 0.f;
            vb = vb > 0.f ? vb : 0.f;
            const float s = va + vb;
            yb[obase + c] = s > 0.f ? s : 0.f;
          }
        }
      }
    }
  }
}
