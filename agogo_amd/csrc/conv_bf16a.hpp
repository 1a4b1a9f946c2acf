// The single-product bf16 dual block of conv_bf16.hpp with bf16 ACTIVATIONS in device memory (AGZ_COMPUTE_BF16_ACT) and both operands
// DMA'd global -> LDS.  Same declared arithmetic (`bf16-tower`), same results bit for bit: a block's output is
// read by the next block only, which rounds it to bf16 (RNE, v_cvt_pk_bf16_f32) before the first multiply — here the PRODUCER rounds it,
// once, with that instruction, in its epilogue, and stores the bf16.  A layout, not a precision.  DESIGN.md section 4g.
//
// What stays (and makes the result equal to conv3x3_bf16_dual_kernel's): one workgroup per (board run of rows_tile pixels, 128-column
// tile [64 a | 64 b]) in the XCD-aware order; four waves of 96 rows x 128 columns; every accumulator sums in the order (64-channel chunk,
// tap, 16-channel step) with v_mfma_f32_32x32x16_bf16; the ragged-M clamp; the fp32 epilogue relu(relu(bn a) + relu(bn b)) on d_ep_dual[l];
// the LDS images (conv_bf16.hpp's bank argument holds unchanged: the images are byte-identical).
//
// What is new.
//   A operand, IN_BF16    In padded NHWC bf16 one pixel's 64-channel chunk is 128 contiguous bytes = one row of the LDS image.  A DMA
//                         instruction (buffer_load ... lds, 16 bytes per lane) writes LDS lane-linearly: wave base + 16 lane.  So round r
//                         of a workgroup fills LDS units idx = 256 r + tid = (pixel q = idx / 8, slot s = idx % 8), 32 pixels, and the
//                         swizzle 128 p + 16 (u ^ f(p)) is kept by choosing WHICH global unit a lane fetches: u = s ^ f(p) (the XOR is
//                         an involution).  A haloed 19x19 slice is 441 x 8 = 3528 units = 14 rounds (BF16_SP_MAX x 8 = 14 x 256 exactly);
//                         tap t of chunk c issues rounds t and t + 9 of chunk c + 1 into the other stage.  Lanes past the slice are
//                         masked off: the tail of the stage is never read.  The chunk travels in the scalar offset.
//   A operand, !IN_BF16   block 0 reads the input convolution's fp32 output: conv_bf16.hpp's load / v_cvt_pk / ds_write staging.
//   B operand             the next (chunk, tap) tile, 16 KB of wq (already in LDS byte order, lane-linear), four DMA instructions per lane.
//   completion            a step's DMA is issued before its MFMAs and every wave waits for ITS OWN outstanding DMA (s_waitcnt vmcnt(0):
//                         a wave's vector-memory operations retire in order and an LDS-DMA counts as a load) before the workgroup
//                         barrier that ends the step — so behind the barrier every wave's part of the next stages has landed, and no
//                         DMA is ever in flight across a barrier (the rule of wino_gemm_h2g_kernel, conv_wino_h2c.hpp).  The four
//                         stages are four separate __shared__ objects and the chunk and tap loops are unrolled by two so that every LDS
//                         access names its stage at compile time: the compiler's LDS-DMA tracking then does not hold this step's ds_reads (stages
//                         Ac, Bc) back for the DMA in flight into the other two.
//   fragments             two sets: channel step k + 1's ds_read_b128s are issued under step k's MFMAs (no staging registers in the way).
//   epilogue, OUT_BF16    the fp32 result is rounded with v_cvt_pk_bf16_f32 (the two 32-channel groups of a lane in one instruction),
//                         goes through the LDS activation stage — dead after the last barrier; every wave uses its own 12 KB,
//                         [96 rows][64 channels] bf16, so no workgroup barrier — and leaves as 16-byte vector stores: 8 lanes per pixel,
//                         128 contiguous bytes of the padded NHWC bf16 output's interior.  Bank argument: a lane writes 2 bytes at
//                         128 lr + 16 ((c >> 3) ^ g(lr)) + 2 (c & 7), g(lr) = 4 ((lr >> 2) & 1).  The 64 lanes of one write hold rows lr
//                         (lanes 0..31) and lr + 4 (lanes 32..63), 32 consecutive channels each: same 128-byte half of the bank window,
//                         units {0..3} ^ g and {0..3} ^ g ^ 4 — disjoint, 32 different banks, two lanes on the two halves of each word.
//                         The read-back is a ds_read_b128 of 8 lanes per row: 16 lanes = an even and an odd row x 8 slots = 16 slots.
//   epilogue, !OUT_BF16   the last block stores fp32 as conv_bf16.hpp does: the heads read what they read in AGZ_COMPUTE_BF16.
// Byte model (19x19, K=256, 512 boards, 2048 workgroups): activations L2 -> CU 2048 x 441 x 256 x 2 B = 0.46 GB (0.92 in conv_bf16.hpp),
// stored 46 KB per workgroup (92); weights 1.21 GB and epilogue parameters 0.76 GB as before.
//
// Element type E (conv_bf16.hpp): Bf16El is everything above; Fp16El is AGZ_COMPUTE_FP16 (DESIGN.md section 2 `fp16-tower`, section 4j) —
// where "bf16" stands above read "the 16-bit element", where v_cvt_pk_bf16_f32 stands read E::pack2 (half: clamp to +-65504, then RNE),
// where the MFMA stands read E::mfma.  The activation pair holds halves, `ep` is the folded image of build_fp16_weights.  The element is
// 16 bits either way: LDS images and swizzles, DMA address maps, the vmcnt / barrier discipline, the XCD order, the accumulation order and
// the staged write-back are the same bytes and the same instructions, and the bank arguments above are not re-argued.
#pragma once
// (included by net.hip INSIDE namespace agz, after conv_bf16.hpp: BF16_*, Bf16Args' helpers bf16_pack2 / bf16_sync / bf16_unit)

#define BF16A_FN __attribute__((target("no-packed-fp32-ops")))
typedef __attribute__((address_space(3))) void* bf16a_lds_ptr_t;

struct Bf16aArgs {
  const float* x;             // fp32 padded NHWC [B][Hp][Wp][Kp]: the input of block 0 (!IN_BF16)
  float* y;                   //                                  the output of the last block (!OUT_BF16)
  const unsigned short* xh;   // bf16 padded NHWC [B][Hp][Wp][Kp] (IN_BF16)
  unsigned short* yh;         //                                  (OUT_BF16)
  const f32x4* ep;            // {sa, ta, sb, tb} [HW][Kp]
  const unsigned short* wq;   // agz_net::build_bf16_weights image
  int HW, W, Wp, HpWp, Kp;
  int n_ntiles, m_per_board, rows_tile, ncc;
};

// the epilogue of one output element, e = {sa, ta, sb, tb}: relu(relu(bn a) + relu(bn b)) in fp32 (shared with conv_bf16s.hpp)
BF16A_FN __device__ __forceinline__ float bf16_dual_ep(float xa, float xb, f32x4 e) {
  float va = xa * e.x + e.y;
  float vb = xb * e.z + e.w;
  va = va > 0.f ? va : 0.f;
  vb = vb > 0.f ? vb : 0.f;
  const float t = va + vb;
  return t > 0.f ? t : 0.f;
}

constexpr int BF16A_ROUNDS = BF16_SP_MAX * 8 / 256;   // DMA rounds of a whole activation stage: 14
static_assert(BF16A_ROUNDS * 256 == BF16_SP_MAX * 8 && BF16A_ROUNDS <= 18, "a stage is a whole number of rounds, at most two per tap");

template <typename E, bool IN_BF16, bool OUT_BF16>
BF16A_FN __global__ __launch_bounds__(256, 1) void conv3x3_bf16a_dual_kernel(Bf16aArgs a) {
  typedef typename E::frag frag_t;
  // four objects, not one array: see `completion` above
  __shared__ __attribute__((aligned(16))) unsigned char ldsA0[BF16_A_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsA1[BF16_A_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB0[BF16_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB1[BF16_B_STAGE];

  // XCD-aware order, tile -> (board, run, n-tile): conv3x3_bf16_dual_kernel's
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

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nit = a.ncc * 9;
  const unsigned dma_w = (unsigned)wid * 1024u;            // the wave's 1 KB of a 4 KB DMA round (the hardware adds 16 lane)

  // weights: the n-tile's [chunk][tap][16 KB] run of wq; lane offset 16 tid, (step, round) in the scalar offset
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.wq) + (size_t)n_tile * nit * (BF16_B_STAGE / 2), 0, nit * BF16_B_STAGE, 0x00020000);
  const unsigned wvo = (unsigned)tid * 16u;
#define BF16A_DMA_B(IT, DST)                                                                                              \
  _Pragma("unroll") for (int j_ = 0; j_ < 4; j_++)                                                                        \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (bf16a_lds_ptr_t)((DST) + j_ * 4096 + dma_w), 16, wvo,                   \
                                             (unsigned)(IT) * (unsigned)BF16_B_STAGE + j_ * 4096u, 0, 0);

  // bf16 activations: the slice's pixels [pbase, pbase + SP) of board b; round r brings LDS units 256 r + tid
  const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.xh) + (IN_BF16 ? ((size_t)b * a.HpWp + pbase) * a.Kp : 0), 0, IN_BF16 ? SP * a.Kp * 2 : 0, 0x00020000);
  // q / Wp for q < BF16_SP_MAX by multiply and shift: with m = 2^20 / Wp + 1, (q m) >> 20 is exact while q (m Wp - 2^20) < 2^20;
  // m Wp - 2^20 <= Wp and q Wp < 448 x 149 (three haloed lines fit the stage: Wp <= BF16_SP_MAX / 3)
  const unsigned wp_magic = (1u << 20) / (unsigned)a.Wp + 1u;
#define BF16A_DMA_A(R, CC, DST)                                                                                           \
  {                                                                                                                       \
    const int idx_ = (R) * 256 + tid;                                                                                     \
    if (idx_ < SP * 8) {                                                                                                  \
      const unsigned q_ = (unsigned)idx_ >> 3, s_ = (unsigned)idx_ & 7u;                                                  \
      const unsigned f_ = ((q_ + (unsigned)pbase - 2u * ((unsigned)line0 + ((q_ * wp_magic) >> 20))) >> 1) & 7u;         \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr_, (bf16a_lds_ptr_t)((DST) + (R) * 4096 + dma_w), 16,                    \
                                               q_ * (unsigned)a.Kp * 2u + ((s_ ^ f_) << 4), (unsigned)(CC) * 128u, 0, 0); \
    }                                                                                                                     \
  }

  // fp32 activations (block 0): conv_bf16.hpp's staging — two 32-byte units per thread and tap through registers
  const char* xb = reinterpret_cast<const char*>(a.x + (IN_BF16 ? 0 : ((size_t)b * a.HpWp + pbase) * a.Kp));
  f32x4 ra[2][2];
  bool av[2];
  unsigned ag[2], al[2];
#define BF16A_LOAD_A(T, CC)                                                                      \
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
#define BF16A_STORE_A(DST)                                                                       \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; s_++)                                               \
    if (av[s_]) {                                                                                \
      u32x4_t v_ = {E::pack2(ra[s_][0].x, ra[s_][0].y), E::pack2(ra[s_][0].z, ra[s_][0].w),      \
                    E::pack2(ra[s_][1].x, ra[s_][1].y), E::pack2(ra[s_][1].z, ra[s_][1].w)};     \
      *reinterpret_cast<u32x4_t*>((DST) + al[s_]) = v_;                                          \
    }
// this wave's DMA has landed (vmcnt = 0; expcnt and lgkmcnt left alone), then every wave's: the barrier
#define BF16A_STEP_END()                \
  __builtin_amdgcn_s_waitcnt(0x0f70);   \
  bf16_sync();

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

  // prologue: the first weight tile and chunk 0 of the slice
  BF16A_DMA_B(0, ldsB0)
  if (IN_BF16) {
#pragma unroll
    for (int r = 0; r < BF16A_ROUNDS; r++) BF16A_DMA_A(r, 0, ldsA0)
  } else {
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
          *reinterpret_cast<u32x4_t*>(ldsA0 + pl[t]) = v;
        }
    }
  }
  BF16A_STEP_END()

  // One (chunk, tap) step.  SB, the weight stage of the step, and the activation stage of the chunk are compile-time constants where
  // the macro is used: every LDS access of a step names its stage.
#define BF16A_FRAGS(S, KS)                                                                                                \
  {                                                                                                                       \
    const unsigned u_ = (unsigned)(2 * (KS) + half);                                                                      \
    _Pragma("unroll") for (int i = 0; i < 3; i++)                                                                         \
      A_[S][i] = *reinterpret_cast<const frag_t*>(Ac + aoff[i] + ((u_ ^ asw[i]) << 4));                                   \
    _Pragma("unroll") for (int jb = 0; jb < 4; jb++)                                                                      \
      B_[S][jb] = *reinterpret_cast<const frag_t*>(Bc + jb * 4096 + brow + ((u_ ^ bsw) << 4));                            \
  }
#define BF16A_STEP(TAP, SB)                                                                                               \
  {                                                                                                                       \
    const int tap = (TAP), it = cc * 9 + tap;                                                                             \
    const unsigned char* const Bc = (SB) ? ldsB1 : ldsB0;                                                                 \
    unsigned char* const Bn = (SB) ? ldsB0 : ldsB1;                                                                       \
    /* the next step's operands leave for the other stages before this step's MFMAs (those stages were last read a */     \
    /* whole step / chunk ago, before the barrier that ended it) */                                                       \
    if (it + 1 < nit) { BF16A_DMA_B(it + 1, Bn) }                                                                         \
    if (more_a) {                                                                                                         \
      if (IN_BF16) {                                                                                                      \
        BF16A_DMA_A(tap, cc + 1, An)                                                                                      \
        if (tap + 9 < BF16A_ROUNDS) BF16A_DMA_A(tap + 9, cc + 1, An)                                                      \
      } else {                                                                                                            \
        BF16A_LOAD_A(tap, cc + 1)                                                                                         \
      }                                                                                                                   \
    }                                                                                                                     \
    const int ky = tap / 3, kx = tap - 3 * ky;                                                                            \
    const int tapoff = ky * a.Wp + kx, tapsw = kx + a.W * ky;                                                             \
    unsigned aoff[3], asw[3];                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 3; i++) {                                                                       \
      aoff[i] = (unsigned)(prel[i] + tapoff) * 128u;                                                                      \
      asw[i] = (unsigned)((mrow[i] + tapsw) >> 1) & 7u;                                                                   \
    }                                                                                                                     \
    frag_t A_[2][3], B_[2][4];   /* two sets: step ks + 1's reads under step ks's MFMAs */                                \
    BF16A_FRAGS(0, 0)                                                                                                     \
    _Pragma("unroll") for (int ks = 0; ks < 4; ks++) {                                                                    \
      if (ks < 3) BF16A_FRAGS((ks + 1) & 1, ks + 1)                                                                       \
      _Pragma("unroll") for (int i = 0; i < 3; i++)                                                                       \
        _Pragma("unroll") for (int j = 0; j < 2; j++)                                                                     \
          _Pragma("unroll") for (int br = 0; br < 2; br++)                                                                \
            acc[i][j][br] = E::mfma(A_[ks & 1][i], B_[ks & 1][br * 2 + j], acc[i][j][br]);                                \
    }                                                                                                                     \
    if (!IN_BF16 && more_a) { BF16A_STORE_A(An) }                                                                         \
    BF16A_STEP_END()                                                                                                      \
  }

  // chunks in pairs: chunk cc uses activation stage cc & 1 = sa, step 9 cc + tap weight stage (sa + tap) & 1
#pragma unroll 1
  for (int cc0 = 0; cc0 < a.ncc; cc0 += 2) {
#pragma unroll
    for (int sa = 0; sa < 2; sa++) {
      const int cc = cc0 + sa;
      if (cc < a.ncc) {
        const unsigned char* const Ac = sa ? ldsA1 : ldsA0;
        unsigned char* const An = sa ? ldsA0 : ldsA1;
        const bool more_a = cc + 1 < a.ncc;
#pragma unroll 1
        for (int t2 = 0; t2 < 8; t2 += 2) {
          BF16A_STEP(t2, sa)
          BF16A_STEP(t2 + 1, sa ^ 1)
        }
        BF16A_STEP(8, sa)
      }
    }
  }
#undef BF16A_STEP
#undef BF16A_FRAGS
#undef BF16A_DMA_A
#undef BF16A_DMA_B
#undef BF16A_LOAD_A
#undef BF16A_STORE_A
#undef BF16A_STEP_END

  // epilogue: BN(scale, shift) + ReLU per branch, add, ReLU; interior of the padded NHWC output
  unsigned char* const stg = ldsA0 + wid * (96 * 128);   // OUT_BF16: this wave's [96 rows][64 channels] bf16 (both A stages are dead)
  float* yb = a.y + (OUT_BF16 ? 0 : (size_t)b * a.HpWp * a.Kp);
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int rh = 0; rh < 2; rh++) {
      // the parameters of eight rows leave together (rows past the end load the last row's), as in conv_bf16.hpp
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
        const int lr = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;      // row inside the wave's 96
        const int m = m0 + wid * 96 + lr;
        float s[2];
#pragma unroll
        for (int j = 0; j < 2; j++) s[j] = bf16_dual_ep(acc[i][j][0][r], acc[i][j][1][r], e[rr][j]);
        if (OUT_BF16) {
          // rows past the end are staged too (their own rows of the wave's region) and never stored
          const unsigned pk = E::pack2(s[0], s[1]);                   // channels lane & 31 and 32 + (lane & 31)
          const unsigned g = (unsigned)((lr >> 2) & 1) << 2, c = (unsigned)(lane & 31);
          unsigned char* row = stg + lr * 128 + ((c & 7u) << 1);
          *reinterpret_cast<unsigned short*>(row + (((c >> 3) ^ g) << 4)) = (unsigned short)pk;
          *reinterpret_cast<unsigned short*>(row + ((((c >> 3) + 4u) ^ g) << 4)) = (unsigned short)(pk >> 16);
        } else if (m < mend) {
          const int h = m / a.W, w = m - h * a.W;
          const unsigned obase = (unsigned)((h + 1) * a.Wp + (w + 1)) * (unsigned)a.Kp;
#pragma unroll
          for (int j = 0; j < 2; j++) yb[obase + n_tile * 64 + j * 32 + (lane & 31)] = s[j];
        }
      }
    }
  }
  if (OUT_BF16) {
    // the wave reads back what its own lanes wrote: LDS serves a wave's accesses in order, the fence keeps the compiler from reordering
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned char* yhb = reinterpret_cast<unsigned char*>(a.yh) + (size_t)b * a.HpWp * a.Kp * 2 + (size_t)n_tile * 128;
#pragma unroll
    for (int t = 0; t < 12; t++) {
      const int lr = t * 8 + (lane >> 3), sl = lane & 7;
      const int m = m0 + wid * 96 + lr;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(stg + lr * 128 + sl * 16);
      if (m < mend) {
        const int h = m / a.W, w = m - h * a.W;
        const unsigned u = (unsigned)sl ^ ((unsigned)((lr >> 2) & 1) << 2);
        *reinterpret_cast<u32x4_t*>(yhb + (unsigned)((h + 1) * a.Wp + (w + 1)) * (unsigned)a.Kp * 2u + u * 16u) = v;
      }
    }
  }
}
#undef BF16A_FN
