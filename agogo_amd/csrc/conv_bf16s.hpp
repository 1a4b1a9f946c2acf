// The small-batch form of conv_bf16a.hpp's block (AGZ_COMPUTE_BF16_ACT with agz_net_set_bf16_small_batch): the same declared arithmetic
// (`bf16-tower`), the same results bit for bit, one board split over many workgroups so that 1 to about 32 boards
// fill the chip.  DESIGN.md section 4h.
//
// Why the bits are the same.  K is never split: every output element is ONE accumulator that starts at zero and sums in the order
// (64-channel chunk, tap, 16-channel step) with v_mfma_f32_32x32x16_bf16 — where the element sits in a wave's tile, which wave and which
// workgroup hold it do not enter the arithmetic.  The operands are the same bf16 values (the weight image is conv_bf16.hpp's, block 0
// rounds its fp32 input with the same v_cvt_pk_bf16_f32), the epilogue is bf16_dual_ep and bf16_pack2 of conv_bf16a.hpp / conv_bf16.hpp.
//
// Work split.  A workgroup owns one board, a run of RB row blocks of 32 GEMM rows (RB = 1, 2 or 4 = blockDim.x / 64: one wave per row
// block) and one 64-column tile [32 branch-a | 32 branch-b].  A wave owns 32 rows x 64 columns = two accumulator tiles, the a and b
// results of the SAME 32 channels, so the dual epilogue stays inside a lane; per 16-channel step it reads one A and two B fragments for
// two MFMAs.  19x19 / K=256: 12 row blocks x 8 column tiles = 96 wave tiles per board.  Tiles are dealt in conv_bf16a.hpp's XCD-aware
// order: the column tiles of one run are consecutive, so they share an L2.
//
// LDS: 2 x 32 KB activation stages + 2 x 8 KB weight stages = 80 KB, half a CU's, two workgroups per CU.
//   A stage   the run's lines plus one on either side, halo columns included, of one 64-channel chunk: conv_bf16.hpp's image,
//             128 p + 16 (u ^ f(p)), f(p) = ((p - 2 line(p)) >> 1) & 7, p counted from the slice's first pixel — the fragment reads and their
//             bank argument are that file's.  RB = 4 at 19x19: at most 10 lines x 21 pixels = 26.3 KB of the 32 (BF16S_SP_MAX = 256 pixels).
//   B stage   [64 columns][64 channels] bf16: rows 0..31 branch a, 32..63 branch b.  Tile n64 = 2 n_tile + j is two contiguous 4 KB pieces
//             of the 16 KB image wq[n_tile][chunk][tap]: its rows 32 j .. 32 j + 31 and 64 + 32 j .. 64 + 32 j + 31.  The image's swizzle
//             (nn >> 1) & 7 does not change when nn moves by a multiple of 16, so each piece lands lane-linearly in bank order: a fragment
//             read's 16 lanes hold 16 consecutive rows nn and one unit u — 8 even and 8 odd rows (slot bit 3 = nn & 1), and within a parity
//             nn >> 1 runs through 8 consecutive values: 16 different slots.  No second weight image, no device memory of its own.
// DMA.  conv_bf16a.hpp's address maps with a round of blockDim.x lanes x 16 bytes: round r of a stage fills LDS units r blockDim.x + tid,
// lane -> (pixel q, slot s) fetches global unit s ^ f; lanes past the slice are masked (and the buffer resource ends at the slice).  A
// stage of BF16S_SP_MAX pixels is at most 32 rounds of one wave: tap t of chunk c issues rounds 4 t .. 4 t + 3 of chunk c + 1, the weight
// tile of the next step goes in 4 / RB rounds per piece.  Block 0 (fp32 in) stages the same units through registers.  Completion is
// conv_bf16a.hpp's rule: every wave waits for its own DMA before the barrier that ends a step, nothing is in flight across a barrier;
// four separate __shared__ objects, chunk and tap loops unrolled by two.  With RB = 1 the barrier is a wave's own.
// Ragged M: rows past the run or the board clamp to the last pixel for the reads and are never stored (a wave whose whole row block lies
// past the board still takes its part of the DMA and the barriers).
// Output: bf16 goes through the wave's own 2 KB of the dead stage A0 ([32 rows][32 channels]: a two-way conflict on 16 two-byte writes,
// left alone) and leaves as 16-byte stores, a pixel's 32 channels = 64 contiguous bytes; the last block stores fp32 as conv_bf16.hpp does.
//
// Element type E (conv_bf16.hpp): Fp16El is the small-batch form of AGZ_COMPUTE_FP16, equal bit for bit to that mode's whole-board kernel
// by the argument above with E::mfma and E::pack2 in the places of the bf16 instructions.  The element is 16 bits either way: the stages,
// the DMA maps, the completion rule and the write-back are the same bytes and the same instructions.
#pragma once
// (included by net.hip INSIDE namespace agz, after conv_bf16a.hpp: Bf16aArgs, bf16a_lds_ptr_t, bf16_dual_ep, bf16_pack2 / bf16_sync / bf16_unit)

#define BF16S_FN __attribute__((target("no-packed-fp32-ops")))

constexpr int BF16S_SP_MAX = 256;                 // haloed pixels of a staged slice
constexpr int BF16S_A_STAGE = BF16S_SP_MAX * 128;
constexpr int BF16S_B_STAGE = 64 * 128;           // [64 columns][64 channels] bf16
constexpr int BF16S_TAP_ROUNDS = 4;               // rounds of a stage a tap brings
static_assert(2 * (BF16S_A_STAGE + BF16S_B_STAGE) <= 80 * 1024, "two workgroups per CU");
static_assert(9 * BF16S_TAP_ROUNDS * 64 >= BF16S_SP_MAX * 8, "nine taps of one wave bring a whole stage");

// Bf16aArgs with the small form's split: n_ntiles = Kp / 32 column tiles, rows_tile = 32 RB, m_per_board = runs of a board
template <typename E, bool IN_BF16, bool OUT_BF16>
BF16S_FN __global__ __launch_bounds__(256, 2) void conv3x3_bf16s_dual_kernel(Bf16aArgs a) {
  typedef typename E::frag frag_t;
  __shared__ __attribute__((aligned(16))) unsigned char ldsA0[BF16S_A_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsA1[BF16S_A_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB0[BF16S_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB1[BF16S_B_STAGE];

  // XCD-aware order, tile -> (board, run, column tile): conv3x3_bf16_dual_kernel's
  const int nblk = gridDim.x, id = blockIdx.x;
  const int xq = nblk >> 3, xr = nblk & 7, xcd = id & 7, slot = id >> 3;
  const int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + slot;
  const int n64 = tile % a.n_ntiles, bm = tile / a.n_ntiles;
  const int b = bm / a.m_per_board, mt = bm - b * a.m_per_board;
  const int m0 = mt * a.rows_tile;
  const int mend = m0 + a.rows_tile < a.HW ? m0 + a.rows_tile : a.HW;           // rows [m0, mend) of board b
  const int line0 = m0 / a.W, line1 = (mend - 1) / a.W;
  const int SP = (line1 - line0 + 3) * a.Wp;               // haloed pixels staged (<= BF16S_SP_MAX, checked by the launcher)
  const int pbase = line0 * a.Wp;                          // first of them in the board's padded image

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int nthr = blockDim.x;                             // 64 RB: the lanes of a DMA round
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nit = a.ncc * 9;
  const unsigned dma_w = (unsigned)wid * 1024u;            // the wave's 1 KB of a round (the hardware adds 16 lane)

  // weights: the [chunk][tap][16 KB] run of the 128-column tile n64 / 2; this tile's pieces are at 4096 j and 8192 + 4096 j of a step
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.wq) + (size_t)(n64 >> 1) * nit * (BF16_B_STAGE / 2), 0, nit * BF16_B_STAGE, 0x00020000);
  const unsigned wvo = (unsigned)tid * 16u, wpc = (unsigned)(n64 & 1) * 4096u;
#define BF16S_DMA_B(IT, DST)                                                                                              \
  for (unsigned k_ = 0; k_ < 4096u; k_ += (unsigned)nthr * 16u)                                                           \
    _Pragma("unroll") for (unsigned p_ = 0; p_ < 2; p_++)                                                                 \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (bf16a_lds_ptr_t)((DST) + p_ * 4096u + k_ + dma_w), 16, wvo,           \
                                               (unsigned)(IT) * (unsigned)BF16_B_STAGE + p_ * 8192u + wpc + k_, 0, 0);

  // bf16 activations: the slice's pixels [pbase, pbase + SP) of board b; round r brings LDS units r nthr + tid
  const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.xh) + (IN_BF16 ? ((size_t)b * a.HpWp + pbase) * a.Kp : 0), 0, IN_BF16 ? SP * a.Kp * 2 : 0, 0x00020000);
  // q / Wp for q < BF16S_SP_MAX by multiply and shift, as in conv_bf16a.hpp (q Wp < 256 x 86: three haloed lines fit the stage)
  const unsigned wp_magic = (1u << 20) / (unsigned)a.Wp + 1u;
#define BF16S_DMA_A(T, CC, DST)                                                                                           \
  _Pragma("unroll") for (int s4_ = 0; s4_ < BF16S_TAP_ROUNDS; s4_++) {                                                    \
    const int r_ = BF16S_TAP_ROUNDS * (T) + s4_;                                                                          \
    const int idx_ = r_ * nthr + tid;                                                                                     \
    if (idx_ < SP * 8) {                                                                                                  \
      const unsigned q_ = (unsigned)idx_ >> 3, s_ = (unsigned)idx_ & 7u;                                                  \
      const unsigned f_ = ((q_ + (unsigned)pbase - 2u * ((unsigned)line0 + ((q_ * wp_magic) >> 20))) >> 1) & 7u;         \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr_, (bf16a_lds_ptr_t)((DST) + (unsigned)(r_ * nthr) * 16u + dma_w), 16,   \
                                               q_ * (unsigned)a.Kp * 2u + ((s_ ^ f_) << 4), (unsigned)(CC) * 128u, 0, 0); \
    }                                                                                                                     \
  }

  // fp32 activations (block 0): the same units through registers, conv_bf16.hpp's load / v_cvt_pk / ds_write staging
  const char* xb = reinterpret_cast<const char*>(a.x + (IN_BF16 ? 0 : ((size_t)b * a.HpWp + pbase) * a.Kp));
  f32x4 ra[BF16S_TAP_ROUNDS][2];
  bool av[BF16S_TAP_ROUNDS];
  unsigned al[BF16S_TAP_ROUNDS];
#define BF16S_LOAD_A(T, CC)                                                                      \
  _Pragma("unroll") for (int s_ = 0; s_ < BF16S_TAP_ROUNDS; s_++) {                              \
    const int idx_ = (BF16S_TAP_ROUNDS * (T) + s_) * nthr + tid;                                 \
    unsigned ag_;                                                                                \
    av[s_] = idx_ < SP * 8;                                                                      \
    bf16_unit(av[s_] ? idx_ : 0, pbase, a.Wp, a.Kp, ag_, al[s_]);                                \
    if (av[s_]) {                                                                                \
      const char* g_ = xb + ag_ + (unsigned)(CC) * 256u;                                         \
      ra[s_][0] = *reinterpret_cast<const f32x4*>(g_);                                          \
      ra[s_][1] = *reinterpret_cast<const f32x4*>(g_ + 16);                                     \
    }                                                                                            \
  }
#define BF16S_STORE_A(DST)                                                                       \
  _Pragma("unroll") for (int s_ = 0; s_ < BF16S_TAP_ROUNDS; s_++)                                \
    if (av[s_]) {                                                                                \
      u32x4_t v_ = {E::pack2(ra[s_][0].x, ra[s_][0].y), E::pack2(ra[s_][0].z, ra[s_][0].w),      \
                    E::pack2(ra[s_][1].x, ra[s_][1].y), E::pack2(ra[s_][1].z, ra[s_][1].w)};     \
      *reinterpret_cast<u32x4_t*>((DST) + al[s_]) = v_;                                          \
    }
// this wave's DMA has landed (vmcnt = 0; expcnt and lgkmcnt left alone), then every wave's: the barrier
#define BF16S_STEP_END()                \
  __builtin_amdgcn_s_waitcnt(0x0f70);   \
  bf16_sync();

  // fragment row of this lane: row block wid of the run, row lane & 31 -> top-left pixel of its 3x3 window inside the slice
  const int mb = m0 + wid * 32;
  int mrow = mb + (lane & 31);
  if (mrow >= mend) mrow = mend - 1;
  const int prel = (mrow / a.W - line0) * a.Wp + mrow % a.W;
  const unsigned bsw = (unsigned)((lane & 31) >> 1) & 7u;
  const unsigned brow = (unsigned)(lane & 31) * 128u;

  f32x16 acc[2];   // [branch]
#pragma unroll
  for (int br = 0; br < 2; br++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[br][r] = 0.f;

  // prologue: the first weight tile and chunk 0 of the slice
  BF16S_DMA_B(0, ldsB0)
#pragma unroll 1
  for (int t = 0; t < 9 && BF16S_TAP_ROUNDS * t * nthr < SP * 8; t++) {
    if (IN_BF16) {
      BF16S_DMA_A(t, 0, ldsA0)
    } else {
      BF16S_LOAD_A(t, 0)
      BF16S_STORE_A(ldsA0)
    }
  }
  BF16S_STEP_END()

  // One (chunk, tap) step; the weight stage of the step and the activation stage of the chunk are compile-time constants where the
  // macro is used, as in conv_bf16a.hpp
#define BF16S_FRAGS(S, KS)                                                                                                \
  {                                                                                                                       \
    const unsigned u_ = (unsigned)(2 * (KS) + half);                                                                      \
    A_[S] = *reinterpret_cast<const frag_t*>(Ac + aoff + ((u_ ^ asw) << 4));                                              \
    _Pragma("unroll") for (int br = 0; br < 2; br++)                                                                      \
      B_[S][br] = *reinterpret_cast<const frag_t*>(Bc + br * 4096 + brow + ((u_ ^ bsw) << 4));                            \
  }
#define BF16S_STEP(TAP, SB)                                                                                               \
  {                                                                                                                       \
    const int tap = (TAP), it = cc * 9 + tap;                                                                             \
    const unsigned char* const Bc = (SB) ? ldsB1 : ldsB0;                                                                 \
    unsigned char* const Bn = (SB) ? ldsB0 : ldsB1;                                                                       \
    /* the next step's operands leave for the other stages before this step's MFMAs (those stages were last read a */     \
    /* whole step / chunk ago, before the barrier that ended it) */                                                       \
    if (it + 1 < nit) { BF16S_DMA_B(it + 1, Bn) }                                                                         \
    if (more_a) {                                                                                                         \
      if (IN_BF16) {                                                                                                      \
        BF16S_DMA_A(tap, cc + 1, An)                                                                                      \
      } else {                                                                                                            \
        BF16S_LOAD_A(tap, cc + 1)                                                                                         \
      }                                                                                                                   \
    }                                                                                                                     \
    const int ky = tap / 3, kx = tap - 3 * ky;                                                                            \
    const unsigned aoff = (unsigned)(prel + ky * a.Wp + kx) * 128u;                                                       \
    const unsigned asw = (unsigned)((mrow + kx + a.W * ky) >> 1) & 7u;                                                    \
    frag_t A_[2], B_[2][2];   /* two sets: step ks + 1's reads under step ks's MFMAs */                                   \
    BF16S_FRAGS(0, 0)                                                                                                     \
    _Pragma("unroll") for (int ks = 0; ks < 4; ks++) {                                                                    \
      if (ks < 3) BF16S_FRAGS((ks + 1) & 1, ks + 1)                                                                       \
      _Pragma("unroll") for (int br = 0; br < 2; br++)                                                                    \
        acc[br] = E::mfma(A_[ks & 1], B_[ks & 1][br], acc[br]);                                                           \
    }                                                                                                                     \
    if (!IN_BF16 && more_a) { BF16S_STORE_A(An) }                                                                         \
    BF16S_STEP_END()                                                                                                      \
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
          BF16S_STEP(t2, sa)
          BF16S_STEP(t2 + 1, sa ^ 1)
        }
        BF16S_STEP(8, sa)
      }
    }
  }
#undef BF16S_STEP
#undef BF16S_FRAGS
#undef BF16S_DMA_A
#undef BF16S_DMA_B
#undef BF16S_LOAD_A
#undef BF16S_STORE_A
#undef BF16S_STEP_END

  // epilogue: conv_bf16a.hpp's, one 32-channel group per lane; interior of the padded NHWC output
  const unsigned c = (unsigned)(n64 * 32 + (lane & 31));
  unsigned char* const stg = ldsA0 + wid * 2048;   // OUT_BF16: this wave's [32 rows][32 channels] bf16 (both A stages are dead)
  float* yb = a.y + (OUT_BF16 ? 0 : (size_t)b * a.HpWp * a.Kp);
#pragma unroll
  for (int rh = 0; rh < 2; rh++) {
    // the parameters of eight rows leave together (rows past the end load the last row's), as in conv_bf16.hpp
    f32x4 e[8];
    float s[8];
#pragma unroll
    for (int rr = 0; rr < 8; rr++) {
      const int r = rh * 8 + rr;
      const int m = mb + (r & 3) + 8 * (r >> 2) + 4 * half;
      e[rr] = a.ep[(unsigned)(m < mend ? m : mend - 1) * (unsigned)a.Kp + c];
    }
#pragma unroll
    for (int rr = 0; rr < 8; rr++) s[rr] = bf16_dual_ep(acc[0][rh * 8 + rr], acc[1][rh * 8 + rr], e[rr]);
#pragma unroll
    for (int rr = 0; rr < 8; rr++) {
      const int r = rh * 8 + rr;
      const int lr = (r & 3) + 8 * (r >> 2) + 4 * half;      // row inside the wave's 32
      if (OUT_BF16) {
        // rows past the end are staged too (their own rows of the wave's region) and never stored; rows r, r + 1 in one conversion
        if ((rr & 1) == 0) {
          const unsigned pk = E::pack2(s[rr], s[rr + 1]);
          unsigned char* p = stg + lr * 64 + ((lane & 31) << 1);
          *reinterpret_cast<unsigned short*>(p) = (unsigned short)pk;
          *reinterpret_cast<unsigned short*>(p + 64) = (unsigned short)(pk >> 16);
        }
      } else if (mb + lr < mend) {
        const int m = mb + lr, h = m / a.W, w = m - h * a.W;
        yb[(unsigned)((h + 1) * a.Wp + (w + 1)) * (unsigned)a.Kp + c] = s[rr];
      }
    }
  }
  if (OUT_BF16) {
    // the wave reads back what its own lanes wrote: LDS serves a wave's accesses in order, the fence keeps the compiler from reordering
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned char* yhb = reinterpret_cast<unsigned char*>(a.yh) + (size_t)b * a.HpWp * a.Kp * 2 + (size_t)n64 * 64;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int lr = t * 16 + (lane >> 2), sl = lane & 3;
      const int m = mb + lr;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(stg + lr * 64 + sl * 16);
      if (m < mend) {
        const int h = m / a.W, w = m - h * a.W;
        *reinterpret_cast<u32x4_t*>(yhb + (unsigned)((h + 1) * a.Wp + (w + 1)) * (unsigned)a.Kp * 2u + (unsigned)sl * 16u) = v;
      }
    }
  }
}
#undef BF16S_FN
