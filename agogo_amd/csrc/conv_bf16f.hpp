// The few-boards form of conv_bf16a.hpp's block (AGZ_COMPUTE_BF16_ACT / AGZ_COMPUTE_FP16 with agz_net_set_bf16_small_batch =
// AGZ_BF16_SMALL_FEW_*): the same declared arithmetic (`bf16-tower` / `fp16-tower`), the same results bit for bit,
// built for ONE to a few boards, where a launch costs what its longest wave costs.  DESIGN.md section 4k.
//
// Why the bits are the same (the invariant of conv_bf16s.hpp, kept).  K is never split: every output element is ONE accumulator that
// starts at zero and sums in the order (64-channel chunk, tap, 16-channel step) with E::mfma (v_mfma_f32_32x32x16_bf16 / _f16) — which
// wave and which workgroup hold the element does not enter the arithmetic.  The operands are the weight image wq16(l) (no second image, no
// device memory of the form's own) and the same 16-bit activations (block 0 rounds its fp32 input with conv_bf16.hpp's E::pack2); the
// epilogue is bf16_dual_ep / E::pack2 on the same ep16(l).  No other MFMA shape is used.
//
// Work split.  A workgroup owns one board, a run of RB row blocks of 32 GEMM rows (RB = 1, 2 or 4) and one 64-column tile
// [32 branch-a | 32 branch-b], conv_bf16s.hpp's B-stage layout.  It has 2 RB waves: wave 2 k + br owns ONE 32 x 32 accumulator tile, row
// block k x the 32 channels of branch br, so a wave chains 9 ncc x 4 MFMAs (144 at K = 256) where a wave of the small form chains 288.
// Tiles are dealt in conv_bf16a.hpp's XCD-aware order: the column tiles of one run are consecutive and share an L2.
//
// LDS: 108 KB resident slice + 6 x 8 KB weight ring = 156 KB, one workgroup per CU.
//   slice   the run's lines plus one on either side, halo columns included, of ALL ncc chunks, brought in once: chunk c is
//           conv_bf16.hpp's image at c SP 128 — 128 p + 16 (u ^ f(p)), f(p) = ((p - 2 line(p)) >> 1) & 7, p counted from the slice's first
//           pixel — so the A-fragment reads and their bank argument are that file's.  SP ncc <= BF16F_SPC_MAX = 864 (19x19 / K = 256: RB = 4,
//           at most 10 lines x 21 pixels x 4 chunks = 840); the launcher takes the largest RB of 4, 2, 1 that fits, and where RB = 1 does
//           not fit (19x19 from K = 576) the form does not apply.
//   ring    stage s holds the weight tile of steps it = s (mod 6): conv_bf16s.hpp's [64 columns][64 channels] tile, the two 4 KB pieces of
//           the 16 KB image wq[n_tile][chunk][tap]; the bank argument of the B-fragment reads is that file's.
// DMA (raw_ptr_buffer_load_lds, 16 bytes per lane, conv_bf16s.hpp's address maps with a round of blockDim.x lanes).  The prologue issues
// the weight tiles of steps 0 .. 5 and the whole slice in one burst, waits once (vmcnt(0)) and ends with a full bf16_sync(): block 0's
// slice is written by ds_write from every wave, so that barrier also follows lgkmcnt(0).  Step `it` >= 1 then: (1) waits until ITS OWN share of
// tile `it` has landed — a counted s_waitcnt vmcnt(n), n = the loads this wave issued after that share, NL min(4, nit - 1 - it) with
// NL = 512 / blockDim.x loads per wave and tile — (2) passes the workgroup barrier, (3) issues tile it + 5 into the stage of tile it - 1,
// (4) reads its fragments of tile `it` and multiplies (step 0: (4) alone, behind the prologue's barrier).  Up to five tiles are in flight across a barrier.
// The pipeline rule, which replaces "nothing is in flight across a barrier" of the other forms:
//   * a stage is READ only after every wave has waited for its own share of that stage and a barrier has passed  — (1), (2), then (4);
//   * a stage is OVERWRITTEN only by DMA issued after a barrier that follows every wave's last read of it        — the reads of tile
//     it - 1 come before barrier (2) of step `it` in every wave's program, the DMA of (3) after it.
// A wave's vector-memory operations retire in order and an LDS-DMA counts as a load, so the count is exact.  The six stages and the slice
// are seven separate __shared__ objects and the step loop is unrolled by six: every LDS access names its object at compile time, so the
// compiler's own LDS-DMA tracking does not hold a step's ds_reads back for DMA in flight into the other stages — in five steps of six:
// before the B reads of stage 5 the compiler still places an s_waitcnt vmcnt(0) of its own (seen in the assembly of every instantiation,
// not explained; correct, and it drains the ring once per lap).  The step barrier is bf16f_sync(), not bf16_sync(): see there.
// Measured (profiles/bf16_few.md): 20.2 us per block at one board of 19x19 / K = 256 against the small form's 22.3 — a step still costs
// 0.56 us although its tile left five steps earlier, so what a step waits for is its own chain ds_read -> MFMA x 4, not the DMA.
// Block 0 (fp32 in) stages the slice's units through registers in the prologue with E::pack2.
// Hand-over.  The dual epilogue needs a and b of one element: after its last MFMA the b-wave writes its 16 accumulator registers lane-
// linearly into its row block's 4 KB of ring stages 0 / 1 — dead: with six stages the last tile, 9 ncc - 1, sits in stage 2 or 5, every
// other stage was last read before the last step's barrier and no DMA is in flight — ONE barrier, then the a-wave reads them with the
// same lane map and applies the unchanged epilogue.  Output as conv_bf16s.hpp: 16-bit results through the a-wave's own 2 KB of the same
// region and out as 16-byte stores; the last block stores fp32.
// Ragged M: rows past the run or the board clamp to the last pixel for the reads and are never stored (waves of a row block past the
// board still take their part of the DMA and the barriers).
//
// Element type E (conv_bf16.hpp): Fp16El is the few-boards form of AGZ_COMPUTE_FP16; 16 bits either way, the same bytes and instructions.
#pragma once
// (included by net.hip INSIDE namespace agz, after conv_bf16s.hpp: Bf16aArgs, bf16a_lds_ptr_t, bf16_dual_ep, bf16_sync / bf16_unit)

#define BF16F_FN __attribute__((target("no-packed-fp32-ops")))

constexpr int BF16F_D = 6;                        // ring stages: tiles are issued D - 1 steps ahead
constexpr int BF16F_SPC_MAX = 864;                // haloed pixels x chunks of a resident slice
constexpr int BF16F_A_BYTES = BF16F_SPC_MAX * 128;
constexpr int BF16F_B_STAGE = 64 * 128;           // [64 columns][64 channels], conv_bf16s.hpp's
static_assert(BF16F_A_BYTES + BF16F_D * BF16F_B_STAGE <= 160 * 1024, "the slice and the ring fit a CU's LDS");
static_assert(BF16F_D == 6, "the step loop is unrolled by six; the last tile 9 ncc - 1 is 2 or 5 mod 6, never hand-over stage 0 or 1");
static_assert(2 * BF16F_B_STAGE >= 4 * 4096, "the hand-over of four row blocks fits stages 0 and 1");
static_assert(4 * (BF16F_D - 2) <= 63, "vmcnt counts the loads in flight");
static_assert((size_t)BF16F_SPC_MAX * (BF16F_SPC_MAX / 3) < (1u << 20), "q / Wp by multiply and shift is exact over the slice");

// s_waitcnt vmcnt(n), expcnt and lgkmcnt left alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14)
#define BF16F_VMCNT(N) __builtin_amdgcn_s_waitcnt(0x0f70 | ((N) & 15) | (((N) >> 4) << 14))
// this wave's share of a tile has landed when at most NL x ahead later loads are outstanding; ahead = D - 2 but for the last steps
template <int NL>
BF16F_FN __device__ __forceinline__ void bf16f_wait(int ahead) {
  if (ahead >= BF16F_D - 2) BF16F_VMCNT(NL * (BF16F_D - 2));
  else if (ahead == 3) BF16F_VMCNT(NL * 3);
  else if (ahead == 2) BF16F_VMCNT(NL * 2);
  else if (ahead == 1) BF16F_VMCNT(NL);
  else BF16F_VMCNT(0);
}
// The barrier of steps 1 .. nit - 1: bf16_sync() without its fences.  A workgroup-scope release fence makes the compiler wait for
// vmcnt(0) — the LDS-DMA in flight, which the rule above keeps in flight on purpose.  In these steps the only LDS writes are the DMA's,
// which vmcnt covers, so what the barrier has to order is program order only: the ds_reads of the step before (consumed by its MFMAs,
// so complete) stay before it, the DMA and the ds_reads of this step stay behind it; the empty asm statements are compiler barriers for
// memory operations and emit nothing.  It is NOT enough where ds_writes pass between waves — vmcnt does not count them and nothing waits
// for lgkmcnt before a bare s_barrier: the end of the prologue (block 0 stages its slice with ds_write) and the hand-over use bf16_sync().
BF16F_FN __device__ __forceinline__ void bf16f_sync() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Bf16aArgs with conv_bf16s.hpp's split: n_ntiles = Kp / 32 column tiles, rows_tile = 32 RB, m_per_board = runs of a board; blockDim.x = 128 RB
template <typename E, int RB, bool IN_BF16, bool OUT_BF16>
BF16F_FN __global__ __launch_bounds__(128 * RB, 1) void conv3x3_bf16f_dual_kernel(Bf16aArgs a) {
  typedef typename E::frag frag_t;
  __shared__ __attribute__((aligned(16))) unsigned char ldsA[BF16F_A_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB0[BF16F_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB1[BF16F_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB2[BF16F_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB3[BF16F_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB4[BF16F_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB5[BF16F_B_STAGE];

  // XCD-aware order, tile -> (board, run, column tile): conv3x3_bf16_dual_kernel's
  const int nblk = gridDim.x, id = blockIdx.x;
  const int xq = nblk >> 3, xr = nblk & 7, xcd = id & 7, slot = id >> 3;
  const int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + slot;
  const int n64 = tile % a.n_ntiles, bm = tile / a.n_ntiles;
  const int b = bm / a.m_per_board, mt = bm - b * a.m_per_board;
  const int m0 = mt * a.rows_tile;
  const int mend = m0 + a.rows_tile < a.HW ? m0 + a.rows_tile : a.HW;           // rows [m0, mend) of board b
  const int line0 = m0 / a.W, line1 = (mend - 1) / a.W;
  const int SP = (line1 - line0 + 3) * a.Wp;               // haloed pixels staged (SP ncc <= BF16F_SPC_MAX, checked by the launcher)
  const int pbase = line0 * a.Wp;                          // first of them in the board's padded image
  const unsigned spb = (unsigned)SP * 128u;                // bytes of one chunk's image

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  constexpr int nthr = 128 * RB;                           // the lanes of a DMA round
  constexpr int NL = 512 / nthr;                           // loads of a wave per weight tile: 4, 2, 1
  static_assert(RB == 1 || RB == 2 || RB == 4, "2 RB waves");
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rbk = wid >> 1, br = wid & 1;                  // row block of the run, branch
  const int nit = a.ncc * 9;
  const unsigned dma_w = (unsigned)wid * 1024u;            // the wave's 1 KB of a round (the hardware adds 16 lane)

  // weights: the [chunk][tap][16 KB] run of the 128-column tile n64 / 2; this tile's pieces are at 4096 j and 8192 + 4096 j of a step.
  // Unit g = round x nthr + tid of the 512 of a tile: piece g >> 8, 16-byte unit g & 255 of it; a wave's 64 units lie in one piece.
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.wq) + (size_t)(n64 >> 1) * nit * (BF16_B_STAGE / 2), 0, nit * BF16_B_STAGE, 0x00020000);
  const unsigned wpc = (unsigned)(n64 & 1) * 4096u;
#define BF16F_DMA_B(IT, DST)                                                                                              \
  _Pragma("unroll") for (unsigned g0_ = 0; g0_ < 512u; g0_ += (unsigned)nthr) {                                                           \
    const unsigned g_ = g0_ + (unsigned)tid;                                                                              \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (bf16a_lds_ptr_t)((DST) + g0_ * 16u + dma_w), 16,                        \
                                             (g_ >> 8) * 8192u + wpc + (g_ & 255u) * 16u,                                 \
                                             (unsigned)(IT) * (unsigned)BF16_B_STAGE, 0, 0);                              \
  }

  // prologue: the weight tiles of steps 0 .. D - 1 (every stage is free), then the whole slice, one wait
  if (0 < nit) { BF16F_DMA_B(0, ldsB0) }
  if (1 < nit) { BF16F_DMA_B(1, ldsB1) }
  if (2 < nit) { BF16F_DMA_B(2, ldsB2) }
  if (3 < nit) { BF16F_DMA_B(3, ldsB3) }
  if (4 < nit) { BF16F_DMA_B(4, ldsB4) }
  if (5 < nit) { BF16F_DMA_B(5, ldsB5) }
  if (IN_BF16) {
    // 16-bit activations: the slice's pixels [pbase, pbase + SP) of board b; round r of chunk c brings LDS units r nthr + tid of its image,
    // lane -> (pixel q, slot s) fetches global unit s ^ f(q); lanes past the slice are masked (and the buffer resource ends at the slice)
    const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(a.xh) + ((size_t)b * a.HpWp + pbase) * a.Kp, 0, SP * a.Kp * 2, 0x00020000);
    const unsigned wp_magic = (1u << 20) / (unsigned)a.Wp + 1u;     // q / Wp = (q m) >> 20: exact while q Wp < 2^20 (static_assert above)
#pragma unroll 1
    for (int r0 = 0; r0 < SP * 8; r0 += nthr) {
      const int idx = r0 + tid;
      if (idx < SP * 8) {
        const unsigned q = (unsigned)idx >> 3, s = (unsigned)idx & 7u;
        const unsigned f = ((q + (unsigned)pbase - 2u * ((unsigned)line0 + ((q * wp_magic) >> 20))) >> 1) & 7u;
        const unsigned vo = q * (unsigned)a.Kp * 2u + ((s ^ f) << 4);
#pragma unroll 1
        for (int cc = 0; cc < a.ncc; cc++)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(xr_, (bf16a_lds_ptr_t)(ldsA + (unsigned)cc * spb + (unsigned)r0 * 16u + dma_w), 16, vo,
                                                   (unsigned)cc * 128u, 0, 0);
      }
    }
  } else {
    // fp32 activations (block 0): the same units through registers, conv_bf16.hpp's load / pack / ds_write staging
    const char* xb = reinterpret_cast<const char*>(a.x + ((size_t)b * a.HpWp + pbase) * a.Kp);
#pragma unroll 1
    for (int r0 = 0; r0 < SP * 8; r0 += nthr) {
      const int idx = r0 + tid;
      if (idx < SP * 8) {
        unsigned ag, al;
        bf16_unit(idx, pbase, a.Wp, a.Kp, ag, al);
#pragma unroll 4
        for (int cc = 0; cc < a.ncc; cc++) {
          const char* g = xb + ag + (unsigned)cc * 256u;
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(g), v1 = *reinterpret_cast<const f32x4*>(g + 16);
          u32x4_t v = {E::pack2(v0.x, v0.y), E::pack2(v0.z, v0.w), E::pack2(v1.x, v1.y), E::pack2(v1.z, v1.w)};
          *reinterpret_cast<u32x4_t*>(ldsA + (unsigned)cc * spb + al) = v;
        }
      }
    }
  }
  // the end of the prologue is step 0's wait and barrier: this wave's DMA has landed, then bf16_sync() WITH its fences — block 0's
  // slice went in by ds_write from every wave and is read by every wave, so the barrier has to follow lgkmcnt(0) as well; nothing
  // is in flight here that the fences could hold back
  BF16F_VMCNT(0);
  bf16_sync();

  // fragment row of this lane: row block rbk of the run, row lane & 31 -> top-left pixel of its 3x3 window inside the slice
  const int mb = m0 + rbk * 32;
  int mrow = mb + (lane & 31);
  if (mrow >= mend) mrow = mend - 1;
  const int prel = (mrow / a.W - line0) * a.Wp + mrow % a.W;
  const unsigned bsw = (unsigned)((lane & 31) >> 1) & 7u;
  const unsigned boff = (unsigned)br * 4096u + (unsigned)(lane & 31) * 128u;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;

  // One (chunk, tap) step `it` (uniform; the stage of the tile, SB, and the stage tile it + D - 1 goes to, SN = SB - 1 mod D, are
  // compile-time constants where the macro is used).  The prologue's wait and bf16_sync() stand for step 0's.
#define BF16F_FRAG(S, KS)                                                                                                 \
  {                                                                                                                       \
    const unsigned u_ = (unsigned)(2 * (KS) + half);                                                                      \
    A_[S] = *reinterpret_cast<const frag_t*>(Ac + aoff + ((u_ ^ asw) << 4));                                              \
    B_[S] = *reinterpret_cast<const frag_t*>(Bc + boff + ((u_ ^ bsw) << 4));                                           \
  }
#define BF16F_STEP(IT, SB_, SN_)                                                                                          \
  if ((IT) < nit) {                                                                                                       \
    const int it = (IT);                                                                                                  \
    if (it > 0) {                                                                                                         \
      bf16f_wait<NL>(nit - 1 - it);                                                                                       \
      bf16f_sync();                                                                                                       \
      if (it + BF16F_D - 1 < nit) { BF16F_DMA_B(it + BF16F_D - 1, SN_) }                                                  \
    }                                                                                                                     \
    const int cc = it / 9, tap = it - 9 * cc;                                                                             \
    const int ky = tap / 3, kx = tap - 3 * ky;                                                                            \
    const unsigned char* const Ac = ldsA + (unsigned)cc * spb;                                                            \
    const unsigned char* const Bc = (SB_);                                                                                \
    const unsigned aoff = (unsigned)(prel + ky * a.Wp + kx) * 128u;                                                       \
    const unsigned asw = (unsigned)((mrow + kx + a.W * ky) >> 1) & 7u;                                                    \
    frag_t A_[2], B_[2];   /* two sets: step ks + 1's reads under step ks's MFMA */                                       \
    BF16F_FRAG(0, 0)                                                                                                      \
    _Pragma("unroll") for (int ks = 0; ks < 4; ks++) {                                                                    \
      if (ks < 3) BF16F_FRAG((ks + 1) & 1, ks + 1)                                                                        \
      acc = E::mfma(A_[ks & 1], B_[ks & 1], acc);                                                                         \
    }                                                                                                                     \
  }

#pragma unroll 1
  for (int it0 = 0; it0 < nit; it0 += BF16F_D) {
    BF16F_STEP(it0, ldsB0, ldsB5)
    BF16F_STEP(it0 + 1, ldsB1, ldsB0)
    BF16F_STEP(it0 + 2, ldsB2, ldsB1)
    BF16F_STEP(it0 + 3, ldsB3, ldsB2)
    BF16F_STEP(it0 + 4, ldsB4, ldsB3)
    BF16F_STEP(it0 + 5, ldsB5, ldsB4)
  }
#undef BF16F_STEP
#undef BF16F_FRAG
#undef BF16F_DMA_B

  // hand-over: the b-wave's accumulators to the a-wave of its row block through 4 KB of the dead stages 0 / 1, lane-linear 16-byte units
  unsigned char* const hnd = (rbk < 2 ? ldsB0 : ldsB1) + (rbk & 1) * 4096;
  if (br) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const f32x4 v = {acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]};
      *reinterpret_cast<f32x4*>(hnd + (i * 64 + lane) * 16) = v;
    }
  }
  bf16_sync();
  if (br) return;
  f32x16 accb;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(hnd + (i * 64 + lane) * 16);
    accb[4 * i] = v.x; accb[4 * i + 1] = v.y; accb[4 * i + 2] = v.z; accb[4 * i + 3] = v.w;
  }
  // (the a-wave's own region again below: a wave's LDS accesses are served in order; the fence keeps the compiler from reordering)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // epilogue: conv_bf16s.hpp's, one 32-channel group per lane; interior of the padded NHWC output
  const unsigned c = (unsigned)(n64 * 32 + (lane & 31));
  unsigned char* const stg = hnd;                  // OUT_BF16: this wave's [32 rows][32 channels] of 16 bits
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
    for (int rr = 0; rr < 8; rr++) s[rr] = bf16_dual_ep(acc[rh * 8 + rr], accb[rh * 8 + rr], e[rr]);
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
#undef BF16F_VMCNT
#undef BF16F_FN
