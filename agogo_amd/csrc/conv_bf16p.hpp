// The packed-boards form of conv_bf16a.hpp's block (AGZ_COMPUTE_BF16_ACT with agz_net_set_bf16_packed_boards): the same declared
// arithmetic (`bf16-tower`), the same results bit for bit, SEVERAL small boards per workgroup so that the 384 GEMM
// rows of its four waves are live rows.  DESIGN.md section 4i.
//
// Why.  conv_bf16a.hpp gives a workgroup one board: every wave issues every MFMA of every step whether its 96 rows are on the board or
// clamped, so a 9x9 block (81 rows) costs what a 19x19 block (361 rows) costs.  Here a workgroup owns boards [b0, b0 + nb),
// nb = min(G, B - b0), G = min(384 / HW, BF16P_SP_MAX / HpWp) (agz_bf16_packed_boards_of: 19 at 3x3, 6 at 7x6, 4 at 9x9, 2 at 13x13),
// and one 128-column tile [64 a | 64 b]: 1 / G of the workgroups, each with the MFMAs of one.
//
// Why the bits are the same.  K is never split: every output element is ONE accumulator that starts at zero and sums in the order
// (64-channel chunk, tap, 16-channel step) with v_mfma_f32_32x32x16_bf16 — which row of which wave's tile holds the element, and which
// boards share the tile, do not enter the arithmetic.  The operands are the same bf16 values (conv_bf16.hpp's weight image, block 0 rounds
// its fp32 input with the same v_cvt_pk_bf16_f32), the epilogue is bf16_dual_ep / bf16_pack2 on the parameters of the element's own
// in-board pixel.  No row ever reads another board's pixels: a window's nine taps stay inside its board's own haloed Hp x Wp image.
//
// Rows.  In both activation layouts ([B][Hp][Wp][Kp], fp32 and bf16) consecutive boards are one contiguous run of padded pixels: the
// workgroup stages the contiguous slice of SP = nb HpWp pixels that starts at board b0's first padded pixel, every board with its own
// halo.  GEMM row m in [0, nb HW) is board g = m / HW, in-board row r = m - g HW, line = r / W, col = r - line W; its window's top-left
// pixel in the slice is g HpWp + line Wp + col and tap (ky, kx) adds ky Wp + kx.  Rows >= nb HW clamp to the last live row for the reads
// and are never stored (7x6, G = 6: 252 rows — the third wave ragged, the fourth only clamped rows; it still takes its part of the DMA
// and the barriers).  Divisions by HW, W, HpWp, Wp are multiply-and-shift with host-made constants (bf16p_div).
//
// Bank map across board boundaries.  conv_bf16.hpp's swizzle f(p) = ((p - 2 line(p)) >> 1) & 7 needs p - 2 line to count pixels as the
// GEMM rows do; it does not where the 16 consecutive rows of a fragment read run from one board into the next (at 3x3 a 32-row fragment
// spans four boards), because the slice has HpWp - HW more pixels per board than the GEMM has rows.  Here
//   image address of (slice pixel p, 16-byte unit u)  =  128 p + 16 (u ^ f),   f = (n(p) >> 1) & 7,
//   n(p) = g HW + pl W + pc   for the pixel at padded in-board coordinates (pl, pc) of board g  ( = p - g (HpWp - HW) - 2 pl ).
//   (a) one n per pixel, whichever window reaches it: the window of row m = (g, line, col) has its tap (ky, kx) at pl = line + ky,
//       pc = col + kx, so n = m + ky W + kx — the reader computes f from its row and the tap, the writer from the pixel, and they agree;
//       the map permutes the 8 units inside a pixel's own 128 bytes, so two pixels never collide whatever f is.
//   (b) n is CONSECUTIVE in m for every tap, across line ends and across board boundaries alike.
//   (c) p - n = g (HpWp - HW) + 2 pl is even (HpWp - HW = 2 H + 2 W + 4): p and n share parity.
//   The 16 lanes a ds_read_b128 serves together hold 16 consecutive rows m and one u: by (b) 8 even and 8 odd n, by (c) 8 even and
//   8 odd p (bit 3 of the slot), and within a parity n >> 1 runs through 8 consecutive integers: 8 different f — 16 different slots,
//   for all nine taps.  (Clamped rows repeat one address: a broadcast.)  Staging writes put the 8 units of one pixel on 8 consecutive
//   lanes (DMA: lane-linear, 16 lanes = an even and an odd pixel x 8 units): 16 slots whatever f is.
//
// Staging.  conv_bf16a.hpp's DMA map with SP = nb HpWp: round r of a workgroup fills LDS units 256 r + tid = (pixel q, slot s) from
// global unit s ^ f(q); lanes with idx >= 8 SP are masked and the buffer resource ends at the slice.  A full stage of BF16P_SP_MAX = 496
// pixels is 15.5 rounds: 16 rounds, the last one partial by construction (its upper two waves are always masked), tap t of chunk c
// issues rounds t and t + 9 (t <= 6) of chunk c + 1.  Block 0 stages fp32 through registers, two units per thread and tap:
// 9 x 2 x 256 = 4608 >= 3968 units.  Completion is conv_bf16a.hpp's rule: every wave waits for its own DMA before the barrier that ends
// a step, nothing is in flight across a barrier; four separate __shared__ objects, chunk and tap loops unrolled by two.
// LDS: 2 x 496 x 128 + 2 x 16 KB = 159 744 B static, one workgroup per CU.
// Output: conv_bf16a.hpp's — bf16 through the wave's own 12 KB of the dead stage A0 (4 x 12 KB <= 62 KB) and 16-byte stores, the last
// block fp32 — each row to the interior of its own board b0 + g.
//
// Element type E (conv_bf16.hpp): Fp16El is the packed-boards form of AGZ_COMPUTE_FP16, equal bit for bit to that mode's whole-board
// kernel by the argument above with E::mfma and E::pack2 in the places of the bf16 instructions.  The element is 16 bits either way: the
// bank map across board boundaries, the staging, the completion rule and the write-back are the same bytes and the same instructions.
#pragma once
// (included by net.hip INSIDE namespace agz, after conv_bf16a.hpp: bf16a_lds_ptr_t, bf16_dual_ep, bf16_pack2 / bf16_sync, BF16_B_STAGE)

#define BF16P_FN __attribute__((target("no-packed-fp32-ops")))

constexpr int BF16P_SP_MAX = 496;                  // haloed pixels of a staged slice (four 9x9 boards: 484)
constexpr int BF16P_A_STAGE = BF16P_SP_MAX * 128;
constexpr int BF16P_ROUNDS = (BF16P_SP_MAX * 8 + 255) / 256;   // DMA rounds of a whole activation stage: 16, the last one half
static_assert(2 * (BF16P_A_STAGE + BF16_B_STAGE) <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");
static_assert(BF16P_ROUNDS <= 18, "at most two rounds per tap");
static_assert(9 * 2 * 256 >= BF16P_SP_MAX * 8, "block 0: two units per thread and tap bring a whole stage");
static_assert(4 * 96 * 128 <= BF16P_A_STAGE, "the four waves' output regions fit the dead stage");
static_assert(BF16P_SP_MAX <= 512 && BF16_ROWS <= 512, "bf16p_div: x d < 2^20");

struct Bf16pArgs {
  const float* x;             // fp32 padded NHWC [B][Hp][Wp][Kp]: the input of block 0 (!IN_BF16)
  float* y;                   //                                  the output of the last block (!OUT_BF16)
  const unsigned short* xh;   // bf16 padded NHWC [B][Hp][Wp][Kp] (IN_BF16)
  unsigned short* yh;         //                                  (OUT_BF16)
  const f32x4* ep;            // {sa, ta, sb, tb} [HW][Kp], shared by all boards
  const unsigned short* wq;   // agz_net::build_bf16_weights image
  int B, G;                   // boards of the launch, boards per workgroup (G HW <= 384, G HpWp <= BF16P_SP_MAX)
  int HW, W, Wp, HpWp, Kp;
  int n_ntiles, ncc;
  unsigned mg_hw, mg_w, mg_hpwp, mg_wp;   // bf16p_magic of HW, W, HpWp, Wp
};

// x / d = (x m) >> 20 with m = 2^20 / d + 1 (host: bf16p_magic), exact while x (m d - 2^20) < 2^20; m d - 2^20 <= d, and here
// x < 512 (a GEMM row or a staged pixel) and d <= 248 (G >= 2: HpWp <= BF16P_SP_MAX / 2)
BF16P_FN __device__ __forceinline__ unsigned bf16p_div(unsigned x, unsigned magic) { return (x * magic) >> 20; }

// staging unit `idx` of the slice (pixel idx / 8, 16-byte unit idx % 8): the swizzle f of its pixel (the bank map above)
BF16P_FN __device__ __forceinline__ unsigned bf16p_f(unsigned q, const Bf16pArgs& a) {
  const unsigned g = bf16p_div(q, a.mg_hpwp);
  const unsigned pl = bf16p_div(q - g * (unsigned)a.HpWp, a.mg_wp);
  return ((q - g * (unsigned)(a.HpWp - a.HW) - 2u * pl) >> 1) & 7u;
}

template <typename E, bool IN_BF16, bool OUT_BF16>
BF16P_FN __global__ __launch_bounds__(256, 1) void conv3x3_bf16p_dual_kernel(Bf16pArgs a) {
  typedef typename E::frag frag_t;
  // four objects, not one array: every LDS access names its stage at compile time (conv_bf16a.hpp, `completion`)
  __shared__ __attribute__((aligned(16))) unsigned char ldsA0[BF16P_A_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsA1[BF16P_A_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB0[BF16_B_STAGE];
  __shared__ __attribute__((aligned(16))) unsigned char ldsB1[BF16_B_STAGE];

  // XCD-aware order, tile -> (board group, n-tile): conv3x3_bf16_dual_kernel's
  const int nblk = gridDim.x, id = blockIdx.x;
  const int xq = nblk >> 3, xr = nblk & 7, xcd = id & 7, slot = id >> 3;
  const int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + slot;
  const int n_tile = tile % a.n_ntiles, grp = tile / a.n_ntiles;
  const int b0 = grp * a.G;
  const int nb = a.B - b0 < a.G ? a.B - b0 : a.G;          // boards [b0, b0 + nb), nb >= 1 (the launcher's grid)
  const int mend = nb * a.HW;                              // live GEMM rows [0, mend)
  const int SP = nb * a.HpWp;                              // pixels staged (<= BF16P_SP_MAX by the definition of G)

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nit = a.ncc * 9;
  const unsigned dma_w = (unsigned)wid * 1024u;            // the wave's 1 KB of a 4 KB DMA round (the hardware adds 16 lane)

  // weights: the n-tile's [chunk][tap][16 KB] run of wq; lane offset 16 tid, (step, round) in the scalar offset
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.wq) + (size_t)n_tile * nit * (BF16_B_STAGE / 2), 0, nit * BF16_B_STAGE, 0x00020000);
  const unsigned wvo = (unsigned)tid * 16u;
#define BF16P_DMA_B(IT, DST)                                                                                              \
  _Pragma("unroll") for (int j_ = 0; j_ < 4; j_++)                                                                        \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (bf16a_lds_ptr_t)((DST) + j_ * 4096 + dma_w), 16, wvo,                   \
                                             (unsigned)(IT) * (unsigned)BF16_B_STAGE + j_ * 4096u, 0, 0);

  // bf16 activations: the slice's pixels [0, SP) from board b0's first padded pixel; round r brings LDS units 256 r + tid
  const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.xh) + (IN_BF16 ? (size_t)b0 * a.HpWp * a.Kp : 0), 0, IN_BF16 ? SP * a.Kp * 2 : 0, 0x00020000);
#define BF16P_DMA_A(R, CC, DST)                                                                                           \
  {                                                                                                                       \
    const int idx_ = (R) * 256 + tid;                                                                                     \
    if (idx_ < SP * 8) {                                                                                                  \
      const unsigned q_ = (unsigned)idx_ >> 3, s_ = (unsigned)idx_ & 7u;                                                  \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr_, (bf16a_lds_ptr_t)((DST) + (R) * 4096 + dma_w), 16,                    \
                                               q_ * (unsigned)a.Kp * 2u + ((s_ ^ bf16p_f(q_, a)) << 4), (unsigned)(CC) * 128u, 0, 0); \
    }                                                                                                                     \
  }

  // fp32 activations (block 0): conv_bf16.hpp's staging — two 32-byte units per thread and tap through registers — on this file's map
  const char* xb = reinterpret_cast<const char*>(a.x + (IN_BF16 ? 0 : (size_t)b0 * a.HpWp * a.Kp));
  f32x4 ra[2][2];
  bool av[2];
  unsigned al[2];
#define BF16P_UNIT(IDX, GOFF, LOFF)                                                              \
  {                                                                                              \
    const unsigned q_ = (unsigned)(IDX) >> 3, u_ = (unsigned)(IDX) & 7u;                         \
    GOFF = (q_ * (unsigned)a.Kp + u_ * 8u) * 4u;                                                 \
    LOFF = q_ * 128u + ((u_ ^ bf16p_f(q_, a)) << 4);                                             \
  }
#define BF16P_LOAD_A(T, CC)                                                                      \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; s_++) {                                             \
    const int idx_ = tid + 256 * (2 * (T) + s_);                                                 \
    unsigned ag_;                                                                                \
    av[s_] = idx_ < SP * 8;                                                                      \
    BF16P_UNIT(av[s_] ? idx_ : 0, ag_, al[s_])                                                   \
    if (av[s_]) {                                                                                \
      const char* g_ = xb + ag_ + (unsigned)(CC) * 256u;                                         \
      ra[s_][0] = *reinterpret_cast<const f32x4*>(g_);                                          \
      ra[s_][1] = *reinterpret_cast<const f32x4*>(g_ + 16);                                     \
    }                                                                                            \
  }
#define BF16P_STORE_A(DST)                                                                       \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; s_++)                                               \
    if (av[s_]) {                                                                                \
      u32x4_t v_ = {E::pack2(ra[s_][0].x, ra[s_][0].y), E::pack2(ra[s_][0].z, ra[s_][0].w),      \
                    E::pack2(ra[s_][1].x, ra[s_][1].y), E::pack2(ra[s_][1].z, ra[s_][1].w)};     \
      *reinterpret_cast<u32x4_t*>((DST) + al[s_]) = v_;                                          \
    }
// this wave's DMA has landed (vmcnt = 0; expcnt and lgkmcnt left alone), then every wave's: the barrier
#define BF16P_STEP_END()                \
  __builtin_amdgcn_s_waitcnt(0x0f70);   \
  bf16_sync();

  // fragment rows of this lane: row block 3 wid + i, row lane & 31 -> top-left pixel of its 3x3 window inside the slice
  int prel[3], mrow[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int m = (3 * wid + i) * 32 + (lane & 31);
    if (m >= mend) m = mend - 1;
    const unsigned g = bf16p_div((unsigned)m, a.mg_hw), r = (unsigned)m - g * (unsigned)a.HW;
    const unsigned line = bf16p_div(r, a.mg_w), col = r - line * (unsigned)a.W;
    prel[i] = (int)(g * (unsigned)a.HpWp + line * (unsigned)a.Wp + col);
    mrow[i] = m;                                           // n of the window's top-left pixel (the bank map above)
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
  BF16P_DMA_B(0, ldsB0)
  if (IN_BF16) {
#pragma unroll
    for (int r = 0; r < BF16P_ROUNDS; r++) BF16P_DMA_A(r, 0, ldsA0)
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
        BF16P_UNIT(pv[t] ? idx : 0, pg, pl[t])
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
  BF16P_STEP_END()

  // One (chunk, tap) step: conv_bf16a.hpp's.  SB, the weight stage of the step, and the activation stage of the chunk are compile-time
  // constants where the macro is used.  The tap moves a row's pixel by ky Wp + kx and its n by ky W + kx.
#define BF16P_FRAGS(S, KS)                                                                                                \
  {                                                                                                                       \
    const unsigned u_ = (unsigned)(2 * (KS) + half);                                                                      \
    _Pragma("unroll") for (int i = 0; i < 3; i++)                                                                         \
      A_[S][i] = *reinterpret_cast<const frag_t*>(Ac + aoff[i] + ((u_ ^ asw[i]) << 4));                                   \
    _Pragma("unroll") for (int jb = 0; jb < 4; jb++)                                                                      \
      B_[S][jb] = *reinterpret_cast<const frag_t*>(Bc + jb * 4096 + brow + ((u_ ^ bsw) << 4));                            \
  }
#define BF16P_STEP(TAP, SB)                                                                                               \
  {                                                                                                                       \
    const int tap = (TAP), it = cc * 9 + tap;                                                                             \
    const unsigned char* const Bc = (SB) ? ldsB1 : ldsB0;                                                                 \
    unsigned char* const Bn = (SB) ? ldsB0 : ldsB1;                                                                       \
    /* the next step's operands leave for the other stages before this step's MFMAs (those stages were last read a */     \
    /* whole step / chunk ago, before the barrier that ended it) */                                                       \
    if (it + 1 < nit) { BF16P_DMA_B(it + 1, Bn) }                                                                         \
    if (more_a) {                                                                                                         \
      if (IN_BF16) {                                                                                                      \
        BF16P_DMA_A(tap, cc + 1, An)                                                                                      \
        if (tap + 9 < BF16P_ROUNDS) BF16P_DMA_A(tap + 9, cc + 1, An)                                                      \
      } else {                                                                                                            \
        BF16P_LOAD_A(tap, cc + 1)                                                                                         \
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
    BF16P_FRAGS(0, 0)                                                                                                     \
    _Pragma("unroll") for (int ks = 0; ks < 4; ks++) {                                                                    \
      if (ks < 3) BF16P_FRAGS((ks + 1) & 1, ks + 1)                                                                       \
      _Pragma("unroll") for (int i = 0; i < 3; i++)                                                                       \
        _Pragma("unroll") for (int j = 0; j < 2; j++)                                                                     \
          _Pragma("unroll") for (int br = 0; br < 2; br++)                                                                \
            acc[i][j][br] = E::mfma(A_[ks & 1][i], B_[ks & 1][br * 2 + j], acc[i][j][br]);                                \
    }                                                                                                                     \
    if (!IN_BF16 && more_a) { BF16P_STORE_A(An) }                                                                         \
    BF16P_STEP_END()                                                                                                      \
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
          BF16P_STEP(t2, sa)
          BF16P_STEP(t2 + 1, sa ^ 1)
        }
        BF16P_STEP(8, sa)
      }
    }
  }
#undef BF16P_STEP
#undef BF16P_FRAGS
#undef BF16P_DMA_A
#undef BF16P_DMA_B
#undef BF16P_LOAD_A
#undef BF16P_STORE_A
#undef BF16P_UNIT
#undef BF16P_STEP_END

  // epilogue: BN(scale, shift) + ReLU per branch, add, ReLU on the parameters of the row's in-board pixel; interior of the padded NHWC
  // output of the row's own board (offsets from board b0: at most BF16P_SP_MAX pixels)
  unsigned char* const stg = ldsA0 + wid * (96 * 128);   // OUT_BF16: this wave's [96 rows][64 channels] bf16 (both A stages are dead)
  float* yb = a.y + (OUT_BF16 ? 0 : (size_t)b0 * a.HpWp * a.Kp);
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int rh = 0; rh < 2; rh++) {
      // the parameters of eight rows leave together (rows past the end load the last row's), as in conv_bf16.hpp
      f32x4 e[8][2];
#pragma unroll
      for (int rr = 0; rr < 8; rr++) {
        const int r = rh * 8 + rr;
        const int m = (3 * wid + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const unsigned mc = (unsigned)(m < mend ? m : mend - 1);
        const unsigned rb = mc - bf16p_div(mc, a.mg_hw) * (unsigned)a.HW;      // in-board row
#pragma unroll
        for (int j = 0; j < 2; j++) e[rr][j] = a.ep[rb * (unsigned)a.Kp + (unsigned)(n_tile * 64 + j * 32 + (lane & 31))];
      }
#pragma unroll
      for (int rr = 0; rr < 8; rr++) {
        const int r = rh * 8 + rr;
        const int lr = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;      // row inside the wave's 96
        const int m = wid * 96 + lr;
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
          const unsigned g = bf16p_div((unsigned)m, a.mg_hw), rb = (unsigned)m - g * (unsigned)a.HW;
          const unsigned h = bf16p_div(rb, a.mg_w), w = rb - h * (unsigned)a.W;
          const unsigned obase = (g * (unsigned)a.HpWp + (h + 1u) * (unsigned)a.Wp + (w + 1u)) * (unsigned)a.Kp;
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
    unsigned char* yhb = reinterpret_cast<unsigned char*>(a.yh) + (size_t)b0 * a.HpWp * a.Kp * 2 + (size_t)n_tile * 128;
#pragma unroll
    for (int t = 0; t < 12; t++) {
      const int lr = t * 8 + (lane >> 3), sl = lane & 7;
      const int m = wid * 96 + lr;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(stg + lr * 128 + sl * 16);
      if (m < mend) {
        const unsigned g = bf16p_div((unsigned)m, a.mg_hw), rb = (unsigned)m - g * (unsigned)a.HW;
        const unsigned h = bf16p_div(rb, a.mg_w), w = rb - h * (unsigned)a.W;
        const unsigned u = (unsigned)sl ^ ((unsigned)((lr >> 2) & 1) << 2);
        *reinterpret_cast<u32x4_t*>(yhb + (g * (unsigned)a.HpWp + (h + 1u) * (unsigned)a.Wp + (w + 1u)) * (unsigned)a.Kp * 2u + u * 16u) = v;
      }
    }
  }
}
#undef BF16P_FN
