// AGZ_COMPUTE_BF16 in the trainer (DESIGN.md section 2 `bf16-train`, section 9): the three GEMMs of a dual-block layer with ONE bf16 product
// per multiply — v_mfma_f32_32x32x16_bf16 on operands rounded once to nearest even, fp32 accumulation, raw fp32 results.  Included by
// train.hip at file scope after its DMA helpers (wg_dma16, wg_rsrc_t, wg_bf16x8_t, wg_s4_t, TGeo, pix_off) and conv_maps.hpp.
//
//   k_round_bf16_planes    fp32 padded NHWC -> bf16, same layout (the halo's zeros stay zeros); eight elements and one 16-byte store per lane
//   k_round_bf16_weights   fp32 master filter [tap][out][in] -> the convolution's DMA image [in / 32][tap][out][32] bf16, either as it is
//                          (forward) or transposed with flipped taps (data gradient): one kernel, one flag
//   k_conv_bf16t           3x3 convolution as an implicit GEMM, forward and data gradient
//   k_wgrad_bf16t          weight gradient, three taps of a kernel row per workgroup
//
// What one plane per operand changes against the fp16x2 kernels (k_conv_h2dma3, k_wgrad_h2t3), which land a hi and a lo plane of both
// operands and spend three MFMAs per fragment pair: the same LDS holds twice the pixels or twice the stages.  The convolution keeps the
// 256 x 128 tile and spends the halved image on 464 instead of 372 rows (boards down to 7 x 6 fit a tile's haloed span), the halved
// weight stage on a ring of FOUR taps three taps ahead, and the rest on a second K group of four waves with operands and accumulators of
// its own, which halves every fp32 summation chain (one eight-wave workgroup per CU); the weight gradient spends it on a 64-pixel
// x image, which takes any board from three columns up (k_wgrad_h2t3: 40 pixels, boards >= 16 wide).
#pragma once

typedef __attribute__((address_space(3))) void* bt_lds_ptr_t;

// ---- rounding passes ----------------------------------------------------------------------------------------------------------------
// two fp32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32), a in the low half; NaN stays NaN, values past the bf16 range
// become Inf as the conversion defines (as in `bf16-tower`)
__device__ __forceinline__ unsigned bt_pack2(float a, float b) {
  typedef float bt_f2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bt_b2 __attribute__((ext_vector_type(2)));
  bt_f2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bt_b2));
}
__global__ __launch_bounds__(256) void k_round_bf16_planes(const float* __restrict__ x, unsigned short* __restrict__ y, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const float4 a = reinterpret_cast<const float4*>(x)[2 * i], b = reinterpret_cast<const float4*>(x)[2 * i + 1];
    uint4 o;
    o.x = bt_pack2(a.x, a.y); o.y = bt_pack2(a.z, a.w); o.z = bt_pack2(b.x, b.y); o.w = bt_pack2(b.z, b.w);
    reinterpret_cast<uint4*>(y)[i] = o;
  }
}
// img[cc][tap][o][k] = r(src), one lane per 8 k (16-byte store).  TR = false: out = N rows, in = Cin, src = wf[tap][o][32 cc + k];
// TR = true (data gradient: the convolution of dz [.., N] into [.., Cin]): out = Cin rows, in = N, src = wf[8 - tap][32 cc + k][o]
template <bool TR>
__global__ __launch_bounds__(256) void k_round_bf16_weights(const float* __restrict__ wf, unsigned short* __restrict__ img, int N, int Cin) {
  const int n_out = TR ? Cin : N, n_in = TR ? N : Cin;
  const size_t total = (size_t)9 * n_out * (n_in >> 3);
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k8 = (int)(idx & 3);
  size_t t = idx >> 2;
  const int o = (int)(t % n_out); t /= n_out;
  const int tap = (int)(t % 9), cc = (int)(t / 9);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int i = cc * 32 + k8 * 8 + k;
    v[k] = TR ? wf[((size_t)(8 - tap) * N + i) * Cin + o] : wf[((size_t)tap * N + o) * Cin + i];
  }
  uint4 q;
  q.x = bt_pack2(v[0], v[1]); q.y = bt_pack2(v[2], v[3]); q.z = bt_pack2(v[4], v[5]); q.w = bt_pack2(v[6], v[7]);
  reinterpret_cast<uint4*>(img)[idx] = q;
}

// ---- the convolution ----------------------------------------------------------------------------------------------------------------
// A workgroup of EIGHT waves computes 256 output pixels x 128 output channels, split over K: waves 0-3 (group 0) take the even 32-channel
// chunks, waves 4-7 (group 1) the odd ones, each group with the 2 x 2 wave layout and a full set of accumulators, and the two partial
// results meet through LDS at the end (group 0 + group 1, a fixed order).  Every fp32 accumulator so sums HALF the 9 Cin terms: a single
// chain over 9 * 2K terms (the data gradient) measured 4.4 times the float32 torch ruler on the local metric at K = 128, past the
// arithmetic's own bar; the error of a sequential fp32 sum grows with the root of its length.  Per 64-channel step ONE image per group of
// the tile's input lands by DMA: the padded
// pixels from (first output pixel) - Wp - 1 to (last output pixel) + Wp + 1 (conv_maps.hpp: cd3_base / cd3_row0 / cd3_tap / cd3_rows, the
// maps k_conv_h2dma3 uses and tests/cpp/conv_maps_check.cpp checks), 64-byte rows, swizzled on the source unit; tap (ky, kx) of output
// pixel m reads image row ra(m) + ky Wp + kx.  The weights of a tap (per group 128 rows x 64 bytes) stream through a ring of
// four taps, issued three taps ahead right after the barrier that frees their slot; each wave lands two instructions of a tap, so
// "tap t has landed" is s_waitcnt vmcnt(4) with two younger taps in flight (2 / 0 at the last two; 0 at a step's first tap,
// which also waits for the image, issued after every wave left the step before).  One MFMA per 32 x 32 x 16 product, chunks ascending,
// taps ascending.  122 KB of LDS while it runs, 128 KB for the exchange: one workgroup per CU, two waves per SIMD as two four-wave
// workgroups would be, one barrier per tap for twice the products.  Rows >= M repeat row M - 1 and weight rows >= Ntot of a last,
// partial column tile are the next tap's rows (or, past
// the image's last byte, the zeros a buffer load returns there): masked at the store, nothing at the load; the buffer resources end at the
// plane's and the image's last byte, so no DMA leaves the allocations, and image rows past the plane land zeros and are never read.
constexpr int BT_IMG = 464;                 // rows of the x image: 29 DMA instructions; 19 x 19 needs 370, 7 x 6 needs 458
constexpr int BT_IMG_INSTR = BT_IMG / 16;
constexpr int BT_RING = 4;
struct ConvBf16tArgs {
  const unsigned short* x;   // [B][Hp][Wp][Cin] bf16 (zero halo)
  const unsigned short* w;   // [Cin / 32][tap][Ntot][32] bf16
  float* y;                  // [B][Hp][Wp][Ntot] raw result (halo untouched)
  TGeo g;
  int Cin, Ntot, n_mtiles, n_ntiles;
};
__global__ __launch_bounds__(512, 1) void k_conv_bf16t(ConvBf16tArgs a) {
  constexpr int PA = BT_IMG * 64;           // 29 696 bytes
  constexpr int SB = 128 * 64;              // a group's weights of one tap
  constexpr int OPS = 2 * PA + BT_RING * 2 * SB;   // two images, four taps of two groups: 124 928 bytes
  constexpr int XCH = 256 * 128 * 4;        // the exchange of group 1's partial tile: 131 072 bytes
  __shared__ __attribute__((aligned(1024))) unsigned char lds[XCH > OPS ? XCH : OPS];

  const int nblk = a.n_mtiles * a.n_ntiles;
  const int id = blockIdx.x;
  int q = nblk >> 3, rr = nblk & 7, xcd = id & 7, slot = id >> 3;
  int tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + slot;
  const int m_tile = tile / a.n_ntiles, n_tile = tile - m_tile * a.n_ntiles;   // (the n-tiles of an m-tile are neighbours on one XCD)
  const int m0 = m_tile * 256, n0 = n_tile * 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = __builtin_amdgcn_readfirstlane(tid >> 8);           // K group: 32-channel chunks 2 cc + grp
  const int wid = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);     // wave of the group
  const int wm = wid >> 1, wn = wid & 1;

  auto mk = [](const void* p, size_t bytes) -> wg_rsrc_t {
    const unsigned long long u = (unsigned long long)p;
    wg_rsrc_t r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)u); r[1] = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane((unsigned)bytes); r[3] = 0x00020000u;
    return r;
  };
  const int NC = a.Cin >> 6, NS = NC * 9;                             // 64-channel steps; taps in all
  const wg_rsrc_t rx = mk(a.x, (size_t)a.g.B * a.g.Hp * a.g.Wp * a.Cin * 2);
  const wg_rsrc_t rw = mk(a.w, (size_t)2 * NS * a.Ntot * 64);
  const unsigned lds0 = (unsigned)(size_t)(bt_lds_ptr_t)lds;

  const unsigned src_unit = cmaps::dma_src_unit(lane);
  const size_t pix0 = pix_off(a.g, m0);
  const int pb = cmaps::cd3_base(pix0, a.g.Wp);                             // padded pixel of image row 0 (>= 0)
  const unsigned va0 = (unsigned)(pb + cmaps::dma_row(lane, 0)) * (unsigned)(a.Cin * 2) + src_unit;
  const unsigned vb0 = (unsigned)(n0 + 32 * wid + cmaps::dma_row(lane, 0)) * 64u + src_unit;
  const unsigned stage_bytes = (unsigned)a.Ntot * 64u;
  auto issue_A = [&](int cc) {                       // instructions j = wid, wid + 4, .. < 29
#pragma unroll
    for (int jj = 0; jj < (BT_IMG_INSTR + 3) / 4; jj++) {
      const int j = wid + 4 * jj;
      if (j < BT_IMG_INSTR) wg_dma16(rx, lds0 + (unsigned)grp * PA + cmaps::dma_dst(0, j), va0 + (unsigned)j * (unsigned)(16 * a.Cin * 2) + (unsigned)(2 * cc + grp) * 64u);
    }
  };
  auto issue_B = [&](int ts) {                       // tap ts = 9 cc + tap of this group's chunk 2 cc + grp; the weight image is [chunk][tap]
    const int cc = ts / 9;
    const unsigned so = (unsigned)(ts + 9 * (cc + grp)) * stage_bytes;   // ((2 cc + grp) * 9 + tap) stages in
    const unsigned d = lds0 + 2u * PA + (unsigned)((ts & (BT_RING - 1)) * 2 + grp) * SB + (unsigned)wid * 2048u;
#pragma unroll
    for (int j = 0; j < 2; j++) wg_dma16(rw, d + cmaps::dma_dst(0, j), vb0 + so + (unsigned)j * 1024u);
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
  unsigned ob[2][2];                                   // weight fragment offsets inside a stage
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) ob[j][ks] = cmaps::lds_off(wn * 64 + j * 32 + (lane & 31), 2 * ks + kh);

#pragma unroll
  for (int t0 = 0; t0 < BT_RING - 1; t0++)
    if (t0 < NS) issue_B(t0);
  int t = 0;
#pragma nounroll
  for (int cc = 0; cc < NC; cc++) {
    if (cc > 0) __builtin_amdgcn_s_barrier();          // every wave is done with the image of chunk cc - 1
    issue_A(cc);
#pragma nounroll
    for (int tap = 0; tap < 9; tap++) {
      // this wave's part of stage t (and, at tap 0, of the image) has landed: two instructions per younger stage may still fly
      const int ahead = NS - 1 - t;
      if (tap == 0 || ahead == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();                      // ... every wave's; and every wave is done with K step t - 1, whose slot is free
      __builtin_amdgcn_sched_barrier(0);
      if (t + BT_RING - 1 < NS) issue_B(t + BT_RING - 1);
      const unsigned char* bs = lds + 2 * PA + ((t & (BT_RING - 1)) * 2 + grp) * SB;
      const int ky = (tap * 11) >> 5;                    // tap / 3 for tap < 9
      const int toff = cmaps::cd3_tap(ky, tap - 3 * ky, a.g.Wp);
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
        wg_bf16x8_t B_[2];
#pragma unroll
        for (int j = 0; j < 2; j++) B_[j] = *reinterpret_cast<const wg_bf16x8_t*>(bs + ob[j][ks]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const wg_bf16x8_t A_ = *reinterpret_cast<const wg_bf16x8_t*>(lds + grp * PA + cmaps::lds_off(ra[i] + toff, 2 * ks + kh));
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_, B_[j], acc[i][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      t++;
    }
  }
  // group 1's partial tile through LDS (word ((i, j, r) * 256 + thread of the group): conflict-free), group 0 adds and stores
  __builtin_amdgcn_s_barrier();                          // every wave is done with the images and the ring
  float* xch = reinterpret_cast<float*>(lds) + (tid & 255);
  if (grp) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) xch[((i * 2 + j) * 16 + r) * 256] = acc[i][j][r];
  }
  __syncthreads();
  if (grp) return;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + (wm * 4 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m >= a.g.M) continue;
      float* yr = a.y + pix_off(a.g, m) * (size_t)a.Ntot + n0 + wn * 64 + (lane & 31);
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (n0 + wn * 64 + j * 32 < a.Ntot) yr[j * 32] = acc[i][j][r] + xch[((i * 2 + j) * 16 + r) * 256];   // (Ntot % 32 == 0: a 32-column group is whole or absent)
    }
}
// rows of the largest image a 256-row tile of this geometry needs (the launcher's limit: <= BT_IMG)
static inline int conv_bf16t_span(const TGeo& g) {
  int mx = 0;
  for (int m0 = 0; m0 < g.M; m0 += 256)
    mx = std::max(mx, cmaps::cd3_rows(cmaps::pix(m0, g.HW, g.W, g.Hp, g.Wp), cmaps::pix(std::min(m0 + 255, g.M - 1), g.HW, g.W, g.Hp, g.Wp), g.Wp));
  return mx;
}
static inline bool conv_bf16t_fits(const TGeo& g, int cin, int ntot) {
  return cin % 64 == 0 && ntot % 32 == 0 && ntot >= 64 && conv_bf16t_span(g) <= BT_IMG &&
         (size_t)g.B * g.Hp * g.Wp * (size_t)std::max(cin, ntot) * 4 < ((size_t)1 << 31) && (size_t)9 * cin * ntot * 2 < ((size_t)1 << 31);
}
static inline void conv_bf16t_launch(hipStream_t s, const unsigned short* x, const unsigned short* w, float* y, const TGeo& g, int cin, int ntot) {
  ConvBf16tArgs ca{};
  ca.x = x; ca.w = w; ca.y = y; ca.g = g; ca.Cin = cin; ca.Ntot = ntot;
  ca.n_mtiles = (g.M + 255) / 256; ca.n_ntiles = (ntot + 127) / 128;
  hipLaunchKernelGGL(k_conv_bf16t, dim3(ca.n_mtiles * ca.n_ntiles), dim3(512), 0, s, ca);
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------
// dw[tap][n][c] = sum over rows m of dz[m][n] * x[pix(m) + tap][c]: k_wgrad_h2t3's scheme on one plane per operand.  A workgroup owns a
// 128 x 128 tile of (n, c), one kernel ROW ky and a chunk of whole boards; a K step is 32 GEMM rows of one board.  The rows of dz
// (32 x 128 bf16) and ONE x image indexed by padded pixel (64 pixels x 128 channels: the step's rows, their row ends and the +-1 shifts)
// arrive by DMA, sixteen bytes per lane, each lane computing its own row's pixel, into [row / 4][channel / 8][row % 4][16 B]; the
// transposing LDS read (ds_read_b64_tr_b16) hands every lane its k-major fragment; the image serves the three taps kx = 0, 1, 2 of the row:
// image row of (k, kx) = delta(k) + kx, delta(k) = k + 2 * (row ends between the step's first row and row k) — any W >= 3 fits the 64
// pixels (31 + 2 * 11 + 2 + 1 at W = 3).  Two stages of 24 KB; step s + 1 lands in six pieces between the six MFMA groups of step s.
// Partial sums of the board chunks meet in dw by fp32 atomicAdd, at k_wgrad's flat offsets.
constexpr int BT_XP = 64;
struct WgBf16tArgs {
  const unsigned short *dz, *x;   // bf16 planes [pix][N], [pix][Cin]
  float* dw;
  TGeo g; int N, Cin, steps_per_board, n_tiles, c_tiles, n_chunks;
};
static inline bool wgrad_bf16t_fits(const TGeo& g, int n, int cin) {
  return g.W >= 3 && n % 8 == 0 && cin % 8 == 0 && (size_t)g.B * g.Hp * g.Wp * (size_t)std::max(n, cin) * 2 < ((size_t)1 << 31);
}
__global__ __launch_bounds__(256, 2) void k_wgrad_bf16t(WgBf16tArgs a) {
  constexpr int PA = 32 * 128 * 2, PB = BT_XP * 128 * 2, STAGE = PA + PB;
  __shared__ __attribute__((aligned(1024))) unsigned char lds0[STAGE];
  __shared__ __attribute__((aligned(1024))) unsigned char lds1[STAGE];
  const int per_chunk = a.n_tiles * a.c_tiles * 3;   // XCD-aware order: a chunk's workgroups share an XCD
  const int local = (int)(blockIdx.x >> 3);
  const int chunk = (local / per_chunk) * 8 + (int)(blockIdx.x & 7);
  if (chunk >= a.n_chunks) return;
  int bid = local % per_chunk;
  const int ct = bid % a.c_tiles; bid /= a.c_tiles;
  const int nt = bid % a.n_tiles; bid /= a.n_tiles;
  const int ky = bid;
  const int n0 = nt * 128, c0 = ct * 128;
  const int b_begin = (int)((long)chunk * a.g.B / a.n_chunks), b_end = (int)((long)(chunk + 1) * a.g.B / a.n_chunks);
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
  const wg_rsrc_t rdz = mk(a.dz, n_pix * a.N * 2), rxx = mk(a.x, n_pix * a.Cin * 2);
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
  auto delta = [&](int k, int w0) -> int {         // padded-pixel distance of the step's row k from its first row
    return k + 2 * ((w0 + k) / a.g.W);
  };
  // the landing of step s in six pieces per wave (two of dz: wave w lands rows 8 w .. 8 w + 7; four of x: sixteen four-pixel groups)
  auto issue_piece = [&](unsigned char* stage, const Step& st, int piece) {
    const unsigned base = (unsigned)(size_t)(bt_lds_ptr_t)stage;
    if (piece < 2) {
      const int k = 8 * wid + 4 * piece + kk;
      const int po = st.po0 + delta(k, st.w0);
      const unsigned oa = (na && k < st.nv) ? (unsigned)(po * a.N + n0 + 8 * cs) * 2u : OOB;
      wg_dma16(rdz, base + (unsigned)(2 * wid + piece) * 1024u, oa);
    } else {
      const int qb = st.po0 + (ky - 1) * a.g.Wp - 1;   // x: image row rho <-> padded pixel qb + rho (halo pixels hold zeros)
      const int m = wid + 4 * (piece - 2);
      const int q = qb + 4 * m + kk;
      const unsigned ob = (cb && st.nv > 0 && q >= 0) ? (unsigned)(q * a.Cin + c0 + 8 * cs) * 2u : OOB;
      wg_dma16(rxx, base + PA + (unsigned)m * 1024u, ob);
    }
  };
  const int i16 = lane & 15, kh = lane >> 5;
  const unsigned cpart = (unsigned)(((((lane >> 4) & 1) * 2 + ((i16 & 3) >> 1)) * 4) * 16 + (i16 & 1) * 8);   // channel part of a read address
  const unsigned foa = (unsigned)(kh * 2048 + (i16 >> 2) * 16) + cpart;                                   // dz: rows are the k themselves
  auto tr2 = [&](const unsigned char* p0, const unsigned char* p1) -> wg_bf16x8_t {
    const wg_s4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s4_t)(p0));
    const wg_s4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s4_t)(p1));
    return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto compute = [&](const unsigned char* stage, int s, unsigned char* next_stage) {
    const int w0 = step_of(s).w0;
    const Step nx = step_of(s + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      wg_bf16x8_t A_[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const unsigned char* q = stage + foa + (wm * 64 + i * 32) * 8 + ks * 4096;
        A_[i] = tr2(q, q + 1024);
      }
      const int k0 = ks * 16 + kh * 8 + (i16 >> 2);  // this lane's rows of the step: k0 and k0 + 4
      const int d0 = delta(k0, w0), d1 = delta(k0 + 4, w0);
#pragma unroll
      for (int kx = 0; kx < 3; kx++) {
        const int r0 = d0 + kx, r1 = d1 + kx;
        const unsigned o0 = (unsigned)((r0 >> 2) * 1024 + (r0 & 3) * 16) + cpart, o1 = (unsigned)((r1 >> 2) * 1024 + (r1 & 3) * 16) + cpart;
        wg_bf16x8_t B_[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const unsigned char* q = stage + PA + (wn * 64 + j * 32) * 8;
          B_[j] = tr2(q + o0, q + o1);
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[kx][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_[i], B_[j], acc[kx][i][j], 0, 0, 0);
        issue_piece(next_stage, nx, ks * 3 + kx);    // next step's landing, a piece after each MFMA group
      }
    }
  };
  // raw s_barrier + explicit vmcnt: a __syncthreads() fence knows nothing of the assembly DMA
  {
    const Step st0 = step_of(0);
#pragma unroll
    for (int piece = 0; piece < 6; piece++) issue_piece(lds0, st0, piece);
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
          if (n < a.N && c < a.Cin) atomicAdd(&a.dw[((size_t)(ky * 3 + kx) * a.N + n) * a.Cin + c], acc[kx][i][j][r]);
        }
}
// chunks of whole boards (k_wgrad_h2t3's rule: about two rounds of workgroups per XCD) and the launch; returns the chunk count.
// pad_lds: unused dynamic LDS on top of the 48 KB, so that a second workgroup does not fit a CU beside the main stream's chain
static inline int wgrad_bf16t_launch(hipStream_t s, int num_cus, const unsigned short* dz, const unsigned short* x, float* dw, const TGeo& g, int n, int cin,
                                     size_t pad_lds) {
  WgBf16tArgs w{};
  w.dz = dz; w.x = x; w.dw = dw; w.g = g; w.N = n; w.Cin = cin;
  w.n_tiles = (n + 127) / 128; w.c_tiles = (cin + 127) / 128; w.steps_per_board = (g.HW + 31) / 32;
  const int per_chunk3 = w.n_tiles * w.c_tiles * 3;
  const int slots = std::max(1, num_cus / 8 * 2);
  w.n_chunks = std::min(g.B, 8 * std::max(1, 2 * slots / per_chunk3));
  hipLaunchKernelGGL(k_wgrad_bf16t, dim3((unsigned)(per_chunk3 * ((w.n_chunks + 7) / 8 * 8))), dim3(256), pad_lds, s, w);
  return w.n_chunks;
}
