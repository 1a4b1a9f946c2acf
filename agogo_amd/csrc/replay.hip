// agz_replay: a sliding window over the most recent `capacity` examples, device resident, and its sampler (BUILD EXTENSION, DESIGN.md §2
// replay-window).  The standard AlphaZero arrangement around dual.Train: a ring of recent positions, minibatches drawn uniformly from it
// with replacement, each row under a random board symmetry applied AS IT IS DRAWN — no materialised copies (agz_examples_augment_dihedral
// holds eight), no index array and no host synchronisation per minibatch.  The draw and the ring arithmetic are replay.hpp's, the eight maps
// sym.hpp's.  Rows are agz_examples rows: planes [F*H*W], policy [PolicyLen], value, fp32 — or, in a window made by
// agz_replay_create_packed, the planes as 2-bit codes under a palette (replay_pack.hpp), decoded by the sampler as it draws.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "replay_win.hpp"   // (hip_runtime.h first: replay.hpp's device half uses __umul64hi)
#include "replay.hpp"
#include "replay_pack.hpp"
#include "replay_ckpt.hpp"
#include "atomic_file.hpp"
#include "ckpt_stream.hpp"
#include "sym.hpp"

namespace agz {

constexpr int REPLAY_THREADS = 256;
constexpr int REPLAY_SEG = REPLAY_THREADS * 8;   // elements of one output row that one workgroup moves
constexpr int REPLAY_TAB = 1024;                 // cells of the largest board sampled under a symmetry (32 x 32); 4 KB of LDS

// Rows [row0, row0 + cnt) of one minibatch of `rows` rows (the whole of it: row0 = 0, cnt = rows): out row r = S_k(window row j), (j, k) =
// replay::draw(seed, step, rows, row0 + r, n, symmetric) — computed here, the same in every lane of the workgroup.  An output row is the
// concatenation [planes F*mm | policy A1 | value 1] cut into segments of REPLAY_SEG elements: grid = (segments, cnt).  The mm source cells of S_k go to LDS once per workgroup; a plane element then costs one LDS read, one gathered
// global read (within a 4*mm-byte board: the same cache lines whatever k is) and one coalesced write.  k == 0 copies straight through.
// Pure data movement: algorithmic bytes = 2 x payload of `rows` rows.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_sample(const float* __restrict__ planes, const float* __restrict__ policy,
                                                                  const float* __restrict__ value, float* __restrict__ X,
                                                                  float* __restrict__ Pi, float* __restrict__ V, int F, int m, int mm,
                                                                  int A1, int rows, int row0, int cnt, uint64_t seed, uint64_t step,
                                                                  int symmetric, uint64_t n, uint64_t total, uint64_t cap) {
  __shared__ int tab[REPLAY_TAB];
  const int xs = F * mm, row = xs + A1 + 1;
  const int e0 = (int)blockIdx.x * REPLAY_SEG;
  const int e1 = min(e0 + REPLAY_SEG, row);
  for (int r = (int)blockIdx.y; r < cnt; r += (int)gridDim.y) {
    const replay::Draw d = replay::draw(seed, step, rows, row0 + r, n, symmetric != 0);
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

// ---- packed windows (agz_replay_create_packed, DESIGN.md §2 replay-packed; the layout is replay_pack.hpp's) -----------------------------

constexpr uint64_t PACK_NONE = ~0ull;   // "no bad cell" in chk[1]
constexpr size_t PACK_STAGING_BYTES = (size_t)8 << 20;   // host rows go up to the device through at most this much staging (at least one row)

// Validation of an append: chk[0] += the elements of src[0, n) whose bit pattern is not in the palette, chk[1] = min(chk[1], the first
// such element).  A lane touches chk only if it met a bad element, so a clean append costs no atomic at all.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_pack_check(const uint32_t* __restrict__ src, uint64_t n, uint32_t p0, uint32_t p1,
                                                                      uint32_t p2, uint32_t p3, int n_pal,
                                                                      unsigned long long* __restrict__ chk) {
  unsigned long long bad = 0, first = PACK_NONE;
  const uint64_t stride = (uint64_t)gridDim.x * REPLAY_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * REPLAY_THREADS + threadIdx.x; i < n; i += stride) {
    if (replay_pack::code_of(p0, p1, p2, p3, n_pal, src[i]) < 0) {
      bad++;
      if (i < first) first = i;
    }
  }
  if (bad) {
    atomicAdd(&chk[0], bad);
    atomicMin(&chk[1], first);
  }
}

// Source rows [0, rows) of `src` ([rows][F * mm] bit patterns, every one in the palette) into the ring slots (slot0 + r) mod cap: at most
// two contiguous slot ranges.  A row is walked in its PADDED index t = (f * wpp + w) * 16 + i, cell c = w * 16 + i of plane f: lanes read
// consecutive cells of a plane (coalesced), the 16 lanes of a word OR their shifted codes together by four xor-shuffles and lane i == 0
// writes the word whole — no atomics on the store, the same words whatever the launch geometry.  Cells past mm contribute zero bits.
// Every lane of a wavefront runs every iteration (the loop bound is the workgroup's), as the shuffles need.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_pack(const uint32_t* __restrict__ src, uint32_t* __restrict__ packed, int F,
                                                                int mm, int wpp, int rows, uint64_t slot0, uint64_t cap, uint32_t p0,
                                                                uint32_t p1, uint32_t p2, uint32_t p3, int n_pal) {
  const int row_words = F * wpp;
  const int64_t padded = (int64_t)row_words * replay_pack::CODES_PER_WORD;
  const size_t xs = (size_t)F * mm;
  for (int r = (int)blockIdx.y; r < rows; r += (int)gridDim.y) {
    const uint32_t* in = src + (size_t)r * xs;
    uint32_t* out = packed + (size_t)((slot0 + (uint64_t)r) % cap) * row_words;
    for (int64_t base = (int64_t)blockIdx.x * REPLAY_THREADS; base < padded; base += (int64_t)gridDim.x * REPLAY_THREADS) {
      const int64_t t = base + threadIdx.x;
      const int word = (int)(t >> 4), i = (int)(t & 15);
      const int f = word / wpp, c = (word - f * wpp) * replay_pack::CODES_PER_WORD + i;
      uint32_t bits = 0;
      if (t < padded && c < mm) {
        const int code = replay_pack::code_of(p0, p1, p2, p3, n_pal, in[(size_t)f * mm + c]);
        bits = (uint32_t)(code < 0 ? 0 : code) << replay_pack::shift_of(c);   // (validated before the launch: never < 0)
      }
      bits |= (uint32_t)__shfl_xor((int)bits, 1);
      bits |= (uint32_t)__shfl_xor((int)bits, 2);
      bits |= (uint32_t)__shfl_xor((int)bits, 4);
      bits |= (uint32_t)__shfl_xor((int)bits, 8);
      if (i == 0 && t < padded) out[word] = bits;
    }
  }
}

// k_replay_sample on a packed window: the same contract, grid and draw.  A plane element is one LDS read (the symmetry's source cell),
// one read of the source cell's word — word (src >> 4) of the SAME plane, straight from global memory: 16 neighbouring cells share a word
// and a 19x19 plane is 92 bytes, so the reads of a wavefront fall into one or two cache lines — a shift, two levels of selects on the
// code bits over the palette (four uint32 kernel arguments, no table in memory) and one coalesced write.  Every output goes through a
// uint32 view of the float buffers: a NaN entry arrives with its payload.  Algorithmic bytes per row: F * wpp * 4 + (A1 + 1) * 4 read,
// (F * mm + A1 + 1) * 4 written.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_sample_packed(const uint32_t* __restrict__ packed,
                                                                         const uint32_t* __restrict__ policy,
                                                                         const uint32_t* __restrict__ value, uint32_t* __restrict__ X,
                                                                         uint32_t* __restrict__ Pi, uint32_t* __restrict__ V, int F, int m,
                                                                         int mm, int wpp, int A1, int rows, int row0, int cnt, uint64_t seed,
                                                                         uint64_t step, int symmetric, uint64_t n, uint64_t total, uint64_t cap,
                                                                         uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  __shared__ int tab[REPLAY_TAB];
  const int xs = F * mm, row = xs + A1 + 1;
  const int e0 = (int)blockIdx.x * REPLAY_SEG;
  const int e1 = min(e0 + REPLAY_SEG, row);
  for (int r = (int)blockIdx.y; r < cnt; r += (int)gridDim.y) {
    const replay::Draw d = replay::draw(seed, step, rows, row0 + r, n, symmetric != 0);
    const size_t s = (size_t)replay::slot(total, cap, d.j);
    const bool mapped = d.k != 0;     // (the host refuses symmetric sampling unless the board is square and mm <= REPLAY_TAB)
    if (mapped) {
      for (int c = (int)threadIdx.x; c < mm; c += REPLAY_THREADS) tab[c] = sym::src(m, d.k, c);
      __syncthreads();
    }
    const uint32_t* in_w = packed + s * (size_t)F * wpp;
    const uint32_t* in_p = policy + s * (size_t)A1;
    uint32_t* out_x = X + (size_t)r * xs;
    uint32_t* out_p = Pi + (size_t)r * A1;
    for (int e = e0 + (int)threadIdx.x; e < e1; e += REPLAY_THREADS) {
      if (e < xs) {
        const int pl = e / mm, c = e - pl * mm;
        const int src = mapped ? tab[c] : c;
        const uint32_t code = in_w[pl * wpp + (src >> 4)] >> replay_pack::shift_of(src);
        out_x[e] = replay_pack::decode(p0, p1, p2, p3, code);
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

// ---- the digest of a window's logical content (agz_replay_digest, DESIGN.md §2 replay-sharded; the definition is replay.hpp's) ----------

constexpr int DIGEST_ROWS = 4096;   // rows of the grid (y); the live rows are dealt to them round-robin

// *sum += the digest terms of every element of the n live rows (the host adds `live`).  The sampler's geometry: a logical row j is the
// concatenation [planes F*mm | policy A1 | value 1] cut into segments of REPLAY_SEG elements, grid = (segments, rows), rows strided.  A
// packed window (packed != NULL) contributes the decoded palette pattern of a cell, so the digest is that of the unpacked rows.  Terms are
// summed as uint64 in a lane, over the wavefront by shuffles, over the workgroup through LDS, and one atomicAdd per workgroup: an
// integer sum, the same whatever the order and the launch geometry.  The window is read once.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_digest(const uint32_t* __restrict__ planes, const uint32_t* __restrict__ packed,
                                                                  const uint32_t* __restrict__ policy, const uint32_t* __restrict__ value,
                                                                  int F, int mm, int wpp, int A1, uint64_t n, uint64_t total, uint64_t cap,
                                                                  uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3,
                                                                  unsigned long long* __restrict__ sum) {
  __shared__ unsigned long long part[REPLAY_THREADS / 64];
  const int xs = F * mm, row = xs + A1 + 1;
  const int e0 = (int)blockIdx.x * REPLAY_SEG;
  const int e1 = min(e0 + REPLAY_SEG, row);
  unsigned long long acc = 0;
  for (uint64_t j = blockIdx.y; j < n; j += gridDim.y) {
    const size_t s = (size_t)replay::slot(total, cap, j);
    const uint32_t* in_x = packed ? packed + s * (size_t)F * wpp : planes + s * (size_t)xs;
    const uint32_t* in_p = policy + s * (size_t)A1;
    for (int e = e0 + (int)threadIdx.x; e < e1; e += REPLAY_THREADS) {
      uint32_t bits;
      if (e < xs) {
        if (packed) {
          const int pl = e / mm, c = e - pl * mm;
          bits = replay_pack::decode(p0, p1, p2, p3, in_x[pl * wpp + (c >> 4)] >> replay_pack::shift_of(c));
        } else {
          bits = in_x[e];
        }
      } else if (e < xs + A1) {
        bits = in_p[e - xs];
      } else {
        bits = value[s];
      }
      acc += replay::digest_term(j, (uint64_t)row, (uint64_t)e, bits);
    }
  }
  // (every lane arrives here: the loops above have no barrier in them)
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < REPLAY_THREADS / 64; w++) t += part[w];
    atomicAdd(sum, t);
  }
}

// ---- checkpoints (agz_replay_save / agz_replay_load, DESIGN.md §2 replay-ckpt; the bytes are replay_ckpt.hpp's) ------------------------

constexpr int CKPT_BLOCKS = 4096;   // workgroups of a scan at most: a chunk is walked grid-stride

// One staged chunk of a checkpoint file, validated and digested without a look at the ring: rows [j0, j0 + cnt) of ONE of the file's three
// arrays, `n_el` words a row as they lie in the file.  acc[0] += the digest terms of the chunk's elements at their file logical index
// (replay.hpp: an integer sum, so it is taken chunk by chunk and run by run; the host adds `live` and compares with the header's word);
// acc[1] += the bad elements, acc[2] = min(acc[2], the first bad one's linear index in its array).
//   words == 0    fp32 elements: element e of a row is element e_off + e of the logical row.  wn > 0 (the planes of an fp32 file on their
//                 way into a packed window): a pattern outside the window's palette w0 .. w3 is bad, linear index j * n_el + e.
//   words == 1    packed planes, n_el = F * wpp words a row, walked in the PADDED index t = word * 16 + i of k_replay_pack: cell c = (word
//                 mod wpp) * 16 + i of plane word / wpp contributes the file palette's (p0 .. p3) pattern at element f * mm + c; a code not
//                 below pn and a set bit past the plane's last cell are bad, linear index
//                 j * n_el * 16 + t.
// The reduction is k_replay_digest's; a lane touches acc[1], acc[2] only if it met a bad element.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_ckpt_scan(const uint32_t* __restrict__ chunk, int words, uint64_t n_el, uint64_t e_off,
                                                                     uint64_t rowlen, uint64_t j0, uint64_t cnt, int mm, int wpp, uint32_t p0,
                                                                     uint32_t p1, uint32_t p2, uint32_t p3, int pn, uint32_t w0, uint32_t w1,
                                                                     uint32_t w2, uint32_t w3, int wn, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long part[REPLAY_THREADS / 64];
  unsigned long long sum = 0, bad = 0, first = PACK_NONE;
  const uint64_t per_row = words ? n_el * replay_pack::CODES_PER_WORD : n_el;
  const uint64_t n = cnt * per_row, stride = (uint64_t)gridDim.x * REPLAY_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * REPLAY_THREADS + threadIdx.x; i < n; i += stride) {
    const uint64_t r = i / per_row, t = i - r * per_row, j = j0 + r;
    if (words) {
      const uint64_t word = t >> 4;
      const int f = (int)(word / (uint64_t)wpp), c = (int)(word - (uint64_t)f * wpp) * replay_pack::CODES_PER_WORD + (int)(t & 15);
      const uint32_t code = (chunk[r * n_el + word] >> replay_pack::shift_of(c)) & (uint32_t)(replay_pack::MAX_PALETTE - 1);
      if (c < mm) {
        if ((int)code >= pn) { bad++; if (j * per_row + t < first) first = j * per_row + t; }
        sum += replay::digest_term(j, rowlen, e_off + (uint64_t)f * mm + c, replay_pack::decode(p0, p1, p2, p3, code));
      } else if (code != 0) {
        bad++;
        if (j * per_row + t < first) first = j * per_row + t;
      }
    } else {
      const uint32_t bits = chunk[i];
      if (wn > 0 && replay_pack::code_of(w0, w1, w2, w3, wn, bits) < 0) { bad++; if (j * per_row + t < first) first = j * per_row + t; }
      sum += replay::digest_term(j, rowlen, e_off + t, bits);
    }
  }
  if (bad) {
    atomicAdd(&acc[1], bad);
    atomicMin(&acc[2], first);
  }
  // (every lane arrives here: the loop above has no barrier in it)
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < REPLAY_THREADS / 64; w++) s += part[w];
    atomicAdd(&acc[0], s);
  }
}

// A staged chunk of PACKED planes a scan has accepted ([rows][F * wpp] words under the file's palette p0 .. p3) into the ring slots
// (slot0 + r) mod cap of a window of the other form or another palette.  planes != NULL: an fp32 window, one lane a cell, the file
// palette's pattern of its code.  Otherwise a packed window: one lane a word, every code c of a cell replaced by (remap >> 2 c) & 3, the
// window's code of the same pattern (the host built the table; every file entry is in the window's palette); the bits past a plane's last
// cell stay zero.  An fp32 chunk on its way into a packed window takes k_replay_pack.
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_ckpt_put(const uint32_t* __restrict__ chunk, uint32_t* __restrict__ planes,
                                                                    uint32_t* __restrict__ packed, int F, int mm, int wpp, int rows,
                                                                    uint64_t slot0, uint64_t cap, uint32_t p0, uint32_t p1, uint32_t p2,
                                                                    uint32_t p3, uint32_t remap) {
  const int row_words = F * wpp, xs = F * mm;
  for (int r = (int)blockIdx.y; r < rows; r += (int)gridDim.y) {
    const uint32_t* in = chunk + (size_t)r * row_words;
    const size_t s = (size_t)((slot0 + (uint64_t)r) % cap);
    if (planes) {
      uint32_t* out = planes + s * (size_t)xs;
      for (int e = (int)blockIdx.x * REPLAY_THREADS + threadIdx.x; e < xs; e += (int)gridDim.x * REPLAY_THREADS) {
        const int f = e / mm, c = e - f * mm;
        out[e] = replay_pack::decode(p0, p1, p2, p3, in[f * wpp + (c >> 4)] >> replay_pack::shift_of(c));
      }
    } else {
      uint32_t* out = packed + s * (size_t)row_words;
      for (int w = (int)blockIdx.x * REPLAY_THREADS + threadIdx.x; w < row_words; w += (int)gridDim.x * REPLAY_THREADS) {
        const int c0 = (w % wpp) * replay_pack::CODES_PER_WORD, cells = min(replay_pack::CODES_PER_WORD, mm - c0);
        const uint32_t word = in[w];
        uint32_t bits = 0;
        for (int i = 0; i < cells; i++) {
          const uint32_t code = (word >> (replay_pack::CODE_BITS * i)) & 3u;
          bits |= ((remap >> (replay_pack::CODE_BITS * code)) & 3u) << (replay_pack::CODE_BITS * i);
        }
        out[w] = bits;
      }
    }
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
  // rows below this append number were never stored: 0 except after agz_replay_load put a file that does not fill the window (live <
  // min(total, cap)) into it.  The ring then counts from `base`: row number g lives in slot (g - base) mod cap, live = min(total - base, cap).
  uint64_t base = 0;
  // a packed window (agz_replay_create_packed): `planes` stays NULL, the planes live in `words` [cap][F * wpp] under `pal`
  bool is_packed = false;
  uint32_t* words = nullptr;
  int wpp = 0;
  replay_pack::Palette pal{};
  size_t ckpt_staging = 256u << 20;   // bytes of the device buffer and of each of the two page-locked host buffers of a save or load (agz_replay_set_ckpt_staging)

  uint64_t ring_total() const { return total - base; }   // what replay.hpp's ring arithmetic takes as `total`
  uint64_t live() const { return replay::live(ring_total(), cap); }
  size_t row_words() const { return (size_t)F * wpp; }
  size_t row_bytes() const { return ((is_packed ? row_words() : xs) + (size_t)A1 + 1) * 4; }

  // A packed append takes all rows or none: every one of the c rows of p (device memory unless kind is host to device) is checked against
  // the palette before anything is written.  One 16-byte read-back: the context's queue is synchronised once.
  int validate(const float* p, uint64_t c, hipMemcpyKind kind, const char* who) {
    const uint64_t nel = c * xs;
    uint64_t first = PACK_NONE;
    uint32_t bits = 0;
    if (kind == hipMemcpyHostToDevice) {
      const uint32_t* u = reinterpret_cast<const uint32_t*>(p);
      for (uint64_t i = 0; i < nel && first == PACK_NONE; i++)
        if (replay_pack::code_of(pal, u[i]) < 0) { first = i; bits = u[i]; }
    } else {
      hipStream_t s = ctx->stream;
      unsigned long long* chk = nullptr;
      unsigned long long got[2] = {0, PACK_NONE};
      AGZ_HIP_TRY(hipMalloc(&chk, sizeof(got)));
      hipError_t e = hipMemsetAsync(chk, 0, 8, s);
      if (e == hipSuccess) e = hipMemsetAsync(chk + 1, 0xFF, 8, s);   // PACK_NONE
      if (e == hipSuccess) {
        const unsigned grid = (unsigned)std::min<uint64_t>((nel + REPLAY_THREADS - 1) / REPLAY_THREADS, 4096);
        hipLaunchKernelGGL(k_replay_pack_check, dim3(grid), dim3(REPLAY_THREADS), 0, s, reinterpret_cast<const uint32_t*>(p), nel, pal.e[0],
                           pal.e[1], pal.e[2], pal.e[3], pal.n, chk);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipMemcpyAsync(got, chk, sizeof(got), hipMemcpyDeviceToHost, s);
      const hipError_t se = hipStreamSynchronize(s);
      if (e == hipSuccess && se == hipSuccess && got[0]) e = hipMemcpy(&bits, reinterpret_cast<const uint32_t*>(p) + got[1], 4, hipMemcpyDeviceToHost);
      hipFree(chk);
      AGZ_HIP_TRY(e);
      AGZ_HIP_TRY(se);
      if (got[0]) first = got[1];
    }
    AGZ_REQUIRE(first == PACK_NONE, AGZ_E_INVALID,
                "%s: row %llu, element %llu (linear element %llu) holds the bit pattern 0x%08X, which is not in the window's palette; "
                "nothing was appended",
                who, (unsigned long long)(first / xs), (unsigned long long)(first % xs), (unsigned long long)first, bits);
    return AGZ_OK;
  }
  // cnt validated source rows into the slots from s0 on (wrapping): device rows are packed where they lie, host rows go up through a
  // bounded staging buffer, chunk after chunk in queue order
  int pack_rows(const float* p, uint64_t cnt, uint64_t s0, hipMemcpyKind kind) {
    hipStream_t s = ctx->stream;
    const int mm = H * W;
    const unsigned gx = (unsigned)std::min<size_t>((row_words() * replay_pack::CODES_PER_WORD + REPLAY_THREADS - 1) / REPLAY_THREADS, 1024);
    const bool host = kind == hipMemcpyHostToDevice;
    const uint64_t chunk = host ? std::min<uint64_t>(cnt, std::max<uint64_t>(1, PACK_STAGING_BYTES / (xs * 4))) : cnt;
    float* staging = nullptr;
    if (host && hipMalloc(&staging, chunk * xs * 4) != hipSuccess) {
      (void)hipGetLastError();
      agz::set_error("agz_replay_append_host: out of device memory for a staging buffer of %llu rows", (unsigned long long)chunk);
      return AGZ_E_NOMEM;
    }
    hipError_t e = hipSuccess;
    for (uint64_t a = 0; a < cnt && e == hipSuccess; a += chunk) {
      const uint64_t len = std::min(chunk, cnt - a);
      const float* src = p + a * xs;
      if (host) {
        e = hipMemcpyAsync(staging, src, len * xs * 4, hipMemcpyHostToDevice, s);
        src = staging;
        if (e != hipSuccess) break;
      }
      hipLaunchKernelGGL(k_replay_pack, dim3(gx, (unsigned)std::min<uint64_t>(len, 65535)), dim3(REPLAY_THREADS), 0, s,
                         reinterpret_cast<const uint32_t*>(src), words, F, mm, wpp, (int)len, (s0 + a) % cap, cap, pal.e[0], pal.e[1], pal.e[2],
                         pal.e[3], pal.n);
      e = hipGetLastError();
    }
    if (host) {
      const hipError_t se = hipStreamSynchronize(s);   // the staging buffer is read by the kernels enqueued above
      hipFree(staging);
      if (e == hipSuccess) e = se;
    }
    AGZ_HIP_TRY(e);
    return AGZ_OK;
  }
  // c rows from (p, q, v) as c single-row appends in order: at most two contiguous row ranges per array; only the last cap rows of a
  // longer append survive
  // checkpoints (agz_replay_save / agz_replay_load, at the end of this file)
  replay_ckpt::Header ckpt_header() const;
  char* ckpt_array(int k) const;
  int ckpt_write(FILE* f, const replay_ckpt::Layout& l);
  int ckpt_read(FILE* f, const char* path, const replay_ckpt::Header& h, const replay_ckpt::Layout& l, bool commit);
  int append(const float* p, const float* q, const float* v, uint64_t c, hipMemcpyKind kind, const char* who) {
    if (is_packed) {
      AGZ_REQUIRE(c <= (uint64_t)INT32_MAX, AGZ_E_INVALID, "%s: %llu rows in one append to a packed window (at most %d)", who,
                  (unsigned long long)c, INT32_MAX);
      int r = validate(p, c, kind, who);
      if (r != AGZ_OK) return r;
    }
    const uint64_t skip = c > cap ? c - cap : 0, cnt = c - skip;
    const uint64_t s0 = replay::head(ring_total() + skip, cap);
    const uint64_t first = std::min<uint64_t>(cnt, cap - s0);
    hipStream_t s = ctx->stream;
    if (is_packed) {
      int r = pack_rows(p + skip * xs, cnt, s0, kind);
      if (r != AGZ_OK) return r;
    }
    const uint64_t at[2] = {skip, skip + first}, to[2] = {s0, 0}, len[2] = {first, cnt - first};
    for (int i = 0; i < 2; i++) {
      if (!len[i]) continue;
      if (!is_packed) AGZ_HIP_TRY(hipMemcpyAsync(planes + to[i] * xs, p + at[i] * xs, len[i] * xs * 4, kind, s));
      AGZ_HIP_TRY(hipMemcpyAsync(policy + to[i] * A1, q + at[i] * A1, len[i] * (size_t)A1 * 4, kind, s));
      AGZ_HIP_TRY(hipMemcpyAsync(value + to[i], v + at[i], len[i] * 4, kind, s));
    }
    total += c;
    return AGZ_OK;
  }
};

ReplayInfo agz::replay_info(const agz_replay* rp) { return ReplayInfo{rp->ctx, rp->F, rp->H, rp->W, rp->A1, rp->ring_total(), rp->cap, rp->is_packed}; }

int agz::replay_check_symmetric(const agz_replay* rp, int symmetric, const char* who) {
  if (!symmetric) return AGZ_OK;
  AGZ_REQUIRE(rp->H == rp->W, AGZ_E_INVALID, "Cannot handle m %d, n %d. This function only takes square boards", rp->H, rp->W);
  AGZ_REQUIRE(rp->A1 >= rp->H * rp->W, AGZ_E_INVALID, "%s: policy shorter than the board", who);
  AGZ_REQUIRE(rp->H * rp->W <= REPLAY_TAB, AGZ_E_INVALID, "%s: symmetric sampling takes boards of at most %d cells", who, REPLAY_TAB);
  return AGZ_OK;
}

int agz::replay_sample_launch(agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric, uint64_t n,
                              uint64_t total, float* X, float* Pi, float* V) {
  const int mm = rp->H * rp->W;
  const int row = (int)rp->xs + rp->A1 + 1;
  const dim3 grid((unsigned)ceil_div(row, REPLAY_SEG), (unsigned)std::min(cnt, 65535));
  if (rp->is_packed) {
    const replay_pack::Palette& pal = rp->pal;
    hipLaunchKernelGGL(k_replay_sample_packed, grid, dim3(REPLAY_THREADS), 0, rp->ctx->stream, rp->words,
                       reinterpret_cast<const uint32_t*>(rp->policy), reinterpret_cast<const uint32_t*>(rp->value),
                       reinterpret_cast<uint32_t*>(X), reinterpret_cast<uint32_t*>(Pi), reinterpret_cast<uint32_t*>(V), rp->F, rp->H, mm, rp->wpp,
                       rp->A1, rows, row0, cnt, seed, step, symmetric, n, total, rp->cap, pal.e[0], pal.e[1], pal.e[2], pal.e[3]);
    AGZ_HIP_TRY(hipGetLastError());
    return AGZ_OK;
  }
  hipLaunchKernelGGL(k_replay_sample, grid, dim3(REPLAY_THREADS), 0, rp->ctx->stream, rp->planes, rp->policy, rp->value, X, Pi, V, rp->F,
                     rp->H, mm, rp->A1, rows, row0, cnt, seed, step, symmetric, n, total, rp->cap);
  AGZ_HIP_TRY(hipGetLastError());
  return AGZ_OK;
}

// rows [row0, row0 + cnt) of a minibatch of `rows` rows: the slice calls' own argument check
static int check_slice(const char* who, int rows, int row0, int cnt) {
  AGZ_REQUIRE(rows >= 1 && row0 >= 0 && cnt >= 1 && (int64_t)row0 + cnt <= rows, AGZ_E_INVALID,
              "%s: rows [%d, %lld) of a minibatch of %d (rows >= 1, row0 >= 0, cnt >= 1 and row0 + cnt <= rows)", who, row0,
              (long long)row0 + cnt, rows);
  return AGZ_OK;
}

// the body of the four public samplers, arguments checked: into device buffers, asynchronous ...
static int sample_slice_dev(const char* who, agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric,
                            float* X_dev, float* Pi_dev, float* V_dev) {
  int r = replay_check_symmetric(rp, symmetric, who);
  if (r != AGZ_OK) return r;
  AGZ_REQUIRE(rp->total > 0, AGZ_E_STATE, "%s: the window is empty", who);
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  return replay_sample_launch(rp, rows, row0, cnt, seed, step, symmetric, rp->live(), rp->ring_total(), X_dev, Pi_dev, V_dev);
}
// ... and into host buffers of cnt rows
static int sample_slice_host(const char* who, agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric,
                             float* X, float* Pi, float* V) {
  int r = replay_check_symmetric(rp, symmetric, who);
  if (r != AGZ_OK) return r;
  AGZ_REQUIRE(rp->total > 0, AGZ_E_STATE, "%s: the window is empty", who);
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  const size_t nx = (size_t)cnt * rp->xs, np = (size_t)cnt * rp->A1, nv = (size_t)cnt;
  float* d = nullptr;
  if (hipMalloc(&d, (nx + np + nv) * 4) != hipSuccess) {
    (void)hipGetLastError();
    agz::set_error("%s: out of device memory for %d rows", who, cnt);
    return AGZ_E_NOMEM;
  }
  hipStream_t s = rp->ctx->stream;
  r = replay_sample_launch(rp, rows, row0, cnt, seed, step, symmetric, rp->live(), rp->ring_total(), d, d + nx, d + nx + np);
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

// the two creates: pal == nullptr keeps the planes as fp32 rows, otherwise as 2-bit codes under *pal
static int replay_create(const char* who, agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, int64_t capacity,
                         const replay_pack::Palette* pal, agz_replay** out) {
  AGZ_REQUIRE(ctx && out, AGZ_E_INVALID, "%s: NULL argument", who);
  AGZ_REQUIRE(Features >= 1 && Height >= 1 && Width >= 1 && PolicyLen >= 1, AGZ_E_INVALID, "%s: bad shape", who);
  AGZ_REQUIRE(capacity >= 1, AGZ_E_INVALID, "%s: capacity %lld (at least 1 row)", who, (long long)capacity);
  const size_t xs = (size_t)Features * Height * Width;
  AGZ_REQUIRE(xs + (size_t)PolicyLen + 1 <= (size_t)1 << 30, AGZ_E_INVALID, "%s: a row of %zu floats is too long", who, xs + PolicyLen + 1);
  AGZ_HIP_TRY(hipSetDevice(ctx->device));
  const size_t cap = (size_t)capacity;
  const int wpp = pal ? replay_pack::wpp(Height * Width) : 0;
  const size_t plane_bytes = pal ? (size_t)Features * wpp * 4 : xs * 4;      // of one row
  void* p = nullptr;
  float *q = nullptr, *v = nullptr;
  if (hipMalloc(&p, cap * plane_bytes) != hipSuccess || hipMalloc(&q, cap * PolicyLen * 4) != hipSuccess || hipMalloc(&v, cap * 4) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(p); hipFree(q); hipFree(v);
    agz::set_error("%s: out of device memory for a window of %zu rows (%zu bytes)", who, cap, cap * (plane_bytes + ((size_t)PolicyLen + 1) * 4));
    return AGZ_E_NOMEM;
  }
  agz_replay* rp = new agz_replay();
  rp->ctx = ctx; rp->F = Features; rp->H = Height; rp->W = Width; rp->A1 = PolicyLen; rp->xs = xs;
  rp->policy = q; rp->value = v; rp->cap = (uint64_t)cap;
  if (pal) {
    rp->is_packed = true; rp->words = static_cast<uint32_t*>(p); rp->wpp = wpp; rp->pal = *pal;
  } else {
    rp->planes = static_cast<float*>(p);
  }
  *out = rp;
  return AGZ_OK;
}

// a palette handed over as floats, taken as bit patterns
static int palette_of(const char* who, const float* palette, int n_palette, replay_pack::Palette* pal) {
  AGZ_REQUIRE(n_palette >= 1 && n_palette <= replay_pack::MAX_PALETTE, AGZ_E_INVALID, "%s: a palette of %d entries (1 to %d)", who, n_palette,
              replay_pack::MAX_PALETTE);
  AGZ_REQUIRE(palette, AGZ_E_INVALID, "%s: NULL palette", who);
  uint32_t bits[replay_pack::MAX_PALETTE];
  memcpy(bits, palette, (size_t)n_palette * 4);
  AGZ_REQUIRE(replay_pack::palette_ok(bits, n_palette), AGZ_E_INVALID, "%s: two palette entries have the same bit pattern", who);
  *pal = replay_pack::make_palette(bits, n_palette);
  return AGZ_OK;
}

extern "C" {

int agz_replay_create(agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, int64_t capacity, agz_replay** out) {
  return replay_create("agz_replay_create", ctx, Features, Height, Width, PolicyLen, capacity, nullptr, out);
}

int agz_replay_create_packed(agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, int64_t capacity, const float* palette,
                             int n_palette, agz_replay** out) {
  AGZ_REQUIRE(ctx && out, AGZ_E_INVALID, "agz_replay_create_packed: NULL argument");
  replay_pack::Palette pal;
  int r = palette_of("agz_replay_create_packed", palette, n_palette, &pal);
  if (r != AGZ_OK) return r;
  return replay_create("agz_replay_create_packed", ctx, Features, Height, Width, PolicyLen, capacity, &pal, out);
}

int agz_encoder_palette(int encoder, float palette[4], int* n) {
  AGZ_REQUIRE(palette && n, AGZ_E_INVALID, "agz_encoder_palette: NULL argument");
  AGZ_REQUIRE(encoder == AGZ_ENC_WQ || encoder == AGZ_ENC_TWOPLANE, AGZ_E_INVALID, "agz_encoder_palette: unknown encoder %d", encoder);
  // the literals encode_nchw (engine.hip) writes; WQ's opponent planes hold -0.0 in empty cells, as vecf32.Scale gives them
  palette[0] = encoder == AGZ_ENC_WQ ? 0.0f : 0.001f;
  palette[1] = encoder == AGZ_ENC_WQ ? -0.0f : 0.0f;
  palette[2] = 1.0f;
  palette[3] = -1.0f;
  *n = 4;
  return AGZ_OK;
}

int agz_replay_pack_host(const float* planes, int64_t n, int Features, int cells, const float* palette, int n_palette, uint32_t* words,
                         int64_t* first_bad) {
  replay_pack::Palette pal;
  int r = palette_of("agz_replay_pack_host", palette, n_palette, &pal);
  if (r != AGZ_OK) return r;
  AGZ_REQUIRE(n >= 0 && Features >= 1 && cells >= 1 && (n == 0 || planes), AGZ_E_INVALID, "agz_replay_pack_host: bad argument");
  const int64_t xs = (int64_t)Features * cells, rw = (int64_t)Features * replay_pack::wpp(cells);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(planes);
  if (first_bad) *first_bad = -1;
  for (int64_t row = 0; row < n; row++) {   // validate everything first: `words` is written only if every cell has a code
    const int64_t bad = replay_pack::pack_row(pal, bits + row * xs, Features, cells, nullptr);
    if (bad >= 0) {
      if (first_bad) *first_bad = row * xs + bad;
      agz::set_error("agz_replay_pack_host: row %lld, element %lld holds the bit pattern 0x%08X, which is not in the palette", (long long)row,
                     (long long)bad, bits[row * xs + bad]);
      return AGZ_E_INVALID;
    }
  }
  if (words)
    for (int64_t row = 0; row < n; row++) replay_pack::pack_row(pal, bits + row * xs, Features, cells, words + row * rw);
  return AGZ_OK;
}

int agz_replay_storage(const agz_replay* rp, int32_t* packed, int64_t* row_bytes, int64_t* device_bytes) {
  AGZ_REQUIRE(rp, AGZ_E_INVALID, "agz_replay_storage: NULL window");
  if (packed) *packed = rp->is_packed ? 1 : 0;
  if (row_bytes) *row_bytes = (int64_t)rp->row_bytes();
  if (device_bytes) *device_bytes = (int64_t)(rp->cap * rp->row_bytes());   // the three arrays of create: nothing else stays allocated
  return AGZ_OK;
}

void agz_replay_destroy(agz_replay* rp) {
  if (!rp) return;
  hipSetDevice(rp->ctx->device);
  hipStreamSynchronize(rp->ctx->stream);
  hipFree(rp->planes); hipFree(rp->words); hipFree(rp->policy); hipFree(rp->value);
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
  rp->base = 0;
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
  return rp->append(e.planes, e.policy, e.value, e.n, hipMemcpyDeviceToDevice, "agz_replay_append_examples");   // (same queue as the set's own appends: ordered after them)
}

int agz_replay_append_dev(agz_replay* rp, const float* planes_dev, const float* policy_dev, const float* value_dev, int64_t n) {
  AGZ_REQUIRE(rp && n >= 0 && (n == 0 || (planes_dev && policy_dev && value_dev)), AGZ_E_INVALID, "agz_replay_append_dev: bad argument");
  if (n == 0) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  return rp->append(planes_dev, policy_dev, value_dev, (uint64_t)n, hipMemcpyDeviceToDevice, "agz_replay_append_dev");
}

int agz_replay_append_host(agz_replay* rp, const float* planes, const float* policy, const float* value, int64_t n) {
  AGZ_REQUIRE(rp && n >= 0 && (n == 0 || (planes && policy && value)), AGZ_E_INVALID, "agz_replay_append_host: bad argument");
  if (n == 0) return AGZ_OK;
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  int r = rp->append(planes, policy, value, (uint64_t)n, hipMemcpyHostToDevice, "agz_replay_append_host");
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
  const uint64_t s0 = replay::slot(rp->ring_total(), rp->cap, (uint64_t)j0);
  const uint64_t first = std::min<uint64_t>((uint64_t)cnt, rp->cap - s0);
  const uint64_t at[2] = {0, first}, from[2] = {s0, 0}, len[2] = {first, (uint64_t)cnt - first};
  for (int i = 0; i < 2; i++) {
    if (!len[i]) continue;
    if (planes && rp->is_packed) {   // the words come down as they are and are decoded here, by the header's definition
      const size_t rw = rp->row_words();
      std::vector<uint32_t> w(len[i] * rw);
      AGZ_HIP_TRY(hipMemcpy(w.data(), rp->words + from[i] * rw, w.size() * 4, hipMemcpyDeviceToHost));
      for (uint64_t r = 0; r < len[i]; r++)
        replay_pack::unpack_row(rp->pal, w.data() + r * rw, rp->F, rp->H * rp->W, reinterpret_cast<uint32_t*>(planes + (at[i] + r) * rp->xs));
    } else if (planes) {
      AGZ_HIP_TRY(hipMemcpy(planes + at[i] * rp->xs, rp->planes + from[i] * rp->xs, len[i] * rp->xs * 4, hipMemcpyDeviceToHost));
    }
    if (policy) AGZ_HIP_TRY(hipMemcpy(policy + at[i] * rp->A1, rp->policy + from[i] * rp->A1, len[i] * (size_t)rp->A1 * 4, hipMemcpyDeviceToHost));
    if (value) AGZ_HIP_TRY(hipMemcpy(value + at[i], rp->value + from[i], len[i] * 4, hipMemcpyDeviceToHost));
  }
  return AGZ_OK;
}

int agz_replay_sample_dev(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, float* X_dev, float* Pi_dev, float* V_dev) {
  AGZ_REQUIRE(rp && X_dev && Pi_dev && V_dev, AGZ_E_INVALID, "agz_replay_sample_dev: NULL argument");
  AGZ_REQUIRE(rows >= 1, AGZ_E_INVALID, "agz_replay_sample_dev: rows %d (at least 1)", rows);
  return sample_slice_dev("agz_replay_sample_dev", rp, rows, 0, rows, seed, step, symmetric, X_dev, Pi_dev, V_dev);
}

int agz_replay_sample(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, float* X, float* Pi, float* V) {
  AGZ_REQUIRE(rp && X && Pi && V, AGZ_E_INVALID, "agz_replay_sample: NULL argument");
  AGZ_REQUIRE(rows >= 1, AGZ_E_INVALID, "agz_replay_sample: rows %d (at least 1)", rows);
  return sample_slice_host("agz_replay_sample", rp, rows, 0, rows, seed, step, symmetric, X, Pi, V);
}

int agz_replay_sample_slice_dev(agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric, float* X_dev,
                                float* Pi_dev, float* V_dev) {
  AGZ_REQUIRE(rp && X_dev && Pi_dev && V_dev, AGZ_E_INVALID, "agz_replay_sample_slice_dev: NULL argument");
  int r = check_slice("agz_replay_sample_slice_dev", rows, row0, cnt);
  if (r != AGZ_OK) return r;
  return sample_slice_dev("agz_replay_sample_slice_dev", rp, rows, row0, cnt, seed, step, symmetric, X_dev, Pi_dev, V_dev);
}

int agz_replay_sample_slice(agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric, float* X, float* Pi,
                            float* V) {
  AGZ_REQUIRE(rp && X && Pi && V, AGZ_E_INVALID, "agz_replay_sample_slice: NULL argument");
  int r = check_slice("agz_replay_sample_slice", rows, row0, cnt);
  if (r != AGZ_OK) return r;
  return sample_slice_host("agz_replay_sample_slice", rp, rows, row0, cnt, seed, step, symmetric, X, Pi, V);
}

int agz_replay_digest(agz_replay* rp, uint64_t* digest) {
  AGZ_REQUIRE(rp && digest, AGZ_E_INVALID, "agz_replay_digest: NULL argument");
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  hipStream_t s = rp->ctx->stream;
  const uint64_t n = rp->live();
  unsigned long long* d = nullptr;
  unsigned long long got = 0;
  AGZ_HIP_TRY(hipMalloc(&d, 8));
  hipError_t e = hipMemsetAsync(d, 0, 8, s);
  if (e == hipSuccess && n) {
    const int row = (int)rp->xs + rp->A1 + 1;
    const dim3 grid((unsigned)ceil_div(row, REPLAY_SEG), (unsigned)std::min<uint64_t>(n, DIGEST_ROWS));
    const replay_pack::Palette& pal = rp->pal;   // (an unpacked window's is all zero and unused)
    hipLaunchKernelGGL(k_replay_digest, grid, dim3(REPLAY_THREADS), 0, s, reinterpret_cast<const uint32_t*>(rp->planes), rp->words,
                       reinterpret_cast<const uint32_t*>(rp->policy), reinterpret_cast<const uint32_t*>(rp->value), rp->F, rp->H * rp->W,
                       rp->wpp, rp->A1, n, rp->ring_total(), rp->cap, pal.e[0], pal.e[1], pal.e[2], pal.e[3], d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&got, d, 8, hipMemcpyDeviceToHost, s);
  const hipError_t se = hipStreamSynchronize(s);
  hipFree(d);
  AGZ_HIP_TRY(e);
  AGZ_HIP_TRY(se);
  *digest = n + (uint64_t)got;
  return AGZ_OK;
}

int agz_replay_digest_host(const float* planes, const float* policy, const float* value, int64_t n, int Features, int cells, int PolicyLen,
                           uint64_t* digest) {
  AGZ_REQUIRE(digest && n >= 0 && Features >= 1 && cells >= 1 && PolicyLen >= 1 && (n == 0 || (planes && policy && value)), AGZ_E_INVALID,
              "agz_replay_digest_host: bad argument");
  *digest = replay::digest_rows(reinterpret_cast<const uint32_t*>(planes), reinterpret_cast<const uint32_t*>(policy),
                                reinterpret_cast<const uint32_t*>(value), (uint64_t)n, (uint64_t)Features * (uint64_t)cells, (uint64_t)PolicyLen);
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

// ---- checkpoints (agz_replay_save / agz_replay_load) ----------------------------------------------------------------------------------
// The bytes are replay_ckpt.hpp's, and so are the chunks (row_chunks); this side describes the window and streams its three arrays
// through ckpt_stream.hpp's pump (stream_out, stream_in) with buffers of ckpt_staging bytes.  A chunk is a range of logical rows of one
// array; a logical range is at most two contiguous slot ranges (replay::slot), so a save needs no kernel and no device buffer.  A load
// reads the file twice: k_replay_ckpt_scan sees every chunk in the staging buffer first and nothing of the ring is touched until the whole
// file has passed; only then is it streamed again, into the ring.  The file itself is atomic_file.hpp's: whole, or the previous one.
replay_ckpt::Header agz_replay::ckpt_header() const {
  replay_ckpt::Header h{};
  h.F = (uint32_t)F; h.H = (uint32_t)H; h.W = (uint32_t)W; h.A1 = (uint32_t)A1;
  h.form = is_packed ? 1u : 0u;
  h.n_palette = is_packed ? (uint32_t)pal.n : 0u;
  for (int i = 0; i < pal.n && is_packed; i++) h.palette[i] = pal.e[i];
  h.total = total; h.live = live();
  // the capacity word is informational beyond the file's own rule live == min(total, capacity).  A window that a larger-capacity load left
  // not yet full (base != 0: live < min(total, cap)) writes its live count there, the capacity of the smallest window that holds these
  // rows of this total: the file is then sound by that rule and loads anywhere, as any other
  h.capacity = base ? h.live : cap;
  return h;
}

char* agz_replay::ckpt_array(int k) const {
  return k == replay_ckpt::PLANES ? (is_packed ? (char*)words : (char*)planes) : k == replay_ckpt::POLICY ? (char*)policy : (char*)value;
}

// the three arrays and the end mark behind a written head.  AGZ_E_INVALID: the file system refused a write.
int agz_replay::ckpt_write(FILE* f, const replay_ckpt::Layout& l) {
  hipStream_t s = ctx->stream;
  std::vector<replay_ckpt::Chunk> ch;
  const size_t bytes = (size_t)replay_ckpt::row_chunks(l, 0, live(), ckpt_staging, [&](const replay_ckpt::Chunk& c) { ch.push_back(c); });
  CkptStaging st;
  int r = st.init(s, bytes, false);
  if (r != AGZ_OK) return r;
  r = stream_out(st, ch.size(),
    [&](size_t i, void* host) -> int {   // the one or two slot ranges of the chunk's rows
      const replay_ckpt::Chunk& c = ch[i];
      const uint64_t rb = l.row_bytes[c.k], s0 = replay::slot(ring_total(), cap, c.j0), first = std::min(c.cnt, cap - s0);
      char* to = (char*)host;
      AGZ_HIP_TRY(hipMemcpyAsync(to, ckpt_array(c.k) + s0 * rb, first * rb, hipMemcpyDeviceToHost, s));
      if (c.cnt > first) AGZ_HIP_TRY(hipMemcpyAsync(to + first * rb, ckpt_array(c.k), (c.cnt - first) * rb, hipMemcpyDeviceToHost, s));
      return AGZ_OK;
    },
    [&](size_t i, void* host) -> int { AGZ_REQUIRE(replay_ckpt::write_rows(f, l, ch[i].k, ch[i].j0, ch[i].cnt, host), AGZ_E_INVALID, "agz_replay_save: write failed"); return AGZ_OK; });
  if (r != AGZ_OK) return r;
  AGZ_REQUIRE(replay_ckpt::write_end(f, l), AGZ_E_INVALID, "agz_replay_save: write failed");
  return AGZ_OK;
}

// One pass over a file whose head read_head() has accepted.  commit == false: every chunk goes through the device staging buffer and
// k_replay_ckpt_scan; the codes, the unused bits, the palette membership and the digest are checked and NOTHING of the window changes.
// commit == true (after such a pass): the newest min(live, cap) rows go into the slots replay.hpp gives them, in the window's form, and
// total := the file's.  A device error in the committing pass leaves the window's content undefined.
int agz_replay::ckpt_read(FILE* f, const char* path, const replay_ckpt::Header& h, const replay_ckpt::Layout& l, bool commit) {
  hipStream_t s = ctx->stream;
  const int mm = H * W;
  const replay_pack::Palette fpal = h.form ? replay_pack::make_palette(h.palette, (int)h.n_palette) : replay_pack::Palette{};
  const int fwpp = replay_pack::wpp(mm);
  // the planes need a kernel unless the file holds them as the window does
  bool same_planes = (h.form != 0) == is_packed;
  uint32_t remap = 0;
  if (h.form && is_packed) {
    for (int c = 0; c < fpal.n; c++) {
      const int code = replay_pack::code_of(pal, fpal.e[c]);
      AGZ_REQUIRE(code >= 0, AGZ_E_INVALID, "agz_replay_load: entry %d of the palette of %s, the bit pattern 0x%08X, is not in the window's palette", c, path, fpal.e[c]);
      remap |= (uint32_t)code << (replay_pack::CODE_BITS * c);
      same_planes = same_planes && code == c;
    }
  }
  const uint64_t keep = std::min<uint64_t>(h.live, cap), skip = commit ? h.live - keep : 0;
  // a file that fills this window (keep == min(total, cap)) lies as its appends laid it, row number g in slot g mod cap; one that does not
  // starts the ring anew at its oldest row
  const uint64_t new_base = keep == replay::live(h.total, cap) ? 0 : h.total - keep;
  std::vector<replay_ckpt::Chunk> ch;
  const size_t bytes = (size_t)replay_ckpt::row_chunks(l, skip, h.live, ckpt_staging, [&](const replay_ckpt::Chunk& c) { ch.push_back(c); });
  CkptStaging st;
  CkptScratch acc_mem;   // the scan's sum, bad count, first bad index
  int r;
  if ((r = st.init(s, bytes, true)) != AGZ_OK || (r = acc_mem.init(s, 3 * sizeof(unsigned long long))) != AGZ_OK) return r;
  unsigned long long* acc = static_cast<unsigned long long*>(acc_mem.p);
  if (!commit) {
    AGZ_HIP_TRY(hipMemsetAsync(acc, 0, 16, s));
    AGZ_HIP_TRY(hipMemsetAsync(acc + 2, 0xFF, 8, s));   // PACK_NONE
  }
  // (commit) the slot the append of the chunk's first row wrote, or would have; a plain copy unless the planes need a kernel
  auto slot_of = [&](const replay_ckpt::Chunk& c) { return (h.total - h.live + c.j0 - new_base) % cap; };
  auto plain = [&](const replay_ckpt::Chunk& c) { return commit && (c.k != replay_ckpt::PLANES || same_planes); };
  r = stream_in(st, ch.size(),
    [&](size_t i, void* host) -> int { AGZ_REQUIRE(replay_ckpt::read_rows(f, l, ch[i].k, ch[i].j0, ch[i].cnt, host), AGZ_E_INVALID, "agz_replay_load: reading %s failed", path); return AGZ_OK; },
    [&](size_t i, void* host) -> int {
      const replay_ckpt::Chunk& c = ch[i];
      const uint64_t rb = l.row_bytes[c.k];
      const char* from = (const char*)host;
      if (plain(c)) {   // into the one or two slot ranges
        const uint64_t slot0 = slot_of(c), first = std::min(c.cnt, cap - slot0);
        AGZ_HIP_TRY(hipMemcpyAsync(ckpt_array(c.k) + slot0 * rb, from, first * rb, hipMemcpyHostToDevice, s));
        if (c.cnt > first) AGZ_HIP_TRY(hipMemcpyAsync(ckpt_array(c.k), from + first * rb, (c.cnt - first) * rb, hipMemcpyHostToDevice, s));
      } else {
        AGZ_HIP_TRY(hipMemcpyAsync(st.dev, from, c.cnt * rb, hipMemcpyHostToDevice, s));
      }
      return AGZ_OK;
    },
    [&](size_t i) -> int {
      const replay_ckpt::Chunk& c = ch[i];
      if (plain(c)) return AGZ_OK;
      const bool planes_k = c.k == replay_ckpt::PLANES;
      const uint64_t rb = l.row_bytes[c.k], slot0 = slot_of(c);
      const uint32_t* chunk = static_cast<const uint32_t*>(st.dev);
      if (!commit) {
        const bool words_k = planes_k && h.form;
        const uint64_t n_el = rb / 4, e_off = planes_k ? 0 : c.k == replay_ckpt::POLICY ? h.xs() : h.xs() + h.A1;
        const uint64_t n = c.cnt * n_el * (words_k ? replay_pack::CODES_PER_WORD : 1);
        const unsigned grid = (unsigned)std::min<uint64_t>((n + REPLAY_THREADS - 1) / REPLAY_THREADS, CKPT_BLOCKS);
        const int wn = planes_k && !h.form && is_packed ? pal.n : 0;   // fp32 planes on their way into a packed window
        hipLaunchKernelGGL(k_replay_ckpt_scan, dim3(grid), dim3(REPLAY_THREADS), 0, s, chunk, words_k ? 1 : 0, n_el, e_off, h.rowlen(), c.j0, c.cnt, mm,
                           fwpp, fpal.e[0], fpal.e[1], fpal.e[2], fpal.e[3], fpal.n, pal.e[0], pal.e[1], pal.e[2], pal.e[3], wn, acc);
      } else if (is_packed && !h.form) {   // fp32 rows the scan found inside the palette: the append's own pack kernel
        const unsigned gx = (unsigned)std::min<size_t>((row_words() * replay_pack::CODES_PER_WORD + REPLAY_THREADS - 1) / REPLAY_THREADS, 1024);
        hipLaunchKernelGGL(k_replay_pack, dim3(gx, (unsigned)std::min<uint64_t>(c.cnt, 65535)), dim3(REPLAY_THREADS), 0, s, chunk, words, F, mm, wpp, (int)c.cnt,
                           slot0, cap, pal.e[0], pal.e[1], pal.e[2], pal.e[3], pal.n);
      } else {                             // packed rows into an fp32 window, or into a packed window of another palette
        const size_t per_row = is_packed ? row_words() : xs;
        const unsigned gx = (unsigned)std::min<size_t>((per_row + REPLAY_THREADS - 1) / REPLAY_THREADS, 1024);
        hipLaunchKernelGGL(k_replay_ckpt_put, dim3(gx, (unsigned)std::min<uint64_t>(c.cnt, 65535)), dim3(REPLAY_THREADS), 0, s, chunk,
                           reinterpret_cast<uint32_t*>(planes), words, F, mm, fwpp, (int)c.cnt, slot0, cap, fpal.e[0], fpal.e[1], fpal.e[2], fpal.e[3], remap);
      }
      AGZ_HIP_TRY(hipGetLastError());
      return AGZ_OK;
    });
  if (r != AGZ_OK) return r;
  if (commit) {
    AGZ_HIP_TRY(hipStreamSynchronize(s));
    total = h.total;
    base = new_base;
    return AGZ_OK;
  }
  unsigned long long got[3] = {0, 0, PACK_NONE};
  AGZ_HIP_TRY(hipMemcpyAsync(got, acc, sizeof(got), hipMemcpyDeviceToHost, s));
  AGZ_HIP_TRY(hipStreamSynchronize(s));
  if (got[1]) {   // the first bad element: its value is read where it lies, in the file
    const uint64_t at = got[2];
    uint32_t word = 0;
    if (h.form) {
      const uint64_t per_row = h.row_words() * replay_pack::CODES_PER_WORD, row = at / per_row, t = at % per_row, w = t >> 4;
      const int f_ = (int)(w / fwpp), cell = (int)(w % fwpp) * replay_pack::CODES_PER_WORD + (int)(t & 15);
      const bool ok = replay_ckpt::seek_to(f, l.off[replay_ckpt::PLANES] + (row * h.row_words() + w) * 4) && fread(&word, 4, 1, f) == 1;
      const unsigned code = (word >> replay_pack::shift_of(cell)) & 3u;
      AGZ_REQUIRE(ok, AGZ_E_INVALID, "agz_replay_load: reading %s failed", path);
      AGZ_REQUIRE(cell < mm, AGZ_E_INVALID,
                  "agz_replay_load: %s: row %llu, plane %d: the word 0x%08X has a bit set past the plane's last cell (%llu bad cells in all); nothing was loaded",
                  path, (unsigned long long)row, f_, word, got[1]);
      agz::set_error("agz_replay_load: %s: row %llu, element %llu holds the code %u, the file's palette has %d entries (%llu bad cells in all); nothing was loaded",
                     path, (unsigned long long)row, (unsigned long long)((uint64_t)f_ * mm + cell), code, fpal.n, got[1]);
      return AGZ_E_INVALID;
    }
    const bool ok = replay_ckpt::seek_to(f, l.off[replay_ckpt::PLANES] + at * 4) && fread(&word, 4, 1, f) == 1;
    AGZ_REQUIRE(ok, AGZ_E_INVALID, "agz_replay_load: reading %s failed", path);
    agz::set_error("agz_replay_load: %s: row %llu, element %llu (linear element %llu) holds the bit pattern 0x%08X, which is not in the window's palette "
                   "(%llu bad cells in all); nothing was loaded",
                   path, (unsigned long long)(at / h.xs()), (unsigned long long)(at % h.xs()), (unsigned long long)at, word, got[1]);
    return AGZ_E_INVALID;
  }
  const uint64_t digest = h.live + (uint64_t)got[0];
  AGZ_REQUIRE(digest == h.digest, AGZ_E_INVALID, "agz_replay_load: %s: the rows' digest is %016llx, the header's %016llx; nothing was loaded", path,
              (unsigned long long)digest, (unsigned long long)h.digest);
  return AGZ_OK;
}

extern "C" {

int agz_replay_save(agz_replay* rp, const char* path) {
  AGZ_REQUIRE(rp && path, AGZ_E_INVALID, "agz_replay_save: NULL argument");
  replay_ckpt::Header h = rp->ckpt_header();
  int r = agz_replay_digest(rp, &h.digest);   // (joins the context's queue: every append enqueued so far is in the window)
  if (r != AGZ_OK) return r;
  const replay_ckpt::Layout l = replay_ckpt::layout(h);
  AtomicFile out(path);
  AGZ_REQUIRE(out.f, AGZ_E_INVALID, "agz_replay_save: cannot open %s", out.tmp.c_str());
  AGZ_REQUIRE(replay_ckpt::write_head(out.f, h), AGZ_E_INVALID, "agz_replay_save: write to %s failed", out.tmp.c_str());
  if ((r = rp->ckpt_write(out.f, l)) != AGZ_OK) return r;
  const AtomicFile::End end = out.commit();
  AGZ_REQUIRE(end != AtomicFile::WRITE_FAILED, AGZ_E_INVALID, "agz_replay_save: write to %s failed", out.tmp.c_str());
  AGZ_REQUIRE(end != AtomicFile::RENAME_FAILED, AGZ_E_INVALID, "agz_replay_save: cannot rename %s to %s", out.tmp.c_str(), path);
  return AGZ_OK;
}

int agz_replay_load(agz_replay* rp, const char* path) {
  AGZ_REQUIRE(rp && path, AGZ_E_INVALID, "agz_replay_load: NULL argument");
  AGZ_HIP_TRY(hipSetDevice(rp->ctx->device));
  AGZ_HIP_TRY(hipStreamSynchronize(rp->ctx->stream));
  FILE* f = fopen(path, "rb");
  AGZ_REQUIRE(f, AGZ_E_INVALID, "agz_replay_load: cannot open %s", path);
  replay_ckpt::Header h{};
  replay_ckpt::Layout l;
  std::string why;
  const replay_ckpt::Status st = replay_ckpt::read_head(f, rp->ckpt_header(), &h, &l, &why);
  int r = AGZ_OK;
  if (st != replay_ckpt::OK) {
    agz::set_error("agz_replay_load: %s %s: %s", path, st == replay_ckpt::MISMATCH ? "holds rows of another shape" : st == replay_ckpt::NOT_WINDOW ? "is not a replay window checkpoint" : "is truncated or inconsistent", why.c_str());
    r = AGZ_E_INVALID;
  }
  if (r == AGZ_OK) r = rp->ckpt_read(f, path, h, l, false);   // the whole file, validated in the staging buffer ...
  if (r == AGZ_OK) r = rp->ckpt_read(f, path, h, l, true);    // ... and only then into the ring
  fclose(f);
  return r;
}

int agz_replay_set_ckpt_staging(agz_replay* rp, size_t bytes) {
  AGZ_REQUIRE(rp, AGZ_E_INVALID, "agz_replay_set_ckpt_staging: NULL window");
  AGZ_REQUIRE(bytes >= 4 && bytes <= ((size_t)4 << 30), AGZ_E_INVALID, "agz_replay_set_ckpt_staging: %zu bytes (4 bytes .. 4 GiB)", bytes);
  rp->ckpt_staging = bytes;
  return AGZ_OK;
}

}  // extern "C"
