// The eight symmetries of a square board, and the position key that picks one per leaf.  ONE definition for host and device:
// engine.hip (k_select / k_leaf write the network's input through src, k_expand / k_expand_prep read the policy row through dst),
// examples.hip (the rotation and the dihedral augmenter), the host helpers of agz.h, and a plain g++ check (tests/cpp/sym_check.cpp).
//
// Two generators on a board x[i][j], m x m:
//     (R x)[i][j] = x[j][m-1-i]      the reference's RotateBoard (encoding_helper.go:80-107), one application
//     (T x)[i][j] = x[j][i]          the transpose
// S_k = R^(k&3) o T^(k>>2), k = 0..7: T first when k >= 4, then R (k&3) times.  As an index map (S_k x)[c] = x[src(m,k,c)].
// S_0..S_3 are the rotation augmenter's images in its order.  inv(k) is the index with S_inv(k) o S_k = id; dst(m,k,c) =
// src(m,inv(k),c) is where cell c of x lands in S_k x.  Plain integer selects on k: no table, and for a k that is the same in every
// lane of a wavefront no divergent branch.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGZ_SYM_HD __host__ __device__ __forceinline__
#else
#define AGZ_SYM_HD inline
#endif

namespace agz {

AGZ_SYM_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

namespace sym {

// cell of x that (S_k x)[i][j] shows
AGZ_SYM_HD int src_ij(int m, int k, int i, int j) {
  const int r = k & 3;
  const int fi = m - 1 - i, fj = m - 1 - j;
  const int a = r == 0 ? i : (r == 1 ? j : (r == 2 ? fi : fj));    // R^r: (i,j) (j,m-1-i) (m-1-i,m-1-j) (m-1-j,i)
  const int b = r == 0 ? j : (r == 1 ? fi : (r == 2 ? fj : i));
  return (k & 4) ? b * m + a : a * m + b;                           // T under it: row and column of the source exchanged
}
AGZ_SYM_HD int src(int m, int k, int c) {
  const int i = c / m;
  return src_ij(m, k, i, c - i * m);
}
// rotations invert to the opposite rotation; R^r o T is a reflection (T R T = R^-1), its own inverse
AGZ_SYM_HD int inv(int k) { return (k & 4) ? k : ((4 - k) & 3); }
AGZ_SYM_HD int dst(int m, int k, int c) { return src(m, inv(k), c); }

// The position key: sum over cells of cell_term + mover_term, uint32 arithmetic (AGZ_INF_HASH's position hash).
AGZ_SYM_HD uint32_t cell_term(int i, int v) { return mix32((uint32_t)i * 4u + (uint32_t)v + 1u); }
AGZ_SYM_HD uint32_t mover_term(int to_move) { return mix32(0xABCD0000u + (uint32_t)to_move); }
AGZ_SYM_HD uint32_t fold_seed(uint64_t seed) { return (uint32_t)seed ^ (uint32_t)(seed >> 32); }
// the leaf symmetry of a position with key ph under AGZ_SYM_RANDOM
AGZ_SYM_HD int of_key(uint32_t ph, uint32_t folded_seed) { return (int)(mix32(ph ^ folded_seed) >> 29); }

template <class B>
AGZ_SYM_HD uint32_t position_key(const B* board, int cells, int to_move) {
  uint32_t h = 0;
  for (int i = 0; i < cells; i++) h += cell_term(i, (int)board[i]);
  return h + mover_term(to_move);
}

}  // namespace sym
}  // namespace agz
