// The per-row stage chain of the residual soft-to-hard vector quantizer, stated ONCE for the kernels that walk
// it with one THREAD per vector: vqres_rows_fwd_kernel and vqres_bwd_kernel (vq_residual.hip; 4.24, 4.23), vqrr_hist_kernel and
// vqrr_hist_general_kernel (vq_res_rate.hip; 4.26) call the pieces below; vqres_ec_kernel (vq_res_ec.hip; 4.25) is held to the same
// contract and writes the same steps itself (one of its instantiations measured slower through the helpers: 4.28).
//   r_1 = x widened to fp32 ONCE (vqb_load_row), in DP registers, zeros beyond D.
//   k_s = arg-min_k vqb_score(r_s, C_s[k]) by vqres_nearest: k ascending, the strict <, so the lowest index keeps a tie and a NaN
//       never wins (a row of NaN scores gives index 0).  The entropy-constrained kernel adds its bias to the score in a sweep of
//       the same shape (vq_res_ec.hip); without a bias it IS this sweep.
//   r_{s+1} = r_s - C_s[k_s]: ONE fp32 subtraction per component, never rounded in between (vqres_advance).  The backward forms
//       r_s from x and the stored indices by the same subtractions in the same order (its replay loop over u < s: the same chain).
//   a_s = C_1[k_1] + .. + C_s[k_s]: fp32, stage order, starting FROM the first centre (a = c, then a += c), rounded once on the
//       store: vqres_sum's additions (vq_residual.hip), so y is the group kernel's and the decoder's, bit for bit.
// Kernels that call these pieces give the same index and y for the same (x, books, n): that is the contract the files state in
// terms of each other, and tests/test_hip_vq_res*.py hold them to it.
// BARRIER RULE: a helper that holds a __syncthreads() (vqres_book) is called unconditionally by every thread of the block.  A row
// past M or past its depth is a PREDICATE after the barriers, never a loop bound: the tile loop and the stage loop run the same
// number of times in every thread, a thread without a vector works on zeros and stores nothing.
#pragma once
#include <math.h>

#include "vq_core.h"
#include "vq_rows.h"

namespace jpdse {

// thread t's vector of the tile that starts at m0: a thread past M repeats the last vector and stores nothing
struct VqResRow {
  bool live;
  int m;
  size_t row;                                      // m * D
  __device__ __forceinline__ VqResRow(int M, int D, int m0)
      : live((int)threadIdx.x < M - m0), m(live ? m0 + (int)threadIdx.x : M - 1), row((size_t)m * D) {}
};

// the tile prologue of the forward-type kernels: the vector, r = x[m] widened (zeros without a vector), a = 0
template <typename T, int DP>
__device__ __forceinline__ VqResRow vqres_row_begin(const T* __restrict__ x, int M, int D, int m0, bool vec, float (&r)[DP],
                                                    float (&a)[DP]) {
  const VqResRow w(M, D, m0);
#pragma unroll
  for (int j = 0; j < DP; ++j) r[j] = a[j] = 0.f;
  if (w.live) vqb_load_row<T, DP>(x + w.row, D, vec, r);
  return w;
}

// the book of a stage as the sweeps read it.  CBL: restaged as cb [L][DP] between two barriers (the first: the book of the stage,
// or tile, before is free) -- EVERY thread of the block calls this; otherwise the global book, read at wave-uniform addresses
template <bool CBL>
__device__ __forceinline__ const float* vqres_book(const float* __restrict__ c, float* cb, int D, int L, int DP) {
  if (!CBL) return c;
  __syncthreads();
  vqb_stage(c, cb, D, L, DP);
  __syncthreads();
  return cb;
}

// sweep 1 of a stage: the minimum score and its centre
template <int DP, bool CBL>
__device__ __forceinline__ float vqres_nearest(const float (&r)[DP], const float* cc, int ld, int D, int L, int& bk) {
  float dmin = INFINITY;
  bk = 0;
  for (int k = 0; k < L; ++k) {
    const float d = vqb_score<DP, CBL>(r, cc + k * ld, D);
    if (d < dmin) {                                // strict: the lower index keeps a tie, a NaN never wins
      dmin = d;
      bk = k;
    }
  }
  return dmin;
}

// sweep 2 of a stage's softmax: 1 / sum_k e[k], k ascending
template <int DP, bool CBL>
__device__ __forceinline__ float vqres_inv_sum(const float (&r)[DP], const float* cc, int ld, int D, int L, float dmin, float sigma) {
  float s = 0.f;
  for (int k = 0; k < L; ++k) s += vq_weight(vqb_score<DP, CBL>(r, cc + k * ld, D), dmin, sigma);
  return 1.f / s;
}

// the end of a stage: r_{s+1} = r_s - C_s[bk] and, with WY, vqres_sum's additions into a (stage order, starting FROM the first centre)
template <int DP, bool CBL, bool WY>
__device__ __forceinline__ void vqres_advance(float (&r)[DP], float (&a)[DP], const float* ck, int D, int s) {
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    const float cj = (CBL || j < D) ? ck[j] : 0.f;
    r[j] = r[j] - cj;
    if (WY) a[j] = s == 0 ? cj : a[j] + cj;
  }
}

}  // namespace jpdse
