// One THREAD per vector: what the kernels of vq_bottleneck.hip and the backward of vq_residual.hip (4.23)
// share.  x[m] lives in DP registers, DP = the power of two >= D in {4, 8, 16, 32}, padded with zeros; the code book sits in LDS
// as [L][DP] when that is at most 8 KiB, a larger one is read from global memory at wave-uniform addresses.  Launch geometry,
// the row loads and stores, the score and the dot product of a row with a centre, and the (dtype, DP, book in LDS) dispatch.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace jpdse {

constexpr int kVqbBlocks = 1024;         // cap of the blocks (= fp32 partials) of either kernel
constexpr int kVqbChunk = 16;            // centres per LDS chunk
constexpr int kVqbCbLdsBytes = 8192;     // a padded code book up to this size is staged in LDS

// ---- launch geometry: functions of (M, D, L) alone -------------------------------------------------------------------------
static inline int vqb_dp(int D) { return D <= 4 ? 4 : (D <= 8 ? 8 : (D <= 16 ? 16 : 32)); }
static inline int vqb_bwd_threads(int D) { return D <= 8 ? 256 : (D <= 16 ? 128 : 64); }   // = vectors per tile
__host__ __device__ static inline int vqb_chunk(int L) { return L < kVqbChunk ? L : kVqbChunk; }
static inline bool vqb_cb_lds(int D, int L) { return (size_t)L * vqb_dp(D) * sizeof(float) <= (size_t)kVqbCbLdsBytes; }
static inline int vqb_blocks(int M, int V) {
  const int tiles = (M + V - 1) / V;
  return tiles < kVqbBlocks ? tiles : kVqbBlocks;
}

// ---- device helpers ---------------------------------------------------------------------------------------------------------
// c [L][D] (global) -> cb [L][DP] (LDS), components D .. DP - 1 zero; the caller synchronises
__device__ __forceinline__ void vqb_stage(const float* __restrict__ c, float* cb, int D, int L, int DP) {
  for (int i = threadIdx.x; i < L * DP; i += blockDim.x) {
    const int k = i / DP, j = i - k * DP;
    cb[i] = j < D ? c[k * D + j] : 0.f;
  }
}

// a vector's D components into DP registers (zeros beyond D); vec: 16-byte accesses (D == DP, rows and base 16-byte aligned)
template <typename T, int DP>
__device__ __forceinline__ void vqb_load_row(const T* __restrict__ p, int D, bool vec, float (&r)[DP]) {
  constexpr int N = Vec16<T>::N;
  if constexpr (DP % N == 0) {
    if (vec) {
#pragma unroll
      for (int i = 0; i < DP; i += N) {
        float t[N];
        Vec16<T>::load(p + i, t);
#pragma unroll
        for (int u = 0; u < N; ++u) r[i + u] = t[u];
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < DP; ++j) r[j] = j < D ? ElemOps<T>::ld(p + j) : 0.f;
}

template <typename T, int DP>
__device__ __forceinline__ void vqb_store_row(T* __restrict__ p, int D, bool vec, const float (&r)[DP]) {
  constexpr int N = Vec16<T>::N;
  if constexpr (DP % N == 0) {
    if (vec) {
#pragma unroll
      for (int i = 0; i < DP; i += N) {
        float t[N];
#pragma unroll
        for (int u = 0; u < N; ++u) t[u] = r[i + u];
        Vec16<T>::store(p + i, t);
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < DP; ++j)
    if (j < D) ElemOps<T>::st(p + j, r[j]);
}

// d = sum_j (x[j] - ck[j])^2, j ascending, one fused multiply-add per component: the same bits in every sweep.  PAD: ck is a
// zero-padded LDS row of DP words; otherwise a global row of D words
template <int DP, bool PAD>
__device__ __forceinline__ float vqb_score(const float (&x)[DP], const float* ck, int D) {
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < DP; ++j)
    if (PAD || j < D) {
      const float t = x[j] - ck[j];
      d = __fmaf_rn(t, t, d);
    }
  return d;
}

template <int DP, bool PAD>
__device__ __forceinline__ float vqb_dot(const float (&g)[DP], const float* ck, int D) {
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < DP; ++j)
    if (PAD || j < D) q = __fmaf_rn(g[j], ck[j], q);
  return q;
}

// f(tag of T, DP as an integral constant, CBL as an integral constant)
template <typename F>
static inline int vqb_dispatch(int dtype, int D, int L, F&& f) {
  return by_dtype(dtype, [&](auto tag) {
    auto with_dp = [&](auto dp) {
      return vqb_cb_lds(D, L) ? f(tag, dp, std::true_type{}) : f(tag, dp, std::false_type{});
    };
    switch (vqb_dp(D)) {
      case 4: return with_dp(std::integral_constant<int, 4>{});
      case 8: return with_dp(std::integral_constant<int, 8>{});
      case 16: return with_dp(std::integral_constant<int, 16>{});
      default: return with_dp(std::integral_constant<int, 32>{});
    }
  });
}

// 16-byte accesses of a row: D fills its registers, a row is a whole number of 16-byte words, every base is aligned
static inline int vqb_vec(int dtype, int D, std::initializer_list<const void*> ptrs) {
  if (D != vqb_dp(D) || (D * esize(dtype)) % 16 != 0) return 0;
  for (const void* p : ptrs)
    if (p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 != 0) return 0;
  return 1;
}

}  // namespace jpdse
