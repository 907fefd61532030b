// What the soft-to-hard vector quantizer's sources share (vq.hip: DESIGN.md 4.13; vq_bottleneck.hip: 4.15, 4.16; vq_fit.hip:
// 4.21): the launcher, the softmax weight, the block-partial idiom, the group layout of a row of scores with its score loop and
// arg-min butterfly, the block-order sum of per-block partials (vq_block_sum) and the two second-stage kernels that merge them.  The kernels have
// internal linkage: each translation unit that includes this header gets its own copy, no relocatable device code is needed.
#pragma once
#include <math.h>

#include "common.h"

namespace jpdse {

// kernel<<<grid, threads, lds, stream>>>(args...) + check_launch(what); args convert to the kernel's parameter types
template <typename... P, typename... A>
static inline int vq_launch(const char* what, void (*kernel)(P...), int grid, int threads, size_t lds, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, as_stream(stream), static_cast<P>(args)...);
  return check_launch(what);
}

// more than 64 KiB of dynamic LDS needs the kernel's opt-in (host only, idempotent): vq_ec.hip, vq_residual.hip (4.23)
template <typename K>
static int vq_lds_optin(const char* who, K kernel, size_t lds) {
  if (lds <= 65536) return JPDSE_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return set_error(JPDSE_ELAUNCH, "%s: %zu bytes of LDS: %s", who, lds, hipGetErrorString(e));
  return JPDSE_OK;
}

// e = exp(-sigma (d - dmin)).  d == dmin: exp(0) = 1 without forming inf - inf when every score overflowed
__device__ __forceinline__ float vq_weight(float d, float dmin, float sigma) {
  return d == dmin ? 1.f : expf(-sigma * (d - dmin));
}

// element i of a block's own fp32 partial, by its single owner thread: written by the block's first tile, added to by the later
// ones (base and index apart: the address is formed where the open-coded statement formed it, which keeps the kernels' code)
__device__ __forceinline__ void vq_partial_put(float* mine, int i, bool first, float acc) { mine[i] = first ? acc : mine[i] + acc; }

// ---- the group layout of a row of [M][L] and its score loop: vq.hip and vq_fit.hip (4.21) assign with the
// same code, so the nearest centre is the same index for index
constexpr int kVqSlots = 8;              // centres per lane: 512 / 64

static inline int vq_group(int L) {      // lanes per row
  int g = 2;
  while (g < L && g < 64) g <<= 1;
  return g;
}

// c [L][D] (global) -> ct [D][L] (LDS); the caller synchronises
__device__ __forceinline__ void vq_stage_transposed(const float* __restrict__ c, float* ct, int D, int L) {
  for (int i = threadIdx.x; i < L * D; i += 256) {
    const int k = i / D, j = i - k * D;
    ct[j * L + k] = c[i];
  }
}

// The group layout of a row of [M][L] (the header): this lane is lane kk of group g of its wave and owns the centres
// centre(i) = kk + 64 i of the slots i with slot_live(i).  Grid-stride over rows: a wave covers the vpw vectors from `base`,
//   for (long long base = ln.first(); base < M; base += ln.stride()) { const int m = ln.vector(base, M); .. }
struct VqLanes {
  int lane, wave, kk, g, vpw, ni, L;
  __device__ __forceinline__ VqLanes(int G, int L_)
      : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), kk(lane & (G - 1)), g(lane / G), vpw(64 / G), ni((L_ + 63) >> 6), L(L_) {}
  __device__ __forceinline__ int centre(int i) const { return kk + 64 * i; }
  __device__ __forceinline__ bool slot_live(int i) const { return i < ni && kk + 64 * i < L; }
  __device__ __forceinline__ long long first() const { return (long long)(blockIdx.x * 4 + wave) * vpw; }
  __device__ __forceinline__ long long stride() const { return (long long)gridDim.x * 4 * vpw; }
  // this group's vector; an idle group (live false) repeats the last vector and stores nothing
  __device__ __forceinline__ bool live(long long base, int M) const { return base + g < M; }
  __device__ __forceinline__ int vector(long long base, int M) const { return live(base, M) ? (int)(base + g) : M - 1; }
};

// the scores of vector m against this lane's centres; slots beyond L stay 0 and are never read
template <typename T>
__device__ __forceinline__ void vq_scores(const T* __restrict__ x, const float* ct, int m, int D, const VqLanes& ln,
                                          float (&d)[kVqSlots]) {
#pragma unroll
  for (int i = 0; i < kVqSlots; ++i) d[i] = 0.f;
  const T* xr = x + (size_t)m * D;
  for (int j = 0; j < D; ++j) {
    const float xv = ElemOps<T>::ld(xr + j);
    const float* row = ct + j * ln.L;
#pragma unroll
    for (int i = 0; i < kVqSlots; ++i)
      if (ln.slot_live(i)) {
        const float t = xv - row[ln.centre(i)];
        d[i] += t * t;
      }
  }
}

// (value, index) butterfly: the smaller value wins (LESS) or the larger (!LESS), the lower index on equal values.  A NaN
// never wins a comparison, and the sentinel index of a lane without a centre is larger than any real one, so group lane 0
// ends with an index of a real centre whatever the values are.
template <bool LESS>
__device__ __forceinline__ void vq_group_arg(float& v, int& k, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int ok = __shfl_xor(k, off, 64);
    const bool better = LESS ? ov < v : ov > v;
    if (better || (ov == v && ok < k)) {
      v = ov;
      k = ok;
    }
  }
}

// sum_b partial[b][i] of nb partials of n words, b ascending, in the partials' own type (fp64 for the sums of squares of
// vq_residual.hip and vq_res_ec.hip: DESIGN.md 4.23, 4.25; int32, exact, for the latter's counts)
template <typename A>
__device__ __forceinline__ A vq_block_sum(const A* __restrict__ partial, int nb, int n, int i) {
  A acc = 0;
  for (int b = 0; b < nb; ++b) acc += partial[(size_t)b * n + i];
  return acc;
}

// out[i] = scale * sum_b partial[b][i], b ascending (fp32).  scale = 1: the bits of the sum
// (vq_block_sum's loop, kept as written: through the helper the loop's branch compiles to the other sense in every object that
// includes this header)
static __global__ __launch_bounds__(256) void vq_merge_kernel(const float* __restrict__ partial, int nb, int n, float scale,
                                                             float* __restrict__ out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) acc += partial[(size_t)b * n + i];
    out[i] = scale * acc;
  }
}

// pmf[k] = (sum_b partial[b][k]) / count, b ascending, in fp64.  One block
static __global__ __launch_bounds__(256) void vq_pmf_final_kernel(const float* __restrict__ partial, int nb, int L, double count,
                                                                 float* __restrict__ pmf) {
  for (int k = threadIdx.x; k < L; k += 256) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += (double)partial[(size_t)b * L + k];
    pmf[k] = (float)(acc / count);
  }
}

}  // namespace jpdse
