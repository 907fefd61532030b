// What the soft-to-hard vector quantizer's sources share (vq.hip: DESIGN.md 4.13; vq_bottleneck.hip: 4.15, 4.16): the launcher,
// the softmax weight, the block-partial idiom and the two second-stage kernels that merge per-block partials.  The kernels have
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

// e = exp(-sigma (d - dmin)).  d == dmin: exp(0) = 1 without forming inf - inf when every score overflowed
__device__ __forceinline__ float vq_weight(float d, float dmin, float sigma) {
  return d == dmin ? 1.f : expf(-sigma * (d - dmin));
}

// element i of a block's own fp32 partial, by its single owner thread: written by the block's first tile, added to by the later
// ones (base and index apart: the address is formed where the open-coded statement formed it, which keeps the kernels' code)
__device__ __forceinline__ void vq_partial_put(float* mine, int i, bool first, float acc) { mine[i] = first ? acc : mine[i] + acc; }

// out[i] = scale * sum_b partial[b][i], b ascending (fp32).  scale = 1: the bits of the sum
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
