// What the code-length maps share (code_cost.hip: DESIGN.md 4.12; vq_cost.hip: 4.20): the cost table T in LDS, the sink that
// prices the decisions of a coder's model walk, the kernel that adds the per-symbol costs of a cell, and the attribution of
// the cell map to the semantic classes -- ONE statement of the class rule and of its kernel for the binarizer's code and for
// the vector quantizer's.  The limits of the label path and its argument checks are api.cpp's (cost_label_check, common.h).
#pragma once
#include "range_coder.h"

namespace jpdse {

constexpr int kCostTable = 2049;                 // T[0 .. 2048]
constexpr int kCostTableWords = 33 * 64;         // its LDS footprint: the next multiple of the wave size
constexpr int kCostClassBlocks = 128;            // blocks per image of the class kernel

static inline size_t cost_table_bytes() { return align_up(kCostTable * sizeof(uint32_t), 256); }

// T into LDS: the one cross-lane step of a cost kernel, taken by the whole wave before any lane leaves
__device__ __forceinline__ void cost_table_stage(uint32_t* cost, const uint32_t* __restrict__ table, int lane) {
  for (int i = lane; i < kCostTable; i += 64) cost[i] = table[i];
  __syncthreads();
}

// The sink that prices (range_coder.h: model walks and their sinks): a decision with the probability q of bit 0 costs T[q]
// (bit 0) or T[2048 - q] (bit 1) and adapts its word as the coder does; a symbol costs the sum over its decisions, stored at
// symbol[at * stride].  total, count: the stream's units and decisions, kept in registers.
struct CostPricer {
  const uint32_t* cost;                          // T, in LDS
  uint32_t* symbol;
  int stride;
  uint32_t sym = 0, count = 0;
  unsigned long long total = 0;

  template <typename P>
  __device__ __forceinline__ void put(P& p, uint32_t bit) {
    const uint32_t q = p;
    p = (P)adapted(q, bit);
    sym += cost[bit ? kProbOne - q : q];
    ++count;
  }
  __device__ __forceinline__ void symbol_done(long long at) {
    symbol[at * stride] = sym;
    total += sym;
    sym = 0;
  }
};

// cell[i] = the sum of the C costs of cell i < cells; 16 lanes per cell, every lane of a wave makes the same number of trips
static __global__ void __launch_bounds__(256) cost_cell_kernel(const uint32_t* __restrict__ symbol, unsigned long long* __restrict__ cell,
                                                               long long cells, int C) {
  const int sub = threadIdx.x & 15;
  const long long step = (long long)gridDim.x * 16;
  for (long long base = (long long)blockIdx.x * 16; base < cells; base += step) {
    const long long i = base + (threadIdx.x >> 4);
    unsigned long long s = 0;
    if (i < cells)
      for (int c = sub; c < C; c += 16) s += symbol[i * C + c];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
    if (sub == 0 && i < cells) cell[i] = s;
  }
}

// units / pixels: [N][n_classes + 1], zeroed by the host.  The class of a pixel is metrics.hip's rule: its label when that is
// an integer in [0, n_classes), else the extra row (NaN included).  grid (blocks, N); LDS: (n_classes + 1) x 2 x 8 bytes
static __global__ void __launch_bounds__(256) cost_class_kernel(const unsigned long long* __restrict__ cell,
                                                                const float* __restrict__ label,
                                                                unsigned long long* __restrict__ units,
                                                                unsigned long long* __restrict__ pixels, int H, int W, int h, int w,
                                                                int shift, int n_classes) {
  extern __shared__ unsigned long long hist[];   // [n_classes + 1][2] = (units, pixels)
  const int rows = n_classes + 1, n = blockIdx.y;
  for (int i = threadIdx.x; i < 2 * rows; i += 256) hist[i] = 0;
  __syncthreads();
  const long long HW = (long long)H * W;
  const float* lab_n = label + (long long)n * HW;
  const unsigned long long* cell_n = cell + (long long)n * h * w;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const float lab = lab_n[p];
    const int k = (lab >= 0.f && lab < (float)n_classes && lab == floorf(lab)) ? (int)lab : n_classes;
    atomicAdd(&hist[2 * k], cell_n[(long long)(y >> shift) * w + (x >> shift)]);
    atomicAdd(&hist[2 * k + 1], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows; i += 256) {
    if (hist[2 * i + 1] != 0) {                 // a class without a pixel in this block adds nothing
      atomicAdd(units + (long long)n * rows + i, hist[2 * i]);
      atomicAdd(pixels + (long long)n * rows + i, hist[2 * i + 1]);
    }
  }
}

// The class tables of N cell maps of h x w under label maps of H x W = (h x w) << shift: zeroes both tables, then the kernel.
// `who` names the call in an error.
static int cost_class_tables(const char* who, const unsigned long long* cell, const float* label, uint64_t* class_units,
                             uint64_t* class_pixels, int N, int H, int W, int h, int w, int shift, int n_classes, hipStream_t s) {
  const int rows = n_classes + 1;
  unsigned long long* units = reinterpret_cast<unsigned long long*>(class_units);
  unsigned long long* pixels = reinterpret_cast<unsigned long long*>(class_pixels);
  const size_t table_bytes = (size_t)N * rows * sizeof(unsigned long long);
  if (hipMemsetAsync(units, 0, table_bytes, s) != hipSuccess || hipMemsetAsync(pixels, 0, table_bytes, s) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "%s: hipMemsetAsync failed", who);
  const long long HW = (long long)H * W;
  const int blocks = (int)min((HW + 255) / 256, (long long)kCostClassBlocks);
  hipLaunchKernelGGL(cost_class_kernel, dim3(blocks, N), dim3(256), (size_t)rows * 2 * sizeof(unsigned long long), s, cell, label,
                     units, pixels, H, W, h, w, shift, n_classes);
  char what[64];
  snprintf(what, sizeof(what), "%s(class)", who);
  return check_launch(what);
}

}  // namespace jpdse
