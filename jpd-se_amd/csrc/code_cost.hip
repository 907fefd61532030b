// Where the bits of the learned codec's code go (no reference counterpart: the reference has no coded stream): the exact
// cost, symbol by symbol, that the adaptive context model of the entropy-coded bitstream assigns to a code, as a map over
// code cells, per channel, and attributed to the semantic classes of the pixels each cell covers.  Definition: DESIGN.md
// 4.12.  Entry points: include/jpdse.h, "learned codec: code-length map".
//
// The cost of a symbol coded with the probability q of bit 0 is T[q] (bit 0) or T[2048 - q] (bit 1), T[v] =
// round(-log2(v / 2048) * 2^16): an integer, in units of 2^-16 bit.  T is built once on the host in fp64
// (jpdse_code_cost_table, api.cpp) and copied into the call's workspace.  Kernels, in launch order:
//   cost_walk_kernel    the serial walk of entropy_encode_kernel (entropy.hip): lane = channel, one wave per block, grid
//                       (ceil(C / 64), N), the lane's 16 probabilities and the bits of its previous row in LDS columns of its
//                       own, wave-uniform loops.  Instead of coding the symbol the lane looks its cost up (T sits in LDS,
//                       8.2 KB, loaded by the whole wave) and stores it: the 64 lanes write 64 neighbouring channels of one
//                       cell.  The lane's running sum stays in a register and is written once, to channel[n][c].
//   cost_cell_kernel    16 lanes per cell add its C costs: cell[n][y][x].
//   cost_class_kernel   (with a label map) a fixed grid, grid-stride over the pixels of an image: per block an LDS histogram
//                       of (n_classes + 1) x {units, pixels} filled with 64-bit LDS atomics, flushed with 64-bit global
//                       atomics into the tables the host zeroed.
// Every sum is an integer sum: no result depends on an order, two calls give identical bits.  Every loop is bounded by the
// shape; global writes are plain stores or those integer atomics.
#include "range_coder.h"

namespace jpdse {

constexpr int kCostMaxW = 4096;                  // the walk's LDS row limit, as kEntropyMaxW
constexpr int kCostTable = 2049;                 // T[0 .. 2048]
constexpr int kCostTableWords = 33 * 64;         // its LDS footprint: the next multiple of the wave size
constexpr int kCostClassesMax = 256;             // what jpdse_eval_metrics_sem takes
constexpr int kCostClassBlocks = 128;            // blocks per image of the class kernel
constexpr long long kCostMaxUnits = 1LL << 40;   // symbols (and image pixels x C): every 64-bit sum stays below 2^60

static bool cost_shape_ok(int N, int h, int w, int C) {
  if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || N > 65535 || w > kCostMaxW || C > 64 * 65535) return false;
  return (long long)h * w <= kCostMaxUnits / C / N;
}
static inline size_t cost_table_bytes() { return align_up(kCostTable * sizeof(uint32_t), 256); }
static inline size_t cost_lds_bytes(int w) { return (size_t)(kCostTableWords + (16 + (w + 31) / 32) * 64) * sizeof(uint32_t); }
// log2(s) when H = s h and W = s w with s a power of two, else -1
static int cost_scale_shift(int H, int W, int h, int w) {
  for (int sh = 0; sh < 31; ++sh) {
    const long long s = 1LL << sh;
    if (s * h == H && s * w == W) return sh;
    if (s * h > H) break;
  }
  return -1;
}

// symbol: uint32 [N][H][W][C] (logical channels, no padding); channel: [N][C].  H, W: the code's extents
template <typename T>
__global__ void __launch_bounds__(64) cost_walk_kernel(const T* __restrict__ b, const uint32_t* __restrict__ table,
                                                       uint32_t* __restrict__ symbol, unsigned long long* __restrict__ channel,
                                                       int H, int W, int C, int Cs) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x, c = blockIdx.x * 64 + lane, n = blockIdx.y;
  for (int i = lane; i < kCostTable; i += 64) lds[i] = table[i];
  __syncthreads();                              // the one cross-lane step: the whole wave is still here
  if (c >= C) return;                           // before the code is read or anything is written
  const uint32_t* cost = lds;
  uint32_t* prob = lds + kCostTableWords + lane;                // [16][64]
  uint32_t* row = lds + kCostTableWords + 16 * 64 + lane;       // [nw][64]: the bits of the row above, as in entropy.hip
  const int nw = (W + 31) >> 5;
  for (int k = 0; k < 16; ++k) prob[k * 64] = kProbInit;
  for (int j = 0; j < nw; ++j) row[j * 64] = 0;
  const T* src = b + (long long)n * H * W * Cs + c;
  uint32_t* dst = symbol + (long long)n * H * W * C + c;
  unsigned long long total = 0;

  for (int y = 0; y < H; ++y) {
    uint32_t upw = row[0], left = 0, ul = 0;
    for (int j = 0; j < nw; ++j) {
      const uint32_t nextw = j + 1 < nw ? row[(j + 1) * 64] : 0u;
      const uint32_t urw = (upw >> 1) | (nextw << 31);
      const int kmax = min(32, W - 32 * j);
      const long long at = (long long)y * W + 32 * j;
      const uint32_t inw = load_bit_word(src + at * Cs, Cs, kmax);
      for (int k = 0; k < kmax; ++k) {
        const uint32_t bit = (inw >> k) & 1u, up = (upw >> k) & 1u;
        uint32_t& p = prob[context_of(left, up, ul, (urw >> k) & 1u) * 64];
        const uint32_t q = p;
        p = adapted(q, bit);
        const uint32_t units = cost[bit ? kProbOne - q : q];
        dst[(at + k) * C] = units;
        total += units;
        ul = up;
        left = bit;
      }
      row[j * 64] = inw;                        // bits beyond W stay 0
      upw = nextw;
    }
  }
  channel[(long long)n * C + c] = total;
}

// cell[i] = the sum of the C costs of cell i < cells; 16 lanes per cell, every lane of a wave makes the same number of trips
__global__ void __launch_bounds__(256) cost_cell_kernel(const uint32_t* __restrict__ symbol, unsigned long long* __restrict__ cell,
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
__global__ void __launch_bounds__(256) cost_class_kernel(const unsigned long long* __restrict__ cell, const float* __restrict__ label,
                                                         unsigned long long* __restrict__ units, unsigned long long* __restrict__ pixels,
                                                         int H, int W, int h, int w, int shift, int n_classes) {
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

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_code_cost_workspace_size(int32_t N, int32_t h, int32_t w, int32_t C, int32_t n_classes) {
  if (!cost_shape_ok(N, h, w, C) || n_classes < 0 || n_classes > kCostClassesMax) return 0;
  // the table and the per-symbol costs uint32 [N][h][w][C] (used when the caller does not want them)
  return cost_table_bytes() + (size_t)N * h * w * C * sizeof(uint32_t);
}

int jpdse_code_cost(const jpdse_code_cost_args* a) {
  JPDSE_REQUIRE(a != nullptr, "code_cost: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "code_cost: bad dtype %d", a->dtype);
  JPDSE_REQUIRE(a->b != nullptr, "code_cost: null pointer b");
  JPDSE_REQUIRE(a->cell != nullptr && a->channel != nullptr, "code_cost: null pointer cell or channel");
  const int N = a->N, h = a->h, w = a->w, C = a->C;
  JPDSE_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0, "code_cost: non-positive extent (N %d, h %d, w %d, C %d)", N, h, w, C);
  JPDSE_REQUIRE(w <= kCostMaxW, "code_cost: w %d above the walk's row limit %d", w, kCostMaxW);
  JPDSE_REQUIRE(cost_shape_ok(N, h, w, C), "code_cost: shape beyond the limits (N %d <= 65535, C %d <= %d, N * h * w * C <= 2^40)",
                N, C, 64 * 65535);
  int shift = 0;
  if (a->label != nullptr) {
    JPDSE_REQUIRE(a->class_units != nullptr && a->class_pixels != nullptr,
                  "code_cost: null pointer class_units or class_pixels with a label map");
    JPDSE_REQUIRE(a->H > 0 && a->W > 0, "code_cost: non-positive extent (H %d, W %d)", a->H, a->W);
    shift = cost_scale_shift(a->H, a->W, h, w);
    JPDSE_REQUIRE(shift >= 0, "code_cost: H %d x W %d is not the same power-of-two multiple of h %d x w %d", a->H, a->W, h, w);
    JPDSE_REQUIRE(a->n_classes >= 1 && a->n_classes <= kCostClassesMax, "code_cost: n_classes %d outside [1, %d]", a->n_classes,
                  kCostClassesMax);
    JPDSE_REQUIRE((long long)a->H * a->W <= kCostMaxUnits / C, "code_cost: H * W * C above 2^40 (H %d, W %d, C %d)", a->H, a->W, C);
  }
  const size_t need = jpdse_code_cost_workspace_size(N, h, w, C, 0);
  if (a->ws == nullptr || a->ws_bytes < need)
    return set_error(JPDSE_EWORKSPACE, "code_cost: workspace too small (%zu bytes, %zu needed)", a->ws ? a->ws_bytes : (size_t)0, need);
  JPDSE_REQUIRE(((uintptr_t)a->ws & 15) == 0, "code_cost: workspace not 16-byte aligned");

  hipStream_t s = as_stream(a->stream);
  uint32_t* table = mptr<uint32_t>(a->ws);
  uint32_t* symbol = a->symbol != nullptr ? a->symbol : reinterpret_cast<uint32_t*>(mptr<char>(a->ws) + cost_table_bytes());
  unsigned long long* cell = reinterpret_cast<unsigned long long*>(a->cell);
  unsigned long long* channel = reinterpret_cast<unsigned long long*>(a->channel);
  if (hipMemcpyAsync(table, code_cost_table_host(), kCostTable * sizeof(uint32_t), hipMemcpyHostToDevice, s) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "code_cost: hipMemcpyAsync failed");
  const int Cs = cpad(C);
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(cost_walk_kernel<T>, dim3((C + 63) / 64, N), dim3(64), cost_lds_bytes(w), s, cptr<T>(a->b), table, symbol,
                           channel, h, w, C, Cs);
        return check_launch("code_cost(walk)");
      }))
    return rc;
  const long long cells = (long long)N * h * w;
  if (int rc = launch256("code_cost(cell)", cost_cell_kernel, dim3(ew_blocks(cells, 16)), a->stream, symbol, cell, cells, C)) return rc;
  if (a->label == nullptr) return JPDSE_OK;

  const int rows = a->n_classes + 1;
  unsigned long long* units = reinterpret_cast<unsigned long long*>(a->class_units);
  unsigned long long* pixels = reinterpret_cast<unsigned long long*>(a->class_pixels);
  const size_t table_bytes = (size_t)N * rows * sizeof(unsigned long long);
  if (hipMemsetAsync(units, 0, table_bytes, s) != hipSuccess || hipMemsetAsync(pixels, 0, table_bytes, s) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "code_cost: hipMemsetAsync failed");
  const long long HW = (long long)a->H * a->W;
  const int blocks = (int)min((HW + 255) / 256, (long long)kCostClassBlocks);
  hipLaunchKernelGGL(cost_class_kernel, dim3(blocks, N), dim3(256), (size_t)rows * 2 * sizeof(unsigned long long), s, cell, a->label,
                     units, pixels, a->H, a->W, h, w, shift, a->n_classes);
  return check_launch("code_cost(class)");
}

}  // extern "C"
