// Where the bits of the learned codec's code go (no reference counterpart: the reference has no coded stream): the exact
// cost, symbol by symbol, that the adaptive context model of the entropy-coded bitstream assigns to a code, as a map over
// code cells, per channel, and attributed to the semantic classes of the pixels each cell covers.  Definition: DESIGN.md
// 4.12.  Entry points: include/jpdse.h, "learned codec: code-length map".
//
// The cost of a symbol coded with the probability q of bit 0 is T[q] (bit 0) or T[2048 - q] (bit 1), T[v] =
// round(-log2(v / 2048) * 2^16): an integer, in units of 2^-16 bit.  T is built once on the host in fp64
// (jpdse_code_cost_table, api.cpp) and copied into the call's workspace.  Kernels, in launch order:
//   cost_walk_kernel    entropy_encode_kernel's walk itself (code_walk, range_coder.h) with the pricing sink (CostPricer,
//                       cost_class.h) in the encoder's place: lane = channel, one wave per block, grid (ceil(C / 64), N), the
//                       lane's 16 probabilities and the bits of its previous row in LDS columns of its own, wave-uniform
//                       loops.  The sink looks a symbol's cost up (T sits in LDS, 8.2 KB, loaded by the whole wave) and
//                       stores it: the 64 lanes write 64 neighbouring channels of one cell.  The lane's running sum stays
//                       in a register and is written once, to channel[n][c].  This file holds no model loop of its own.
//   cost_cell_kernel    (cost_class.h) 16 lanes per cell add its C costs: cell[n][y][x].
//   cost_class_kernel   (cost_class.h; with a label map) a fixed grid, grid-stride over the pixels of an image: per block an LDS histogram
//                       of (n_classes + 1) x {units, pixels} filled with 64-bit LDS atomics, flushed with 64-bit global
//                       atomics into the tables the host zeroed.
// Every sum is an integer sum: no result depends on an order, two calls give identical bits.  Every loop is bounded by the
// shape; global writes are plain stores or those integer atomics.
#include "cost_class.h"
#include "range_coder.h"

namespace jpdse {

constexpr int kCostMaxW = 4096;                  // the walk's LDS row limit, as kEntropyMaxW

static bool cost_shape_ok(int N, int h, int w, int C) {
  if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || N > 65535 || w > kCostMaxW || C > 64 * 65535) return false;
  return (long long)h * w <= kCostMaxUnits / C / N;
}
static inline size_t cost_lds_bytes(int w) { return (size_t)(kCostTableWords + (16 + (w + 31) / 32) * 64) * sizeof(uint32_t); }

// symbol: uint32 [N][H][W][C] (logical channels, no padding); channel: [N][C].  H, W: the code's extents
template <typename T>
__global__ void __launch_bounds__(64) cost_walk_kernel(const T* __restrict__ b, const uint32_t* __restrict__ table,
                                                       uint32_t* __restrict__ symbol, unsigned long long* __restrict__ channel,
                                                       int H, int W, int C, int Cs) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x, c = blockIdx.x * 64 + lane, n = blockIdx.y;
  cost_table_stage(lds, table, lane);
  if (c >= C) return;                           // before the code is read or anything is written
  uint32_t* prob = lds + kCostTableWords + lane;                // [16][64]
  uint32_t* row = lds + kCostTableWords + 16 * 64 + lane;       // [nw][64]: the bits of the row above, as in entropy.hip
  const int nw = (W + 31) >> 5;
  for (int k = 0; k < 16; ++k) prob[k * 64] = kProbInit;
  for (int j = 0; j < nw; ++j) row[j * 64] = 0;
  const CostPricer pr = code_walk(b + (long long)n * H * W * Cs + c, prob, row, H, W, Cs,
                                  CostPricer{lds, symbol + (long long)n * H * W * C + c, C});
  channel[(long long)n * C + c] = pr.total;
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
  if (a->label != nullptr)
    if (int rc = cost_label_check("code_cost", a->class_units, a->class_pixels, a->H, a->W, h, w, C, a->n_classes, &shift)) return rc;
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

  return cost_class_tables("code_cost", cell, a->label, a->class_units, a->class_pixels, N, a->H, a->W, h, w, shift, a->n_classes, s);
}

}  // extern "C"
