// Where the bits of the vector-quantised code go (no reference counterpart): the exact cost, symbol by symbol, that the
// adaptive model of the order-0 index coder (vq_coder.hip, .jpdv files) or of the spatial-context plane coder (vq_plane.hip,
// .jpdw files) assigns to the indices of one image, as a map over code cells, per channel group, per stream, and attributed to
// the semantic classes of the pixels each cell covers.  Definition: DESIGN.md 4.20.  Entry points: include/jpdse.h,
// "soft-to-hard vector quantizer: code-length maps of the two coders"; argument checks and the sizes: api.cpp.
//
// The cost of a decision coded with the probability q of bit 0 is T[q] (bit 0) or T[2048 - q] (bit 1), code_cost.hip's table,
// in units of 2^-16 bit; the cost of a symbol is the sum over the decisions its coder spends on it.  Kernels, in launch order:
//   vq_index_cost_kernel  the index encoder's walk itself (vq_index_walk, vq_model.h) with the pricing sink (CostPricer,
//                         cost_class.h) in the encoder's place: no model loop of its own, only the prologue, the sink and
//                         the stores.
//   vq_plane_cost_kernel  the serial walk of vq_plane_encode_kernel with the byte emission removed: the same loads of the
//                         indices, the same entries and conditions, the update range_coder.h's adapted().  It stays a copy:
//                         on the shared walk it was 1.3-1.5 % slower than this text (vq_model.h names the figures).
//                         Both: lane = stream, one wave per block, grid ceil(S / 64), the lane's table in its private LDS
//                         column (vq_col.h).  T sits in LDS behind the columns (8,448 bytes, loaded by the whole wave before
//                         any lane leaves).  A lane stores the cost of a symbol at the symbol's own position in the index
//                         tensor -- the lanes that share an interleave step or a strip write neighbouring words, as the
//                         encoders read them -- and keeps its stream's total and decision count in registers, written once.
//   cost_cell_kernel      (cost_class.h) 16 lanes per cell add its G costs.
//   vq_cost_group_kernel  a block per group adds the group's costs over all cells.
//   cost_class_kernel     (cost_class.h; with a label map) the class tables, the kernel and the rule of code_cost.hip.
// LDS: (2^nb + 66) * 128 bytes for the index walk, (10 + 2^nb + 66) * 128 for the plane walk: 73,984 and 75,264 bytes at nb = 9,
// above 64 KiB: the launch opts in (vq_plane_lds_optin); two blocks per CU still fit the 160 KiB.
// Every sum is an integer sum: no result depends on an order, two calls give identical bits.  Every loop is bounded by the
// shape; global writes are plain stores or the integer atomics of cost_class_kernel.
#include "cost_class.h"
#include "vq_col.h"
#include "vq_model.h"

namespace jpdse {

// one adaptive decision with the lane's table entry e: its cost, and the entry's update
__device__ __forceinline__ uint32_t cost_put(const uint32_t* cost, uint16_t* prob, int e, uint32_t bit) {
  const uint32_t q = prob[e * 64];
  prob[e * 64] = (uint16_t)adapted(q, bit);
  return cost[bit ? kProbOne - q : q];
}

// symbol: uint32 [M], at the positions of index; units / decisions: [S].  A lane that met an index outside [0, L) stores 2 to
// *status, which the host zeroed: every writer stores the same word.
// grid ceil(S / 64), one wave per block, (2^nb * 64 halfwords + kCostTableWords words) of dynamic LDS.
__global__ void __launch_bounds__(64) vq_index_cost_kernel(const int32_t* __restrict__ index, const uint32_t* __restrict__ table,
                                                           uint32_t* __restrict__ symbol, unsigned long long* __restrict__ units,
                                                           uint32_t* __restrict__ decisions, int32_t* __restrict__ status, int M,
                                                           int L, int S, int nb) {
  extern __shared__ uint32_t vq_cost_lds[];     // the columns [2^nb][64] of halfwords, then T
  const int lane = threadIdx.x, s = blockIdx.x * 64 + lane;
  uint32_t* cost = vq_cost_lds + (1 << nb) * 32;
  cost_table_stage(cost, table, lane);
  if (s >= S) return;                           // no cross-lane operation below
  uint16_t* prob = reinterpret_cast<uint16_t*>(vq_cost_lds) + vq_col(lane);      // entry 0 is unused
  for (int m = 1; m < (1 << nb); ++m) prob[m * 64] = (uint16_t)kProbInit;
  int bad = 0;
  const CostPricer pr = vq_index_walk(index, prob, s, M, L, S, nb, CostPricer{cost, symbol, 1}, bad);
  units[s] = pr.total;
  decisions[s] = pr.count;
  if (bad) *status = 2;
}

// The same for the index planes: stream s = k * G + g is strip k of group g; the walk of vq_plane_encode_kernel.
// grid ceil(S / 64), one wave per block, ((10 + 2^nb) * 64 halfwords + kCostTableWords words) of dynamic LDS.
__global__ void __launch_bounds__(64) vq_plane_cost_kernel(const int32_t* __restrict__ index, const uint32_t* __restrict__ table,
                                                           uint32_t* __restrict__ symbol, unsigned long long* __restrict__ units,
                                                           uint32_t* __restrict__ decisions, int32_t* __restrict__ status, int h,
                                                           int w, int G, int L, int strip_rows, int S, int nb) {
  extern __shared__ uint32_t vq_cost_lds[];     // the columns [10 + 2^nb][64] of halfwords, then T
  const int lane = threadIdx.x, s = blockIdx.x * 64 + lane;
  uint32_t* cost = vq_cost_lds + (kPlaneTree + (1 << nb)) * 32;
  cost_table_stage(cost, table, lane);
  if (s >= S) return;                           // no cross-lane operation below
  uint16_t* prob = reinterpret_cast<uint16_t*>(vq_cost_lds) + vq_col(lane);
  plane_table_init(prob, nb);
  const PlaneStream st = plane_stream(s, h, G, strip_rows);
  const long long rowstep = (long long)w * G;
  const long long first = ((long long)st.y0 * w) * G + st.g;
  const int32_t* cell = index + first;          // the cell of the step; the next one is cell + G
  uint32_t* dst = symbol + first;
  unsigned long long total = 0;
  uint32_t count = 0;
  int bad = 0, lf = 0, u = 0, ul = 0;
  // the words of the next step are loaded before the current one is priced
  int32_t next = cell[0], next_u = 0;
  for (int row = 0; row < st.rows; ++row) {
    for (int x = 0; x < w; ++x, cell += G, dst += G) {
      const int v = plane_clean(next, L, bad);
      const bool has_l = x > 0, has_u = row > 0;
      if (has_u) {
        ul = u;                                 // of the cell to the left: used with has_l only
        u = plane_clean(next_u, L, bad);
      }
      if (x + 1 < w || row + 1 < st.rows) {
        next = cell[G];
        if (row > 0 || x + 1 == w) next_u = cell[G - rowstep];
      }
      const bool has_ul = has_l && has_u;
      bool matched = false;
      uint32_t sym = 0;
      if (has_l) {
        const int e = (has_u && lf == u ? 1 : 0) | (has_ul && ul == lf ? 2 : 0) | (has_ul && ul == u ? 4 : 0);
        matched = v == lf;
        sym += cost_put(cost, prob, e, matched ? 1u : 0u);
        ++count;
      }
      if (!matched && has_u && !(has_l && u == lf)) {
        const int e = has_l ? kPlaneUp + (ul == lf ? 1 : 0) : kPlaneUpOnly;
        matched = v == u;
        sym += cost_put(cost, prob, e, matched ? 1u : 0u);
        ++count;
      }
      if (!matched) {
        uint32_t m = 1;
        for (int k = nb - 1; k >= 0; --k) {
          const uint32_t bit = ((uint32_t)v >> k) & 1u;
          sym += cost_put(cost, prob, kPlaneTree + (int)m, bit);
          m = m << 1 | bit;
        }
        count += (uint32_t)nb;
      }
      dst[0] = sym;
      total += sym;
      lf = v;
    }
  }
  units[s] = total;
  decisions[s] = count;
  if (bad) *status = 2;
}

// group[g] = the sum over the cells i < cells of symbol[i * G + g]; a block per group, grid-stride over the groups: every
// thread of a block makes the same trips
__global__ void __launch_bounds__(256) vq_cost_group_kernel(const uint32_t* __restrict__ symbol, unsigned long long* __restrict__ group,
                                                            long long cells, int G) {
  __shared__ unsigned long long part[4];
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    unsigned long long s = 0;
    for (long long i = threadIdx.x; i < cells; i += 256) s += symbol[i * G + g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) group[g] = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
  }
}

static inline size_t vq_cost_lds_bytes(int entries) { return (size_t)entries * 64 * sizeof(uint16_t) + kCostTableWords * sizeof(uint32_t); }

// what the two calls share around their walk.  The workspace: T, then the per-symbol costs when the caller does not want them
struct VqCostRun {
  const char* who;
  long long M;
  int G;
  uint32_t *table, *symbol;
  int32_t* status;
  hipStream_t s;
};

static int vq_cost_begin(VqCostRun& r, const char* who, long long M, int G, uint32_t* symbol, int32_t* status, void* ws, void* stream) {
  r = VqCostRun{who, M, G, mptr<uint32_t>(ws), symbol, status, as_stream(stream)};
  if (r.symbol == nullptr) r.symbol = reinterpret_cast<uint32_t*>(mptr<char>(ws) + cost_table_bytes());
  if (hipMemcpyAsync(r.table, code_cost_table_host(), kCostTable * sizeof(uint32_t), hipMemcpyHostToDevice, r.s) != hipSuccess ||
      hipMemsetAsync(status, 0, sizeof(int32_t), r.s) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "%s: hipMemcpyAsync / hipMemsetAsync failed", who);
  return JPDSE_OK;
}

// the reductions behind a walk; h, w: the cell grid, read with a label only
static int vq_cost_reduce(const VqCostRun& r, uint64_t* cell_out, uint64_t* group_out, const float* label, uint64_t* class_units,
                          uint64_t* class_pixels, int H, int W, int h, int w, int shift, int n_classes) {
  unsigned long long* cell = reinterpret_cast<unsigned long long*>(cell_out);
  unsigned long long* group = reinterpret_cast<unsigned long long*>(group_out);
  const long long cells = r.M / r.G;
  if (int rc = launch256(r.who, cost_cell_kernel, dim3(ew_blocks(cells, 16)), r.s, r.symbol, cell, cells, r.G)) return rc;
  if (int rc = launch256(r.who, vq_cost_group_kernel, dim3(min(r.G, 2048)), r.s, r.symbol, group, cells, r.G)) return rc;
  if (label == nullptr) return JPDSE_OK;
  return cost_class_tables(r.who, cell, label, class_units, class_pixels, 1, H, W, h, w, shift, n_classes, r.s);
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

int jpdse_vq_index_cost(const jpdse_vq_index_cost_args* a) {
  int shift = 0;
  if (int rc = vq_index_cost_check(a, &shift)) return rc;
  const int M = a->M, L = a->L, S = a->S, nb = vq_index_bits(L);
  VqCostRun r;
  if (int rc = vq_cost_begin(r, "vq_index_cost", M, a->G, a->symbol, a->status, a->ws, a->stream)) return rc;
  const size_t lds = vq_cost_lds_bytes(1 << nb);
  if (int rc = vq_plane_lds_optin("vq_index_cost", vq_index_cost_kernel, lds)) return rc;
  hipLaunchKernelGGL(vq_index_cost_kernel, dim3((S + 63) / 64), dim3(64), lds, r.s, a->index, r.table, r.symbol,
                     reinterpret_cast<unsigned long long*>(a->stream_units), a->stream_decisions, a->status, M, L, S, nb);
  if (int rc = check_launch("vq_index_cost(walk)")) return rc;
  return vq_cost_reduce(r, a->cell, a->group, a->label, a->class_units, a->class_pixels, a->H, a->W, a->h, a->w, shift, a->n_classes);
}

int jpdse_vq_plane_cost(const jpdse_vq_plane_cost_args* a) {
  int shift = 0;
  if (int rc = vq_plane_cost_check(a, &shift)) return rc;
  const int h = a->h, w = a->w, G = a->G, L = a->L, rows = a->strip_rows, nb = vq_index_bits(L);
  const int S = vq_plane_streams(h, G, rows);
  VqCostRun r;
  if (int rc = vq_cost_begin(r, "vq_plane_cost", (long long)h * w * G, G, a->symbol, a->status, a->ws, a->stream)) return rc;
  const size_t lds = vq_cost_lds_bytes(kPlaneTree + (1 << nb));
  if (int rc = vq_plane_lds_optin("vq_plane_cost", vq_plane_cost_kernel, lds)) return rc;
  hipLaunchKernelGGL(vq_plane_cost_kernel, dim3((S + 63) / 64), dim3(64), lds, r.s, a->index, r.table, r.symbol,
                     reinterpret_cast<unsigned long long*>(a->stream_units), a->stream_decisions, a->status, h, w, G, L, rows, S, nb);
  if (int rc = check_launch("vq_plane_cost(walk)")) return rc;
  return vq_cost_reduce(r, a->cell, a->group, a->label, a->class_units, a->class_pixels, a->H, a->W, h, w, shift, a->n_classes);
}

}  // extern "C"
