// Entropy-constrained code of the residual soft-to-hard vector quantizer (ctu.quantizers.ResidualS2HVQ.encode_ec).
// Entry points: include/jpdse.h, "residual vector quantizer"; contract, the LDS rule, resources and measurements: DESIGN.md 4.25.
//   x [M][D] (fp32 or bf16), S code books fp32 [S][L][D], n <= S stages in use, G groups, vector m in group m % G, bias fp32
//   [n][G][L] or NULL.  The chain of vq_res_rows.h with cost_s[k] = d(r_s, C_s[k]) + bias[s][m % G][k] in the place of the
//   score d, the bias one fp32 add after the score loop: k_s = the arg-min of the cost by the same strict <, so a +inf cost
//   never replaces anything and a row of +inf alone gives index 0.  hist int32 [n][G][L]: the counts of k_s; sse fp64 [n][G]:
//   the sum of the chosen d WITHOUT the bias, each widened to fp64.
// Kernels:
//   vqres_ec_kernel      vqres_rows_fwd_kernel's layout: one THREAD per vector, r (and with WY the running sum a) in DP
//       registers, the stage loop inside the thread, book s restaged as [L][DP] in LDS when CBL, otherwise read through L2 at
//       wave-uniform addresses.  Bias: the stage's [G][L] slice is restaged with the book, TRANSPOSED as bl [L][G] (the lanes
//       of a wave hold consecutive groups: consecutive words, no bank conflict), when it fits the budget below; otherwise each
//       lane reads its row through L2, loaded before the score that hides its latency.  Statistics: after a stage's arg-min
//       every thread leaves (k, d) of its vector in LDS; past a barrier every cell (g, k) of the stage has ONE OWNER THREAD
//       (cell % 256) that scans the tile's vectors of group g in ascending order and adds its count to the block's table
//       [n][G][L] (LDS when it fits, otherwise the block's workspace slice); the fp64 sums of d: G a power of two <= 64 --
//       xor-shuffles over the lanes that share lane % G (offsets 32 .. G), the four waves in order; any other G -- thread g
//       sums its vectors ascending.  Either way thread g adds the tile's sum to the block's fp64 partial [n][G].
//   vqres_ec_merge_kernel   hist = the sum of the blocks' tables (int32, exact), sse = the blocks' partials in block order
//       (vq_block_sum, vq_core.h).
// A thread beyond M works on zeros, stores nothing, is outside every scan and reaches every barrier.  No atomics; grid, tiles,
// owners and the LDS layout are functions of (M, D, L, G, n) alone: two calls give identical bits.
#include <math.h>

#include "common.h"
#include "vq_core.h"
#include "vq_rows.h"

namespace jpdse {

constexpr int kVqResEcTile = 256;                 // vectors per tile = threads per block
constexpr int kVqResEcPartialWords = 1 << 22;     // cap of blocks * n * G * L: tables of at most 16 MiB
constexpr size_t kVqResEcLdsBudget = 48 * 1024;   // three blocks per CU (160 KiB): what 3 waves per SIMD at DP 32 can use

// ---- launch geometry and LDS layout: functions of (M, D, L, G, n) alone -------------------------------------------------------
static inline int vqres_ec_blocks(int M, int L, int G, int n) {
  const int tiles = (M + kVqResEcTile - 1) / kVqResEcTile;
  int cap = kVqResEcPartialWords / (n * G * L);
  cap = cap < 1 ? 1 : (cap > kVqbBlocks ? kVqbBlocks : cap);
  return tiles < cap ? tiles : cap;
}
// LDS: red fp64 [4][64] | it int32 [256] | dt fp32 [256] | cb fp32 [L][DP] when staged | bl fp32 [L][G] | tab int32 [n][G][L]
static inline size_t vqres_ec_fixed_lds(int D, int L) {
  return 4 * 64 * sizeof(double) + 2 * kVqResEcTile * sizeof(float) + (vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) * sizeof(float) : 0);
}
static inline bool vqres_ec_bias_lds(int D, int L, int G) {
  return vqres_ec_fixed_lds(D, L) + (size_t)G * L * sizeof(float) <= kVqResEcLdsBudget;
}
static inline bool vqres_ec_table_lds(int D, int L, int G, int n) {
  return vqres_ec_bias_lds(D, L, G) &&
         vqres_ec_fixed_lds(D, L) + (size_t)(n + 1) * G * L * sizeof(float) <= kVqResEcLdsBudget;
}
static inline size_t vqres_ec_lds(int D, int L, int G, int n, bool stats) {
  size_t b = vqres_ec_fixed_lds(D, L);
  if (vqres_ec_bias_lds(D, L, G)) b += (size_t)G * L * sizeof(float);
  if (stats && vqres_ec_table_lds(D, L, G, n)) b += (size_t)n * G * L * sizeof(int);
  return b;
}
static inline bool vqres_ec_shuffle(int G) { return G <= 64 && (G & (G - 1)) == 0; }
// the workspace: sse fp64 [blocks][n][G] | hist int32 [blocks][n][G][L]
static inline size_t vqres_ec_ws_hist(int M, int L, int G, int n) { return (size_t)vqres_ec_blocks(M, L, G, n) * n * G * sizeof(double); }
static inline size_t vqres_ec_ws_bytes(int M, int L, int G, int n) {
  return vqres_ec_ws_hist(M, L, G, n) + (size_t)vqres_ec_blocks(M, L, G, n) * n * G * L * sizeof(int);
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------
// bmode: 0 no bias, 1 the stage's slice in LDS, 2 through L2.  tl: the block's table in LDS.  phist / psse: the blocks' partials
// (both or neither).  y is read only with WY.
template <typename T, int DP, bool CBL, bool WY>
__global__ __launch_bounds__(256) void vqres_ec_kernel(const T* __restrict__ x, const float* __restrict__ books,
                                                      const float* __restrict__ bias, int M, int D, int L, int G, int n, int vec,
                                                      int bmode, int bl_words, int tl, int shuffle, T* __restrict__ y,
                                                      int* __restrict__ index, int* __restrict__ phist, double* __restrict__ psse) {
  extern __shared__ double vqres_ec_lds_mem[];
  constexpr int V = kVqResEcTile;
  double* red = vqres_ec_lds_mem;
  int* it = reinterpret_cast<int*>(red + 4 * 64);
  float* dt = reinterpret_cast<float*>(it + V);
  float* cb = dt + V;
  float* bl = cb + (CBL ? L * DP : 0);
  int* tab = reinterpret_cast<int*>(bl + bl_words);
  const int ld = CBL ? DP : D;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, LD = L * D, E = G * L;
  const bool stats = phist != nullptr;
  int* mine = stats ? phist + (size_t)blockIdx.x * n * E : nullptr;
  double* msse = stats ? psse + (size_t)blockIdx.x * n * G : nullptr;
  int* cells = tl ? tab : mine;
  if (stats) {
    for (int i = t; i < n * E; i += 256) cells[i] = 0;
    for (int i = t; i < n * G; i += 256) msse[i] = 0.0;   // its owner adds to it only past a barrier
  }
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    // vqres_row_begin's prologue and, below, vqres_advance's step and vqres_nearest's sweep with the bias, as this kernel wrote
    // them before vq_res_rows.h: with the two helpers <float, 32, false, true> measured 0.9 % slower
    const bool live = t < nv;
    const int m = live ? m0 + t : M - 1;
    const int g = m % G;
    const int r0 = m0 % G;                       // slot j of the tile holds the vectors j, j + G, ..: group (r0 + j) % G
    const size_t row = (size_t)m * D;
    float r[DP], a[DP];                          // a: dead code without WY
#pragma unroll
    for (int j = 0; j < DP; ++j) r[j] = a[j] = 0.f;
    if (live) vqb_load_row<T, DP>(x + row, D, vec != 0, r);
    for (int s = 0; s < n; ++s) {
      const float* c = books + (size_t)s * LD;
      const float* bs = bmode != 0 ? bias + (size_t)s * E : nullptr;
      if (CBL || bmode == 1) {
        __syncthreads();                         // the book and the bias slice of the stage (or tile) before are free
        if (CBL) vqb_stage(c, cb, D, L, DP);
        if (bmode == 1)
          for (int i = t; i < E; i += 256) {
            const int gg = i / L, k = i - gg * L;
            bl[k * G + gg] = bs[i];
          }
        __syncthreads();
      }
      const float* cc = CBL ? cb : c;
      const float* bg = bmode != 0 ? bs + (size_t)g * L : nullptr;
      // vqres_nearest's sweep (vq_res_rows.h) with the bias added to the score: the same order, the same strict <
      float best = INFINITY, dsel = vqb_score<DP, CBL>(r, cc, D);   // centre 0 stays when nothing is below +inf
      int bk = 0;
      for (int k = 0; k < L; ++k) {
        float b = 0.f;
        if (bmode == 1) b = bl[k * G + g];
        if (bmode == 2) b = bg[k];
        const float d = vqb_score<DP, CBL>(r, cc + k * ld, D);
        const float cost = bmode != 0 ? d + b : d;
        if (cost < best) {                       // strict: the lower index keeps a tie, +inf and NaN never replace anything
          best = cost;
          dsel = d;
          bk = k;
        }
      }
      const float* ck = cc + bk * ld;            // vqres_advance's step, as written before it (see the tile prologue above)
#pragma unroll
      for (int j = 0; j < DP; ++j) {
        const float cj = (CBL || j < D) ? ck[j] : 0.f;
        r[j] = r[j] - cj;
        if constexpr (WY) a[j] = s == 0 ? cj : a[j] + cj;
      }
      if (live) index[(size_t)s * M + m] = bk;
      if (!stats) continue;
      if (live) {
        it[t] = bk;
        dt[t] = dsel;
      }
      __syncthreads();
      for (int cell = t; cell < E; cell += 256) {
        const int gg = cell / L, k = cell - gg * L;
        int cnt = 0;
        for (int v = gg >= r0 ? gg - r0 : gg - r0 + G; v < nv; v += G) cnt += it[v] == k ? 1 : 0;
        if (cnt != 0) cells[(size_t)s * E + cell] += cnt;
      }
      if (shuffle) {                             // V % G == 0: r0 == 0 and the group of vector t is lane % G
        double acc = live ? (double)dt[t] : 0.0;
        for (int off = 32; off >= G; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane < G) red[wave * 64 + lane] = acc;
      } else {
        for (int gg = t; gg < G; gg += 256) {
          double acc = 0.0;
          for (int v = gg >= r0 ? gg - r0 : gg - r0 + G; v < nv; v += G) acc += (double)dt[v];
          msse[(size_t)s * G + gg] += acc;
        }
      }
      __syncthreads();                           // it / dt are free again; red is complete
      if (shuffle && t < G) msse[(size_t)s * G + t] += ((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t];
    }
    if constexpr (WY)
      if (live) vqb_store_row<T, DP>(y + row, D, vec != 0, a);
  }
  if (stats && tl) {
    __syncthreads();
    for (int i = t; i < n * E; i += 256) mine[i] = tab[i];
  }
}

// cells = n * G * L, sums = n * G
__global__ __launch_bounds__(256) void vqres_ec_merge_kernel(const int* __restrict__ phist, const double* __restrict__ psse, int nb,
                                                            int cells, int sums, int* __restrict__ hist, double* __restrict__ sse) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < cells + sums; i += gridDim.x * 256) {
    if (i < cells)
      hist[i] = vq_block_sum(phist, nb, cells, i);
    else
      sse[i - cells] = vq_block_sum(psse, nb, sums, i - cells);
  }
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_res_ec_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G, int32_t n) {
  if (vq_res_grouped_check("vq_res_ec_workspace_size", JPDSE_F32, M, D, L, JPDSE_VQ_RES_MAX_STAGES, n, G) != JPDSE_OK) return 0;
  return vqres_ec_ws_bytes(M, L, G, n);
}

int jpdse_vq_res_ec_assign(const jpdse_vq_res_ec_assign_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_ec_assign: null argument struct");
  if (int rc = vq_res_grouped_check("vq_res_ec_assign", a->dtype, a->M, a->D, a->L, a->S, a->n_stages, a->G)) return rc;
  JPDSE_REQUIRE(a->x && a->books && a->index, "vq_res_ec_assign: null pointer (x, books, index)");
  JPDSE_REQUIRE((a->hist == nullptr) == (a->sse == nullptr), "vq_res_ec_assign: hist and sse come together or not at all");
  const int M = a->M, D = a->D, L = a->L, G = a->G, n = a->n_stages;
  const bool stats = a->hist != nullptr;
  if (stats) {
    if (int rc = vq_ws_check("vq_res_ec_assign", a->ws, a->ws_bytes, vqres_ec_ws_bytes(M, L, G, n))) return rc;
    JPDSE_REQUIRE(reinterpret_cast<uintptr_t>(a->ws) % 8 == 0, "vq_res_ec_assign: workspace not 8-byte aligned");
  }
  const int nb = vqres_ec_blocks(M, L, G, n);
  double* psse = stats ? mptr<double>(a->ws) : nullptr;
  int* phist = stats ? reinterpret_cast<int*>(static_cast<char*>(a->ws) + vqres_ec_ws_hist(M, L, G, n)) : nullptr;
  const bool bl = vqres_ec_bias_lds(D, L, G), tl = stats && vqres_ec_table_lds(D, L, G, n);
  const int bmode = a->bias == nullptr ? 0 : (bl ? 1 : 2);
  const size_t lds = vqres_ec_lds(D, L, G, n, stats);
  const int vec = vqb_vec(a->dtype, D, {a->x, a->y});
  if (int rc = vqb_dispatch(a->dtype, D, L, [&](auto tag, auto dp, auto cbl) {
        using T = decltype(tag);
        constexpr int DP = decltype(dp)::value;
        constexpr bool CBL = decltype(cbl)::value;
        auto go = [&](auto kernel) {
          return vq_launch("vq_res_ec_assign", kernel, nb, 256, lds, a->stream, cptr<T>(a->x), a->books, a->bias, M, D, L, G, n, vec,
                           bmode, bl ? G * L : 0, tl ? 1 : 0, vqres_ec_shuffle(G) ? 1 : 0, mptr<T>(a->y), a->index, phist, psse);
        };
        return a->y != nullptr ? go(vqres_ec_kernel<T, DP, CBL, true>) : go(vqres_ec_kernel<T, DP, CBL, false>);
      }))
    return rc;
  if (!stats) return JPDSE_OK;
  return vq_launch("vq_res_ec_assign(merge)", vqres_ec_merge_kernel, ew_blocks(n * G * L + n * G), 256, 0, a->stream, phist, psse, nb,
                   n * G * L, n * G, a->hist, a->sse);
}

}  // extern "C"
