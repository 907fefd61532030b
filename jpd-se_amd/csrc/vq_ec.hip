// Entropy-constrained assignment of the soft-to-hard vector quantizer (ctu.quantizers.S2HVQ.encode_ec).
// Entry points: include/jpdse.h, "entropy-constrained assignment"; contract, the LDS decision and measurements: DESIGN.md 4.22.
//   x [M][D] (fp32 or bf16), the code book c fp32 [L][D], G groups, vector m in group m % G, bias fp32 [G][L] or NULL.
//   cost[m][k] = d[m][k] + bias[m % G][k], d the direct score of vq.hip (vq_scores, unchanged), the bias one fp32 add after the
//   loop; index[m] = the arg-min, lowest index on equal cost (vq_group_arg<true>).  A lane without a centre starts at (+inf, a
//   sentinel index above every real one) and a centre whose bias is +inf costs +inf: both lose to any finite cost, and among
//   equal +inf the lowest REAL index wins, so the result is always a centre.
// Kernels:
//   vqe_assign_kernel   a block walks tiles of 256 vectors.  Assignment: the group layout of vq_hard_fwd_kernel, x read from
//       global memory once.  The lane that owns the winner leaves (index, d without the bias) of the tile in LDS.  Histogram:
//       every cell (g, k) has ONE OWNER THREAD (cell % 256) that scans the tile's vectors of group g in ascending order and adds
//       its count to the block's table: L compare steps per thread and tile whatever G is, against D L / 64 LDS reads per
//       vector of the score loop.  Distortion: G a power of two <= 64 -- thread t holds vector t of the tile, the lanes that share
//       lane % G are added across the wave in fp64 with xor-shuffles (offsets 32, 16, .. G: vqr_hist_kernel's sums), the four
//       waves in order, into a register of thread g; any other G -- thread g sums its vectors ascending into the block's fp64
//       partial.  TL: the block's [G][L] table and the bias sit in LDS; otherwise (large G L) the table IS the block's partial
//       in the workspace and the bias is read through L2, loaded before the score loop that hides its latency.
//   vqe_merge_kernel    hist = the sum of the blocks' tables (int32, exact), sse = the blocks' fp64 partials in block order.
//   vqe_lengths_kernel  one block per group: n = the row sum, bias = lambda (log2 n - log2 hist) (+inf on an empty bin, exact 0
//       everywhere at lambda == 0), bits = sum hist (log2 n - log2 hist), fp64, k = t, t + 256 per thread, threads in order.
// No atomics; grid, tiles and owners are functions of (M, D, L, G) alone: two calls give identical bits.
#include <math.h>

#include "common.h"
#include "vq_core.h"

namespace jpdse {

constexpr int kVqEcTile = 256;               // vectors per tile
constexpr int kVqEcBlocks = 2048;            // cap of the blocks (= partial tables) of vqe_assign_kernel
constexpr int kVqEcPartialWords = 1 << 22;   // cap of blocks * G * L: tables of at most 16 MiB
constexpr size_t kVqEcLdsBudget = 80 * 1024; // two blocks per CU (160 KiB)

// ---- launch geometry: functions of (M, D, L, G) alone ---------------------------------------------------------------------------
static inline int vqe_blocks(int M, int L, int G) {
  const int tiles = (M + kVqEcTile - 1) / kVqEcTile;
  int cap = kVqEcPartialWords / (G * L);
  cap = cap < 1 ? 1 : (cap > kVqEcBlocks ? kVqEcBlocks : cap);
  return tiles < cap ? tiles : cap;
}
// LDS: red fp64 [4][64] | ct [D][L] | it [256] | dt [256] | with TL: tab int32 [G][L] | bl fp32 [G][L]
static inline size_t vqe_fixed_lds(int D, int L) { return 4 * 64 * sizeof(double) + ((size_t)D * L + 2 * kVqEcTile) * sizeof(float); }
static inline bool vqe_tables_lds(int D, int L, int G) { return vqe_fixed_lds(D, L) + 2 * (size_t)G * L * sizeof(float) <= kVqEcLdsBudget; }
static inline bool vqe_sse_shuffle(int G) { return G <= 64 && (G & (G - 1)) == 0; }
// the workspace: sse fp64 [blocks][G] | hist int32 [blocks][G][L]
static inline size_t vqe_ws_hist(int M, int L, int G) { return (size_t)vqe_blocks(M, L, G) * G * sizeof(double); }
static inline size_t vqe_ws_bytes(int M, int L, int G) { return vqe_ws_hist(M, L, G) + (size_t)vqe_blocks(M, L, G) * G * L * sizeof(int); }

// ---- kernels ------------------------------------------------------------------------------------------------------------------
template <typename T, bool TL>
__global__ __launch_bounds__(256) void vqe_assign_kernel(const T* __restrict__ x, const float* __restrict__ c,
                                                        const float* __restrict__ bias, int M, int D, int L, int G, int GL,
                                                        int shuffle, int* __restrict__ index, int* __restrict__ phist,
                                                        double* __restrict__ psse) {
  extern __shared__ double vqe_lds[];
  constexpr int V = kVqEcTile;
  double* red = vqe_lds;
  float* ct = reinterpret_cast<float*>(red + 4 * 64);
  int* it = reinterpret_cast<int*>(ct + D * L);
  float* dt = reinterpret_cast<float*>(it + V);
  int* tab = it + 2 * V;
  float* bl = reinterpret_cast<float*>(tab + G * L);
  const int E = G * L, t = threadIdx.x;
  const bool stats = phist != nullptr || psse != nullptr;
  int* mine = phist != nullptr ? phist + (size_t)blockIdx.x * E : nullptr;
  double* msse = psse != nullptr ? psse + (size_t)blockIdx.x * G : nullptr;
  int* cells = TL ? tab : mine;
  vq_stage_transposed(c, ct, D, L);
  if (mine != nullptr)
    for (int i = t; i < E; i += 256) cells[i] = 0;
  if (TL && bias != nullptr)
    for (int i = t; i < E; i += 256) bl[i] = bias[i];
  __syncthreads();
  const VqLanes ln(GL, L);
  const int lane = ln.lane, wave = ln.wave, kk = ln.kk;
  double sacc = 0.0;                           // shuffle: the running sum of group t (t < G)
  bool first = true;
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    for (int vb = wave * ln.vpw; vb < nv; vb += 4 * ln.vpw) {
      const bool live = vb + ln.g < nv;
      const int v = live ? vb + ln.g : nv - 1;
      const int m = m0 + v;
      float b[kVqSlots];
#pragma unroll
      for (int i = 0; i < kVqSlots; ++i) b[i] = 0.f;
      if (bias != nullptr) {                   // before the score loop, which hides the latency of a row read through L2
        const int row = (m % G) * L;
#pragma unroll
        for (int i = 0; i < kVqSlots; ++i)
          if (ln.slot_live(i)) b[i] = TL ? bl[row + ln.centre(i)] : bias[row + ln.centre(i)];
      }
      float d[kVqSlots];
      vq_scores(x, ct, m, D, ln, d);
      float best = INFINITY;
      int bk = kk < L ? kk : 0x7fffffff;
      if (kk < L) best = bias != nullptr ? d[0] + b[0] : d[0];
#pragma unroll
      for (int i = 1; i < kVqSlots; ++i)
        if (ln.slot_live(i)) {
          const float cost = bias != nullptr ? d[i] + b[i] : d[i];
          if (cost < best) {                   // strict: the lower index keeps a tie, and +inf never replaces anything
            best = cost;
            bk = ln.centre(i);
          }
        }
      vq_group_arg<true>(best, bk, GL);
      bk = __shfl(bk, lane & ~(GL - 1), 64);   // group lane 0 decides for the row
      bk = bk < L ? bk : L - 1;
      if (live) {
        if (kk == 0) index[m] = bk;
        if (stats && (bk & 63) == kk) {        // the lane that owns the winner: its score without the bias
          float dsel = d[0];
#pragma unroll
          for (int i = 1; i < kVqSlots; ++i)
            if ((bk >> 6) == i) dsel = d[i];
          it[v] = bk;
          dt[v] = dsel;
        }
      }
    }
    if (!stats) continue;
    __syncthreads();
    const int r0 = m0 % G;                     // slot j of the tile holds the vectors j, j + G, ..: group (r0 + j) % G
    if (mine != nullptr) {
      for (int cell = t; cell < E; cell += 256) {
        const int g = cell / L, k = cell - g * L;
        int cnt = 0;
        for (int v = g >= r0 ? g - r0 : g - r0 + G; v < nv; v += G) cnt += it[v] == k ? 1 : 0;
        if (cnt != 0) cells[cell] += cnt;
      }
    }
    if (msse != nullptr) {
      if (shuffle) {                           // V % G == 0: r0 == 0 and the group of vector t is lane % G
        double s = t < nv ? (double)dt[t] : 0.0;
        for (int off = 32; off >= G; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane < G) red[wave * 64 + lane] = s;
      } else {
        for (int g = t; g < G; g += 256) {
          double s = 0.0;
          for (int v = g >= r0 ? g - r0 : g - r0 + G; v < nv; v += G) s += (double)dt[v];
          msse[g] = first ? s : msse[g] + s;
        }
      }
    }
    __syncthreads();                           // it / dt are free again; red is complete
    if (msse != nullptr && shuffle && t < G) sacc += ((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t];
    first = false;
  }
  if (msse != nullptr && shuffle && t < G) msse[t] = sacc;
  if (TL && mine != nullptr) {
    __syncthreads();
    for (int i = t; i < E; i += 256) mine[i] = tab[i];
  }
}

__global__ __launch_bounds__(256) void vqe_merge_kernel(const int* __restrict__ phist, const double* __restrict__ psse, int nb, int E,
                                                       int G, int* __restrict__ hist, double* __restrict__ sse) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < E + G; i += gridDim.x * 256) {
    if (i < E) {
      if (hist == nullptr) continue;
      int acc = 0;
      for (int b = 0; b < nb; ++b) acc += phist[(size_t)b * E + i];
      hist[i] = acc;
    } else {
      if (sse == nullptr) continue;
      const int g = i - E;
      double acc = 0.0;
      for (int b = 0; b < nb; ++b) acc += psse[(size_t)b * G + g];
      sse[g] = acc;
    }
  }
}

__global__ __launch_bounds__(256) void vqe_lengths_kernel(const int* __restrict__ hist, int L, double lambda, float* __restrict__ bias,
                                                         double* __restrict__ bits) {
  __shared__ long long cnt[256];
  __shared__ double red[256];
  __shared__ double lgn;
  const int g = blockIdx.x, t = threadIdx.x;
  const int* row = hist + (size_t)g * L;
  long long n = 0;
  for (int k = t; k < L; k += 256) n += row[k] > 0 ? row[k] : 0;
  cnt[t] = n;
  __syncthreads();
  if (t == 0) {
    long long tot = 0;
    for (int u = 0; u < 256; ++u) tot += cnt[u];
    lgn = tot > 0 ? log2((double)tot) : 0.0;
  }
  __syncthreads();
  double acc = 0.0;
  for (int k = t; k < L; k += 256) {
    const int h = row[k];
    float b = lambda == 0.0 ? 0.f : INFINITY;
    if (h > 0) {
      const double len = lgn - log2((double)h);
      acc += (double)h * len;
      if (lambda != 0.0) b = (float)(lambda * len);
    }
    if (bias != nullptr) bias[(size_t)g * L + k] = b;
  }
  red[t] = acc;
  __syncthreads();
  if (t == 0 && bits != nullptr) {
    double tot = 0.0;
    for (int u = 0; u < 256; ++u) tot += red[u];
    bits[g] = tot;
  }
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_ec_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G) {
  if (vq_shape_check("vq_ec_workspace_size", M, D, L) != JPDSE_OK) return 0;
  if (vqr_group_check("vq_ec_workspace_size", M, L, G) != JPDSE_OK) return 0;
  return vqe_ws_bytes(M, L, G);
}

int jpdse_vq_ec_assign(const jpdse_vq_ec_assign_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_ec_assign: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_ec_assign: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_ec_assign", a->M, a->D, a->L)) return rc;
  if (int rc = vqr_group_check("vq_ec_assign", a->M, a->L, a->G)) return rc;
  JPDSE_REQUIRE(a->x && a->code_book && a->index, "vq_ec_assign: null pointer");
  const int M = a->M, D = a->D, L = a->L, G = a->G;
  const bool stats = a->hist != nullptr || a->sse != nullptr;
  if (stats) {
    if (int rc = vq_ws_check("vq_ec_assign", a->ws, a->ws_bytes, vqe_ws_bytes(M, L, G))) return rc;
    JPDSE_REQUIRE(reinterpret_cast<uintptr_t>(a->ws) % 8 == 0, "vq_ec_assign: workspace not 8-byte aligned");
  }
  const int nb = vqe_blocks(M, L, G);
  double* psse = a->sse != nullptr ? mptr<double>(a->ws) : nullptr;
  int* phist = a->hist != nullptr ? reinterpret_cast<int*>(static_cast<char*>(a->ws) + vqe_ws_hist(M, L, G)) : nullptr;
  const bool tl = vqe_tables_lds(D, L, G);
  const size_t lds = vqe_fixed_lds(D, L) + (tl ? 2 * (size_t)G * L * sizeof(float) : 0);
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        auto go = [&](auto kernel) {
          if (int rc = vq_lds_optin("vq_ec_assign", kernel, lds)) return rc;
          return vq_launch("vq_ec_assign", kernel, nb, 256, lds, a->stream, cptr<T>(a->x), a->code_book, a->bias, M, D, L, G,
                           vq_group(L), vqe_sse_shuffle(G) ? 1 : 0, a->index, phist, psse);
        };
        return tl ? go(vqe_assign_kernel<T, true>) : go(vqe_assign_kernel<T, false>);
      }))
    return rc;
  if (!stats) return JPDSE_OK;
  return vq_launch("vq_ec_assign(merge)", vqe_merge_kernel, ew_blocks(G * L + G), 256, 0, a->stream, phist, psse, nb, G * L, G,
                   a->hist, a->sse);
}

int jpdse_vq_ec_lengths(const jpdse_vq_ec_lengths_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_ec_lengths: null argument struct");
  JPDSE_REQUIRE(a->L >= 2 && a->L <= 512, "vq_ec_lengths: n_center L = %d (2 .. 512)", a->L);
  JPDSE_REQUIRE(a->G >= 1 && (long long)a->G * a->L <= 65536, "vq_ec_lengths: G = %d groups (at least 1, G * L at most 65536)", a->G);
  JPDSE_REQUIRE(isfinite(a->lambda) && a->lambda >= 0.0, "vq_ec_lengths: lambda is %g (a finite value >= 0)", a->lambda);
  JPDSE_REQUIRE(a->hist && (a->bias || a->bits), "vq_ec_lengths: null pointer");
  return vq_launch("vq_ec_lengths", vqe_lengths_kernel, a->G, 256, 0, a->stream, a->hist, a->L, a->lambda, a->bias, a->bits);
}

}  // extern "C"
