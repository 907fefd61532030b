// Rate term of the residual soft-to-hard vector quantizer (ctu.quantizers.ResidualS2HVQ.rate): the entropy of the per-group
// histograms of every stage's soft assignment, value and gradient w.r.t. the histograms.
// Entry points: include/jpdse.h, "residual vector quantizer: the rate term"; definition, path selection, resources and
// measurements: DESIGN.md 4.26.
//   x [M][D] (fp32 or bf16), S code books fp32 [S][L][D], n <= S stages in use, G groups, vector m in group m % G.  The chain and
//   its barrier rule: vq_res_rows.h.  p_s[m][k] = e * (1 / sum) with e = vq_weight(score, minimum, sigma), as vqr_hist_kernel
//   (vq_bottleneck.hip) forms it for one stage; hist[s][g][k] = the sum of p_s over the vectors of group g.
// Kernels (the chain's pieces per stage, with the histogram of p between the sweeps and the step):
//   vqrr_hist_kernel          G a power of two <= 64 whose tables fit (vqrr_waves): per stage, sweep 1 the minimum and the arg-min,
//       sweep 2 the row sum, sweep 3 p: the lanes of a group (lane % G) are added across the wave with xor-shuffles, offsets 32,
//       16, .. G, and lane g < G adds the sum into the wave's own table [n][G][L + 1] (the odd stride: the G owners on different
//       banks), tile after tile; the waves are merged in wave order at the end into the block's fp32 partial [n][G][L].
//   vqrr_hist_general_kernel  any other G, or tables that do not fit: sweep 3 goes through LDS in chunks of KC centres ([KC][257]);
//       thread (slot j < min(G, vectors), kk) sums the vectors j, j + G, .. of the tile ascending and adds the sum to the block's
//       partial in the workspace (zeroed by the block; the barrier after every chunk orders the tiles).
//   vqrr_final_kernel         one block: per stage the partials in block order in fp64, q, bits, rates[s] and dhist in fp64, written
//       as fp32; rate = the fp32 sum of the fp32 rates[s] in stage order.
// With WY the kernels also store index and y: vqres_rows_fwd_kernel's, bit for bit (the same helpers).  A thread beyond M works on
// zeros, adds zeros, stores nothing and reaches every barrier.  No atomics; grid, tile,
// path and every order of summation are functions of (M, D, L, G, n) alone: two calls give identical bits.
#include <math.h>

#include "common.h"
#include "vq_core.h"
#include "vq_res_rows.h"
#include "vq_rows.h"

namespace jpdse {

constexpr int kVqrrBlocks = 512;                  // cap of the blocks (= fp32 partials [n][G][L]) of the histogram launch
constexpr int kVqrrPartialWords = 1 << 22;        // cap of blocks * n * G * L: a workspace of at most 16 MiB
constexpr size_t kVqrrSlabBytes = 48 * 1024;      // the tables of a block of 4, 2 or 1 waves: with the staged book below 64 KiB
constexpr size_t kVqrrSlabOptin = 144 * 1024;     // one wave's tables above that: opted in; with the staged book below 160 KiB
constexpr int kVqrrFinalThreads = 1024;

// ---- launch geometry: functions of (M, D, L, G, n) alone -------------------------------------------------------------------------
// waves per block of the shuffle path; 0: the general path
static inline int vqrr_waves(int L, int G, int n) {
  if (G < 1 || G > 64 || (G & (G - 1)) != 0) return 0;
  const size_t slab = (size_t)n * G * (L + 1) * sizeof(float);
  for (int w = 4; w >= 1; w >>= 1)
    if (w * slab <= kVqrrSlabBytes) return w;
  return slab <= kVqrrSlabOptin ? 1 : 0;
}
static inline int vqrr_tile(int L, int G, int n) { return vqrr_waves(L, G, n) > 0 ? 64 * vqrr_waves(L, G, n) : 256; }
static inline int vqrr_blocks(int M, int L, int G, int n) {
  const int V = vqrr_tile(L, G, n);
  const int tiles = (M + V - 1) / V;
  int cap = kVqrrPartialWords / (n * G * L);
  cap = cap < 1 ? 1 : (cap > kVqrrBlocks ? kVqrrBlocks : cap);
  return tiles < cap ? tiles : cap;
}
static inline size_t vqrr_workspace_bytes(int M, int L, int G, int n) { return (size_t)vqrr_blocks(M, L, G, n) * n * G * L * sizeof(float); }
// LDS: cb [L][DP] when staged | slab [waves][n][G][L + 1] (shuffle path) or pt [KC][257] (general path)
static inline size_t vqrr_lds(int D, int L, int G, int n) {
  const int w = vqrr_waves(L, G, n);
  size_t words = vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) : 0;
  words += w > 0 ? (size_t)w * n * G * (L + 1) : (size_t)vqb_chunk(L) * 257;
  return words * sizeof(float);
}

// ---- the histogram launch ---------------------------------------------------------------------------------------------------------
// blockDim.x = 64 * waves = the vectors of a tile, a multiple of G.  partial: this block's [n][G][L] sums
template <typename T, int DP, bool CBL, bool WY>
__global__ __launch_bounds__(256) void vqrr_hist_kernel(const T* __restrict__ x, const float* __restrict__ books, int M, int D, int L,
                                                       int G, int n, float sigma, int vec, float* __restrict__ partial,
                                                       T* __restrict__ y, int* __restrict__ index) {
  extern __shared__ float vqrr_lds_mem[];
  const int V = blockDim.x, LS = L + 1, nw = V >> 6, LD = L * D;
  float* slab = vqrr_lds_mem + (CBL ? L * DP : 0);
  for (int i = threadIdx.x; i < nw * n * G * LS; i += V) slab[i] = 0.f;    // ordered before the first add by the barriers below
  const int ld = CBL ? DP : D;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool owner = lane < G;
  float* mine = slab + ((size_t)wave * n * G + (owner ? lane : 0)) * LS;   // the owner's row of stage 0 of the wave's tables
  const int ntiles = (M + V - 1) / V;
  if (!CBL) __syncthreads();
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;                       // a multiple of G: the group of vector m0 + t is lane % G
    float r[DP], a[DP];
    const VqResRow me = vqres_row_begin<T, DP>(x, M, D, m0, vec != 0, r, a);
    const bool live = me.live;
    const int m = me.m;
    for (int s = 0; s < n; ++s) {
      const float* cc = vqres_book<CBL>(books + (size_t)s * LD, vqrr_lds_mem, D, L, DP);
      int bk;
      const float dmin = vqres_nearest<DP, CBL>(r, cc, ld, D, L, bk);
      const float inv = vqres_inv_sum<DP, CBL>(r, cc, ld, D, L, dmin, sigma);
      float* tab = mine + (size_t)s * G * LS;
      for (int k = 0; k < L; ++k) {
        float v = live ? vq_weight(vqb_score<DP, CBL>(r, cc + k * ld, D), dmin, sigma) * inv : 0.f;
        for (int off = 32; off >= G; off >>= 1) v += __shfl_xor(v, off, 64);
        if (owner) tab[k] += v;
      }
      vqres_advance<DP, CBL, WY>(r, a, cc + bk * ld, D, s);
      if (WY && live) index[(size_t)s * M + m] = bk;
    }
    if (WY && live) vqb_store_row<T, DP>(y + me.row, D, vec != 0, a);
  }
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * n * G * L;
  for (int i = t; i < n * G * L; i += V) {
    const int sg = i / L, k = i - sg * L;          // sg = s G + g
    float acc = 0.f;
    for (int w = 0; w < nw; ++w) acc += slab[((size_t)w * n * G + sg) * LS + k];
    out[i] = acc;
  }
}

// 256 vectors per tile.  partial: this block's [n][G][L] sums, zeroed here and added to tile after tile
template <typename T, int DP, bool CBL, bool WY>
__global__ __launch_bounds__(256) void vqrr_hist_general_kernel(const T* __restrict__ x, const float* __restrict__ books, int M, int D,
                                                               int L, int G, int n, float sigma, int vec, float* partial,
                                                               T* __restrict__ y, int* __restrict__ index) {
  extern __shared__ float vqrr_lds_mem[];
  constexpr int V = 256;
  const int KC = vqb_chunk(L), LD = L * D;
  float* pt = vqrr_lds_mem + (CBL ? L * DP : 0);
  const int ld = CBL ? DP : D;
  const int t = threadIdx.x;
  float* mine = partial + (size_t)blockIdx.x * n * G * L;
  for (int i = t; i < n * G * L; i += V) mine[i] = 0.f;
  __syncthreads();
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    const int ns = G < nv ? G : nv;                // slot j holds the tile's vectors j, j + G, ..: group (m0 + j) % G
    float r[DP], a[DP];
    const VqResRow me = vqres_row_begin<T, DP>(x, M, D, m0, vec != 0, r, a);
    const bool live = me.live;
    const int m = me.m;
    for (int s = 0; s < n; ++s) {
      const float* cc = vqres_book<CBL>(books + (size_t)s * LD, vqrr_lds_mem, D, L, DP);
      int bk;
      const float dmin = vqres_nearest<DP, CBL>(r, cc, ld, D, L, bk);
      const float inv = vqres_inv_sum<DP, CBL>(r, cc, ld, D, L, dmin, sigma);
      float* tab = mine + (size_t)s * G * L;
      for (int k0 = 0; k0 < L; k0 += KC) {
        const int kc = L - k0 < KC ? L - k0 : KC;
        if (live)
          for (int kk = 0; kk < kc; ++kk)
            pt[kk * (V + 1) + t] = vq_weight(vqb_score<DP, CBL>(r, cc + (k0 + kk) * ld, D), dmin, sigma) * inv;
        __syncthreads();
        for (int w = t; w < kc * ns; w += V) {
          const int j = w / kc, kk = w - j * kc;
          float acc = 0.f;
          for (int v = j; v < nv; v += G) acc += pt[kk * (V + 1) + v];
          tab[(size_t)((m0 + j) % G) * L + k0 + kk] += acc;
        }
        __syncthreads();                           // pt is free again; the block's adds to `mine` are ordered tile by tile
      }
      vqres_advance<DP, CBL, WY>(r, a, cc + bk * ld, D, s);
      if (WY && live) index[(size_t)s * M + m] = bk;
    }
    if (WY && live) vqb_store_row<T, DP>(y + me.row, D, vec != 0, a);
  }
}

// ---- the final launch: one block ----------------------------------------------------------------------------------------------------
// Per stage s: hist[s][i] = sum_b partial[b][s][i] (b ascending, fp64), i = g L + k; every thread adds its terms of the stage in
// ascending i (i = t, t + 1024, ..), the 1024 sums are added in ascending t, 32 at a time, then the 32 in order: vqr_final_kernel's
// order (vq_bottleneck.hip).  cnt = M / G.
__global__ __launch_bounds__(kVqrrFinalThreads) void vqrr_final_kernel(const float* __restrict__ partial, int nb, int n, int GL, double cnt,
                                                                      double scale, double denom, float* __restrict__ hist,
                                                                      float* __restrict__ rate, float* __restrict__ rates,
                                                                      float* __restrict__ dhist) {
  __shared__ double red[kVqrrFinalThreads];
  __shared__ double red2[32];
  const int t = threadIdx.x;
  const size_t E = (size_t)n * GL;
  float total = 0.f;                               // thread 0's
  for (int s = 0; s < n; ++s) {
    double mysum = 0.0;
    for (int i = t; i < GL; i += kVqrrFinalThreads) {
      const size_t e = (size_t)s * GL + i;
      double acc = 0.0;
#pragma unroll 8
      for (int b = 0; b < nb; ++b) acc += (double)partial[(size_t)b * E + e];
      double term = 0.0, dh = 0.0;
      if (acc > 0.0) {
        const double lq = log2(acc / cnt);
        term = acc * lq;
        dh = scale * (-(lq + 1.4426950408889634)) / denom;      // 1 / ln 2
      }
      mysum += term;
      if (hist != nullptr) hist[e] = (float)acc;
      if (dhist != nullptr) dhist[e] = (float)dh;
    }
    red[t] = mysum;
    __syncthreads();
    if (t < 32) {
      double v = 0.0;
      for (int u = 0; u < 32; ++u) v += red[t * 32 + u];
      red2[t] = v;
    }
    __syncthreads();
    if (t == 0) {
      double v = 0.0;
      for (int u = 0; u < 32; ++u) v += red2[u];
      const float rs = (float)((0.0 - v) / denom);
      rates[s] = rs;
      total = s == 0 ? rs : total + rs;
    }
    __syncthreads();                               // red and red2 are free again
  }
  if (t == 0) rate[0] = total;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_res_rate_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G, int32_t n) {
  if (vq_res_grouped_check("vq_res_rate_workspace_size", JPDSE_F32, M, D, L, JPDSE_VQ_RES_MAX_STAGES, n, G) != JPDSE_OK) return 0;
  return vqrr_workspace_bytes(M, L, G, n);
}

int jpdse_vq_res_rate_fwd(const jpdse_vq_res_rate_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_rate_fwd: null argument struct");
  if (int rc = vq_res_grouped_check("vq_res_rate_fwd", a->dtype, a->M, a->D, a->L, a->S, a->n_stages, a->G)) return rc;
  JPDSE_REQUIRE(isfinite(a->sigma) && a->sigma > 0.f, "vq_res_rate_fwd: sigma is %g (a finite value > 0)", (double)a->sigma);
  JPDSE_REQUIRE(isfinite(a->scale), "vq_res_rate_fwd: scale is %g (a finite value)", (double)a->scale);
  JPDSE_REQUIRE(isfinite(a->denom) && a->denom > 0.f, "vq_res_rate_fwd: denom is %g (a finite value > 0)", (double)a->denom);
  JPDSE_REQUIRE(a->x && a->books, "vq_res_rate_fwd: null pointer (x, books)");
  JPDSE_REQUIRE(a->rate && a->rates, "vq_res_rate_fwd: null pointer (rate, rates)");
  JPDSE_REQUIRE((a->y == nullptr) == (a->index == nullptr), "vq_res_rate_fwd: y and index come together or not at all");
  const int M = a->M, D = a->D, L = a->L, G = a->G, n = a->n_stages;
  if (int rc = vq_ws_check("vq_res_rate_fwd", a->ws, a->ws_bytes, vqrr_workspace_bytes(M, L, G, n))) return rc;
  float* partial = mptr<float>(a->ws);
  const int waves = vqrr_waves(L, G, n), nb = vqrr_blocks(M, L, G, n);
  const int vec = vqb_vec(a->dtype, D, {a->x, a->y});
  const size_t lds = vqrr_lds(D, L, G, n);
  if (int rc = vqb_dispatch(a->dtype, D, L, [&](auto tag, auto dp, auto cbl) {
        using T = decltype(tag);
        constexpr int DP = decltype(dp)::value;
        constexpr bool CBL = decltype(cbl)::value;
        auto go = [&](auto kernel, int threads) {
          if (int rc = vq_lds_optin("vq_res_rate_fwd", kernel, lds)) return rc;
          return vq_launch("vq_res_rate_fwd", kernel, nb, threads, lds, a->stream, cptr<T>(a->x), a->books, M, D, L, G, n, a->sigma, vec,
                           partial, mptr<T>(a->y), a->index);
        };
        if (waves > 0)
          return a->y != nullptr ? go(vqrr_hist_kernel<T, DP, CBL, true>, 64 * waves) : go(vqrr_hist_kernel<T, DP, CBL, false>, 64 * waves);
        return a->y != nullptr ? go(vqrr_hist_general_kernel<T, DP, CBL, true>, 256) : go(vqrr_hist_general_kernel<T, DP, CBL, false>, 256);
      }))
    return rc;
  return vq_launch("vq_res_rate_fwd(final)", vqrr_final_kernel, 1, kVqrrFinalThreads, 0, a->stream, partial, nb, n, G * L, (double)(M / G),
                   (double)a->scale, (double)a->denom, a->hist, a->rate, a->rates, a->dhist);
}

}  // extern "C"
