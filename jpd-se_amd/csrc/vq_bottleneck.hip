// The soft-to-hard vector quantizer as a bottleneck: features in, features out, the [M][L] assignment never in HBM.
// Entry points: include/jpdse.h, "vector-quantizer bottleneck"; definition, reduction orders and measurements: DESIGN.md 4.15.
//   d[m][k] and p[m][k] are those of vq.hip: the direct score, j ascending; p with the row minimum subtracted
//   and the entry at the minimum exactly 1 before the division.
// Kernels (one THREAD per vector: x[m] lives in DP registers, DP = the power of two >= D in {4, 8, 16, 32}, padded with zeros):
//   vqb_fwd_kernel   sweep 1 over k: minimum and arg-min (strict <: the lowest k keeps a tie, a NaN never wins);
//                    sweep 2 (soft forward, or a pmf): e[k] = exp(-sigma (d - dmin)), s = sum e, a[j] = sum e[k] c[k][j], k ascending;
//                    y = a / s, or the gathered centre.  A pmf takes a third pass in chunks of KC centres: the tile's p = e / s goes
//                    to LDS, thread (k, part) sums its share of the tile's vectors ascending, the parts are added in order by one
//                    owner per k into the block's own fp32 partial.
//   vqb_bwd_kernel   p is recomputed from x: sweep 1 the minimum, sweep 2 s and sum e[k] dp[k] (dp[k] = <dy, c[k]> + dpmf[k] / M), sweep 3
//                    in chunks of KC centres: dd = -sigma p (dp - <p, dp>), dx += dd (x - c[k]) in registers; with a code-book
//                    gradient the chunk's p and dd go to LDS and thread ((k, j), part) sums p dy - 2 dd (x - c) over its share of the
//                    tile's vectors ascending, parts added in order into the block's fp32 partial [L][D].
//   vq_merge_kernel / vq_pmf_final_kernel (vq_core.h)   the partials in block order: fp32 for dC, fp64 for the pmf.
//   vq_rows.h (shared with vq_residual.hip)   the thread-per-vector geometry, row loads and stores, vqb_score, vqb_dot, dispatch.
//   Shared by the kernels, below: VqbBook (the code book's view), VqbTile + vqb_load_tile_row, vqb_nearest (sweep 1), vqb_e and
//   vqb_weight_sum (sweep 2): the forward and the general histogram.  vqb_bwd_kernel and vqr_hist_kernel keep their own
//   preamble and sweeps: on the helpers some instantiations of the first took more VGPRs, the second ran 2% slower (fp32, G 1).
//   The three chunk-to-LDS reductions stay apart: a "part" owns a span of vectors of one centre (forward pmf), of one (centre,
//   component) (backward dC) or a stride-G slot (general histogram); only the chunk bounds are common.
//   vqr_*            the rate term on per-group histograms: described where they stand, below the backward.
// The code book sits in LDS as [L][DP] (zero padded: every lane reads the same word, a broadcast, and the padded components add
// exact zeros) when that is at most 8 KiB; a larger one is read from global memory at wave-uniform addresses.
// No atomics; grids, tiles and chunks are functions of (M, D, L) alone; LDS per block below 64 KiB.
#include <math.h>

#include "common.h"
#include "vq_core.h"
#include "vq_rows.h"

namespace jpdse {

// ---- launch geometry: functions of (M, D, L) alone -------------------------------------------------------------------------
static inline size_t vqb_workspace_bytes(int M, int D, int L) {
  const size_t fwd = (size_t)vqb_blocks(M, 256) * L * sizeof(float);
  const size_t bwd = (size_t)vqb_blocks(M, vqb_bwd_threads(D)) * L * D * sizeof(float);
  return fwd > bwd ? fwd : bwd;
}
static inline size_t vqb_fwd_lds(int D, int L, bool pmf) {
  size_t n = vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) : 0;
  if (pmf) n += (size_t)vqb_chunk(L) * 257 + 256;
  return n * sizeof(float);
}
// nq: the words of the dq region (L: dpmf / M; G (L + 1): a staged dhist; 0: a dhist read from global memory)
static inline size_t vqb_bwd_lds(int D, int L, bool dc, size_t nq) {
  const int V = vqb_bwd_threads(D), KC = vqb_chunk(L);
  size_t n = (vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) : 0) + nq;
  if (dc) n += 2 * (size_t)KC * (V + 1) + 2 * (size_t)V * D + (size_t)(KC * D > V ? KC * D : V);
  return n * sizeof(float);
}

// The code book as a kernel reads it: CBL: staged here in LDS as [L][DP] (the caller synchronises before row()); otherwise the
// global [L][D].  row(k): centre k
template <int DP, bool CBL>
struct VqbBook {
  const float* cc;
  int ld;
  __device__ __forceinline__ VqbBook(const float* c, float* lds, int D, int L) : cc(CBL ? lds : c), ld(CBL ? DP : D) {
    if (CBL) vqb_stage(c, lds, D, L, DP);
  }
  __device__ __forceinline__ const float* row(int k) const { return cc + k * ld; }
};

// tile `tile` of V vectors, one per thread: the first vector, the vectors inside M, whether this thread has one
struct VqbTile {
  int m0, nv;
  bool live;
  __device__ __forceinline__ VqbTile(int tile, int V, int M) : m0(tile * V), nv(M - m0 < V ? M - m0 : V), live((int)threadIdx.x < nv) {}
  __device__ __forceinline__ int m() const { return m0 + threadIdx.x; }       // this thread's vector
};

// this thread's vector of the tile in DP registers; zeros for a thread without one
template <typename T, int DP>
__device__ __forceinline__ void vqb_load_tile_row(const T* x, const VqbTile& tl, int D, int vec, float (&xr)[DP]) {
#pragma unroll
  for (int j = 0; j < DP; ++j) xr[j] = 0.f;
  if (tl.live) vqb_load_row<T, DP>(x + (size_t)tl.m() * D, D, vec != 0, xr);
}

// sweep 1: the minimum score and its centre (strict <: the lower index keeps a tie; a NaN never wins)
template <int DP, bool CBL>
__device__ __forceinline__ float vqb_nearest(const float (&xr)[DP], const VqbBook<DP, CBL>& cb, int D, int L, int& bk) {
  float dmin = INFINITY;
  bk = 0;
  for (int k = 0; k < L; ++k) {
    const float d = vqb_score<DP, CBL>(xr, cb.row(k), D);
    if (d < dmin) {
      dmin = d;
      bk = k;
    }
  }
  return dmin;
}

// e[k], the numerator of p[m][k]: the callers divide by s (forward, backward) or multiply by 1 / s (rate term)
template <int DP, bool CBL>
__device__ __forceinline__ float vqb_e(const float (&xr)[DP], const VqbBook<DP, CBL>& cb, int k, int D, float dmin, float sigma) {
  return vq_weight(vqb_score<DP, CBL>(xr, cb.row(k), D), dmin, sigma);
}

// sweep 2 where nothing rides along: s = sum_k e[k], k ascending
template <int DP, bool CBL>
__device__ __forceinline__ float vqb_weight_sum(const float (&xr)[DP], const VqbBook<DP, CBL>& cb, int D, int L, float dmin,
                                                float sigma) {
  float s = 0.f;
  for (int k = 0; k < L; ++k) s += vqb_e(xr, cb, k, D, dmin, sigma);
  return s;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// LDS: cb [L][DP] when CBL | pt [KC][257] | red [256] with a pmf.  partial: this block's [L] sums of p, or nullptr.
template <typename T, int DP, bool CBL>
__global__ __launch_bounds__(256) void vqb_fwd_kernel(const T* __restrict__ x, const float* __restrict__ c, int M, int D, int L,
                                                     float sigma, int hard, int vec, T* __restrict__ y, int* __restrict__ index,
                                                     float* __restrict__ partial) {
  extern __shared__ float vqb_lds[];
  constexpr int V = 256;
  const int KC = vqb_chunk(L);
  float* pt = vqb_lds + (CBL ? L * DP : 0);
  float* red = pt + KC * (V + 1);
  const VqbBook<DP, CBL> cb(c, vqb_lds, D, L);
  if (CBL) __syncthreads();
  const int t = threadIdx.x;
  const int ntiles = (M + V - 1) / V;
  float* mine = partial != nullptr ? partial + (size_t)blockIdx.x * L : nullptr;
  bool first = true;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const VqbTile tl(tile, V, M);
    const int m0 = tl.m0, nv = tl.nv;
    const bool live = tl.live;
    const size_t row = (size_t)(m0 + t) * D;
    float xr[DP];
    vqb_load_tile_row<T, DP>(x, tl, D, vec, xr);
    int bk;
    const float dmin = vqb_nearest(xr, cb, D, L, bk);
    float s = 1.f;
    float a[DP];
    if (!hard || mine != nullptr) {
      s = 0.f;
#pragma unroll
      for (int j = 0; j < DP; ++j) a[j] = 0.f;
      for (int k = 0; k < L; ++k) {
        const float* ck = cb.row(k);
        const float e = vqb_e(xr, cb, k, D, dmin, sigma);
        s += e;
#pragma unroll
        for (int j = 0; j < DP; ++j)
          if (CBL || j < D) a[j] = __fmaf_rn(e, ck[j], a[j]);
      }
    }
    if (live) {
      index[m0 + t] = bk;
      if (hard) {
        const float* ck = cb.row(bk);
#pragma unroll
        for (int j = 0; j < DP; ++j) a[j] = (CBL || j < D) ? ck[j] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < DP; ++j) a[j] = a[j] / s;
      }
      vqb_store_row<T, DP>(y + row, D, vec != 0, a);
    }
    if (mine != nullptr) {
      const int parts = V / KC, span = (V + parts - 1) / parts;
      for (int k0 = 0; k0 < L; k0 += KC) {
        const int kc = L - k0 < KC ? L - k0 : KC;
        if (live)
          for (int kk = 0; kk < kc; ++kk)
            pt[kk * (V + 1) + t] = vqb_e(xr, cb, k0 + kk, D, dmin, sigma) / s;
        __syncthreads();
        {
          const int kk = t % KC, part = t / KC;
          if (part < parts && kk < kc) {
            const int v1 = (part + 1) * span < nv ? (part + 1) * span : nv;
            float acc = 0.f;
            for (int v = part * span; v < v1; ++v) acc += pt[kk * (V + 1) + v];
            red[part * KC + kk] = acc;
          }
        }
        __syncthreads();
        if (t < kc) {
          float acc = 0.f;
          for (int part = 0; part < parts; ++part) acc += red[part * KC + t];
          vq_partial_put(mine, k0 + t, first, acc);
        }
      }
    }
    first = false;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// blockDim.x = V vectors per tile.  LDS: cb [L][DP] when CBL | dq [L] = dpmf / M | with a partial: pt, ddt [KC][V + 1] | xt, dyt
// [V][D] | red [max(V, KC D)].  partial: this block's [L][D] sums, or nullptr: no code-book gradient.
// GM: the second term of dp[m][k].  0: dq[k] = dpmf[k] / M, G unused (jpdse_vq_quantize_bwd, and the grouped call without a
// dhist); 1: dpmf IS dhist [G][L], staged in LDS as dq [G][L + 1] (the odd stride: lanes of different groups on different
// banks) and read at the vector's group (m % G); 2: a dhist too large for LDS, read from global memory.
template <typename T, int DP, bool CBL, int GM>
__global__ __launch_bounds__(256) void vqb_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ c,
                                                     const float* __restrict__ dpmf, int M, int D, int L, int G, float sigma, int vec,
                                                     T* __restrict__ dx, float* __restrict__ partial) {
  extern __shared__ float vqb_lds[];
  const int V = blockDim.x;
  const int KC = L < kVqbChunk ? L : kVqbChunk;
  float* dq = vqb_lds + (CBL ? L * DP : 0);
  float* pt = dq + (GM == 1 ? G * (L + 1) : (GM == 2 ? 0 : L));
  float* ddt = pt + KC * (V + 1);
  float* xt = ddt + KC * (V + 1);
  float* dyt = xt + V * D;
  float* red = dyt + V * D;
  if (CBL) vqb_stage(c, vqb_lds, D, L, DP);
  if constexpr (GM == 0) {
    for (int k = threadIdx.x; k < L; k += V) dq[k] = dpmf != nullptr ? dpmf[k] / (float)M : 0.f;
  } else if constexpr (GM == 1) {
    for (int i = threadIdx.x; i < G * L; i += V) dq[(i / L) * (L + 1) + i % L] = dpmf[i];
  }
  __syncthreads();
  const float* cc = CBL ? vqb_lds : c;
  const int ld = CBL ? DP : D;
  const int t = threadIdx.x;
  const int ntiles = (M + V - 1) / V;
  float* mine = partial != nullptr ? partial + (size_t)blockIdx.x * L * D : nullptr;
  const int parts = V / (KC * D) > 1 ? V / (KC * D) : 1, span = (V + parts - 1) / parts;
  bool first = true;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    const bool live = t < nv;
    const size_t row = (size_t)(m0 + t) * D;
    float xr[DP], gr[DP], dxr[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) xr[j] = gr[j] = dxr[j] = 0.f;
    if (live) {
      vqb_load_row<T, DP>(x + row, D, vec != 0, xr);
      vqb_load_row<T, DP>(dy + row, D, vec != 0, gr);
    }
    // this vector's row of the second term of dp (a vector past M reads group 0's row: inside the table, never used)
    const float* dqr = dq;
    if constexpr (GM == 1) dqr = dq + (live ? (m0 + t) % G : 0) * (L + 1);
    if constexpr (GM == 2) dqr = dpmf + (size_t)(live ? (m0 + t) % G : 0) * L;
    float dmin = INFINITY;
    for (int k = 0; k < L; ++k) {
      const float d = vqb_score<DP, CBL>(xr, cc + k * ld, D);
      if (d < dmin) dmin = d;
    }
    float s = 0.f, pd = 0.f;
    for (int k = 0; k < L; ++k) {
      const float* ck = cc + k * ld;
      const float e = vq_weight(vqb_score<DP, CBL>(xr, ck, D), dmin, sigma);
      const float q = vqb_dot<DP, CBL>(gr, ck, D) + dqr[k];
      s += e;
      pd = __fmaf_rn(e, q, pd);
    }
    pd = pd / s;                               // <p, dp>
    if (mine != nullptr && live) {
#pragma unroll
      for (int j = 0; j < DP; ++j)
        if (j < D) {
          xt[t * D + j] = xr[j];
          dyt[t * D + j] = gr[j];
        }
    }
    for (int k0 = 0; k0 < L; k0 += KC) {
      const int kc = L - k0 < KC ? L - k0 : KC;
      for (int kk = 0; kk < kc; ++kk) {
        const float* ck = cc + (k0 + kk) * ld;
        const float p = vq_weight(vqb_score<DP, CBL>(xr, ck, D), dmin, sigma) / s;
        const float q = vqb_dot<DP, CBL>(gr, ck, D) + dqr[k0 + kk];
        const float dd = -sigma * (p * (q - pd));
#pragma unroll
        for (int j = 0; j < DP; ++j)
          if (CBL || j < D) dxr[j] = __fmaf_rn(dd, xr[j] - ck[j], dxr[j]);
        if (mine != nullptr && live) {
          pt[kk * (V + 1) + t] = p;
          ddt[kk * (V + 1) + t] = dd;
        }
      }
      if (mine != nullptr) {
        const int nown = kc * D;
        __syncthreads();
        for (int w = t; w < nown * parts; w += V) {
          const int part = w / nown, q = w - part * nown;
          const int kk = q / D, j = q - kk * D;
          const float ck = cc[(k0 + kk) * ld + j];
          const int v1 = (part + 1) * span < nv ? (part + 1) * span : nv;
          const float* pr = pt + kk * (V + 1);
          const float* dr = ddt + kk * (V + 1);
          float acc = 0.f;
          for (int v = part * span; v < v1; ++v) acc += pr[v] * dyt[v * D + j] - 2.f * (dr[v] * (xt[v * D + j] - ck));
          red[w] = acc;
        }
        __syncthreads();
        for (int q = t; q < nown; q += V) {
          float acc = 0.f;
          for (int part = 0; part < parts; ++part) acc += red[part * nown + q];
          vq_partial_put(mine, k0 * D + q, first, acc);
        }
      }
    }
    if (live && dx != nullptr) {
#pragma unroll
      for (int j = 0; j < DP; ++j) dxr[j] = 2.f * dxr[j];
      vqb_store_row<T, DP>(dx + row, D, vec != 0, dxr);
    }
    first = false;
    if (mine != nullptr) __syncthreads();      // the tile's xt / dyt / red are free again
  }
}

// ---- rate term: per-group histograms of p (include/jpdse.h, "the rate term on per-group histograms") ---------
// Group of a vector: m % G.  One thread per vector as above; p = e * (1 / s), or the one-hot of the arg-min with `hard`.
//   vqr_hist_kernel          G a power of two <= 64 whose [G][L + 1] table per wave fits kVqrSlabBytes with 4, 2 or 1 waves per
//                            block (= 256, 128 or 64 vectors per tile, all multiples of G: the group of a lane is lane % G).  Per
//                            centre the lanes of a group are summed across the wave with xor-shuffles, offsets 32, 16, .. G (hard:
//                            the group's bits of a ballot are counted, exact), lane g < G adds the sum into the wave's own table
//                            (stride L + 1: the G owners on different banks), tile after tile; the waves are merged in order at the end.
//   vqr_hist_general_kernel  any other G: chunks of KC centres go to LDS ([KC][257]), thread (slot j < min(G, vectors), kk) sums
//                            the vectors j, j + G, .. of the tile ascending and adds the sum to the block's partial in the
//                            workspace (zeroed by the block; a barrier after every chunk orders the tiles).
//   vqr_final_kernel         one block: the partials in block order in fp64, then q, bits, rate and dhist in fp64.
// No atomics; grid, tile and path are functions of (M, L, G) alone.
constexpr int kVqrBlocks = 512;              // cap of the blocks (= fp32 partials [G][L]) of the histogram launch
constexpr int kVqrPartialWords = 1 << 22;    // cap of blocks * G * L: a workspace of at most 16 MiB
constexpr int kVqrSlabBytes = 49152;         // the per-wave tables of a block; with the staged code book below 64 KiB
constexpr int kVqrFinalThreads = 1024;

// waves per block of the shuffle path; 0: the general path
static inline int vqr_waves(int D, int L, int G) {
  if (G < 1 || G > 64 || (G & (G - 1)) != 0) return 0;
  const size_t slab = (size_t)G * (L + 1) * sizeof(float);
  for (int w = 4; w >= 1; w >>= 1)
    if (w * slab <= (size_t)kVqrSlabBytes) return w;
  return 0;
}
static inline int vqr_tile(int D, int L, int G) { return vqr_waves(D, L, G) > 0 ? 64 * vqr_waves(D, L, G) : 256; }
static inline int vqr_blocks(int M, int L, int G) {
  const int V = vqr_tile(0, L, G);
  const int tiles = (M + V - 1) / V;
  int cap = kVqrPartialWords / (G * L);
  cap = cap < 1 ? 1 : (cap > kVqrBlocks ? kVqrBlocks : cap);
  return tiles < cap ? tiles : cap;
}
static inline size_t vqr_workspace_bytes(int M, int L, int G) { return (size_t)vqr_blocks(M, L, G) * G * L * sizeof(float); }
static inline size_t vqr_lds(int D, int L, int G) {
  const int w = vqr_waves(D, L, G);
  size_t n = vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) : 0;
  n += w > 0 ? (size_t)w * G * (L + 1) : (size_t)vqb_chunk(L) * 257;
  return n * sizeof(float);
}

// LDS: cb [L][DP] when CBL | slab [waves][G][L + 1].  partial: this block's [G][L] sums
template <typename T, int DP, bool CBL>
__global__ __launch_bounds__(256) void vqr_hist_kernel(const T* __restrict__ x, const float* __restrict__ c, int M, int D, int L, int G,
                                                      float sigma, int hard, int vec, float* __restrict__ partial) {
  extern __shared__ float vqb_lds[];
  const int V = blockDim.x, LS = L + 1, nw = V >> 6;
  float* slab = vqb_lds + (CBL ? L * DP : 0);
  if (CBL) vqb_stage(c, vqb_lds, D, L, DP);
  for (int i = threadIdx.x; i < nw * G * LS; i += V) slab[i] = 0.f;
  __syncthreads();
  const float* cc = CBL ? vqb_lds : c;
  const int ld = CBL ? DP : D;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool owner = lane < G;
  float* mine = slab + wave * G * LS + (owner ? lane : 0) * LS;     // the owner's row of the wave's table
  unsigned long long gmask = 0;                                     // the lanes of this lane's group
  for (int b = lane % G; b < 64; b += G) gmask |= 1ull << b;
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;                                        // a multiple of G: the group of vector m0 + t is lane % G
    const int nv = M - m0 < V ? M - m0 : V;
    const bool live = t < nv;
    float xr[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) xr[j] = 0.f;
    if (live) vqb_load_row<T, DP>(x + (size_t)(m0 + t) * D, D, vec != 0, xr);
    float dmin = INFINITY;
    int bk = 0;
    for (int k = 0; k < L; ++k) {
      const float d = vqb_score<DP, CBL>(xr, cc + k * ld, D);
      if (d < dmin) {
        dmin = d;
        bk = k;
      }
    }
    if (hard) {
      for (int k = 0; k < L; ++k) {
        const unsigned long long hit = __ballot(live && bk == k);
        if (hit != 0 && owner) mine[k] += (float)__popcll(hit & gmask);
      }
    } else {
      float s = 0.f;
      for (int k = 0; k < L; ++k) s += vq_weight(vqb_score<DP, CBL>(xr, cc + k * ld, D), dmin, sigma);
      const float inv = 1.f / s;
      for (int k = 0; k < L; ++k) {
        float v = live ? vq_weight(vqb_score<DP, CBL>(xr, cc + k * ld, D), dmin, sigma) * inv : 0.f;
        for (int off = 32; off >= G; off >>= 1) v += __shfl_xor(v, off, 64);
        if (owner) mine[k] += v;
      }
    }
  }
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * G * L;
  for (int i = t; i < G * L; i += V) {
    const int g = i / L, k = i - g * L;
    float acc = 0.f;
    for (int w = 0; w < nw; ++w) acc += slab[(w * G + g) * LS + k];
    out[i] = acc;
  }
}

// LDS: cb [L][DP] when CBL | pt [KC][257].  partial: this block's [G][L] sums, zeroed here and added to tile after tile
template <typename T, int DP, bool CBL>
__global__ __launch_bounds__(256) void vqr_hist_general_kernel(const T* __restrict__ x, const float* __restrict__ c, int M, int D,
                                                              int L, int G, float sigma, int hard, int vec, float* partial) {
  extern __shared__ float vqb_lds[];
  constexpr int V = 256;
  const int KC = vqb_chunk(L);
  float* pt = vqb_lds + (CBL ? L * DP : 0);
  const VqbBook<DP, CBL> cb(c, vqb_lds, D, L);
  const int t = threadIdx.x;
  float* mine = partial + (size_t)blockIdx.x * G * L;
  for (int i = t; i < G * L; i += V) mine[i] = 0.f;
  __syncthreads();
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const VqbTile tl(tile, V, M);
    const int m0 = tl.m0, nv = tl.nv;
    const bool live = tl.live;
    float xr[DP];
    vqb_load_tile_row<T, DP>(x, tl, D, vec, xr);
    int bk;
    const float dmin = vqb_nearest(xr, cb, D, L, bk);
    const float inv = hard ? 1.f : 1.f / vqb_weight_sum(xr, cb, D, L, dmin, sigma);
    const int ns = G < nv ? G : nv;            // slot j holds the tile's vectors j, j + G, ..: group (m0 + j) % G
    for (int k0 = 0; k0 < L; k0 += KC) {
      const int kc = L - k0 < KC ? L - k0 : KC;
      if (live)
        for (int kk = 0; kk < kc; ++kk) {
          const int k = k0 + kk;
          pt[kk * (V + 1) + t] = hard ? (bk == k ? 1.f : 0.f) : vqb_e(xr, cb, k, D, dmin, sigma) * inv;
        }
      __syncthreads();
      for (int w = t; w < kc * ns; w += V) {
        const int j = w / kc, kk = w - j * kc;
        float acc = 0.f;
        for (int v = j; v < nv; v += G) acc += pt[kk * (V + 1) + v];
        const int g = (m0 + j) % G;
        mine[(size_t)g * L + k0 + kk] += acc;
      }
      __syncthreads();                         // pt is free again; the block's adds to `mine` are ordered tile by tile
    }
  }
}

// hist[i] = sum_b partial[b][i] (b ascending, fp64), i = g L + k; n = M / G.  One block of kVqrFinalThreads threads
__global__ __launch_bounds__(kVqrFinalThreads) void vqr_final_kernel(const float* __restrict__ partial, int nb, int G, int L, double n,
                                                                    double scale, double denom, float* __restrict__ hist,
                                                                    float* __restrict__ rate, float* __restrict__ dhist) {
  __shared__ double red[kVqrFinalThreads];
  __shared__ double red2[32];
  const int E = G * L, t = threadIdx.x;
  double mysum = 0.0;
  for (int i = t; i < E; i += kVqrFinalThreads) {
    double acc = 0.0;
#pragma unroll 8
    for (int b = 0; b < nb; ++b) acc += (double)partial[(size_t)b * E + i];
    double term = 0.0, dh = 0.0;
    if (acc > 0.0) {
      const double lq = log2(acc / n);
      term = acc * lq;
      dh = scale * (-(lq + 1.4426950408889634)) / denom;      // 1 / ln 2
    }
    mysum += term;
    if (hist != nullptr) hist[i] = (float)acc;
    if (dhist != nullptr) dhist[i] = (float)dh;
  }
  red[t] = mysum;
  __syncthreads();
  if (t < 32) {
    double a = 0.0;
    for (int u = 0; u < 32; ++u) a += red[t * 32 + u];
    red2[t] = a;
  }
  __syncthreads();
  if (t == 0) {
    double a = 0.0;
    for (int u = 0; u < 32; ++u) a += red2[u];
    rate[0] = (float)((0.0 - a) / denom);
  }
}

// both backward entry points after their shape checks.  second: dpmf [L] (grouped false) or dhist [G][L] (grouped true), or NULL
static int vqb_bwd_run(const char* who, int dtype, int M, int D, int L, int G, float sigma, const void* dy, const void* x,
                       const float* code_book, const float* second, bool grouped, void* dx, float* dcode_book, void* ws,
                       size_t ws_bytes, void* stream) {
  JPDSE_REQUIRE(dy && x && code_book, "%s: null pointer", who);
  float* partial = nullptr;
  if (dcode_book != nullptr) {
    if (int rc = vq_ws_check(who, ws, ws_bytes, vqb_workspace_bytes(M, D, L))) return rc;
    partial = mptr<float>(ws);
  }
  if (dx == nullptr && partial == nullptr) return JPDSE_OK;
  const int V = vqb_bwd_threads(D), nb = vqb_blocks(M, V);
  const int vec = vqb_vec(dtype, D, {x, dy, dx});
  // a dhist goes to LDS when the block's LDS stays below 64000 bytes with it, otherwise it is read from global memory
  int gm = 0;
  if (grouped) gm = vqb_bwd_lds(D, L, partial != nullptr, (size_t)G * (L + 1)) <= 64000 ? 1 : 2;
  const size_t lds = vqb_bwd_lds(D, L, partial != nullptr, gm == 1 ? (size_t)G * (L + 1) : (gm == 2 ? 0 : (size_t)L));
  if (int rc = vqb_dispatch(dtype, D, L, [&](auto tag, auto dp, auto cbl) {
        using T = decltype(tag);
        constexpr int DPv = decltype(dp)::value;
        constexpr bool CBLv = decltype(cbl)::value;
        auto go = [&](auto kernel) {
          return vq_launch(who, kernel, nb, V, lds, stream, cptr<T>(dy), cptr<T>(x), code_book, second, M, D, L, G, sigma, vec,
                            mptr<T>(dx), partial);
        };
        if (gm == 1) return go(vqb_bwd_kernel<T, DPv, CBLv, 1>);
        if (gm == 2) return go(vqb_bwd_kernel<T, DPv, CBLv, 2>);
        return go(vqb_bwd_kernel<T, DPv, CBLv, 0>);
      }))
    return rc;
  if (partial == nullptr) return JPDSE_OK;
  return vq_launch(who, vq_merge_kernel, ew_blocks(L * D), 256, 0, stream, partial, nb, L * D, 1.f, dcode_book);
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_quantize_workspace_size(int32_t M, int32_t D, int32_t L) {
  if (vq_shape_check("vq_quantize_workspace_size", M, D, L) != JPDSE_OK) return 0;
  return vqb_workspace_bytes(M, D, L);
}

int jpdse_vq_quantize_fwd(const jpdse_vq_quantize_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_quantize_fwd: null argument struct");
  if (int rc = vqb_common_check("vq_quantize_fwd", a->dtype, a->M, a->D, a->L, a->sigma)) return rc;
  JPDSE_REQUIRE(a->x && a->code_book && a->y && a->index, "vq_quantize_fwd: null pointer");
  const int M = a->M, D = a->D, L = a->L;
  const int nb = vqb_blocks(M, 256);
  float* partial = nullptr;
  if (a->pmf != nullptr) {
    if (int rc = vq_ws_check("vq_quantize_fwd", a->ws, a->ws_bytes, vqb_workspace_bytes(M, D, L))) return rc;
    partial = mptr<float>(a->ws);
  }
  const int vec = vqb_vec(a->dtype, D, {a->x, a->y});
  const size_t lds = vqb_fwd_lds(D, L, partial != nullptr);
  if (int rc = vqb_dispatch(a->dtype, D, L, [&](auto tag, auto dp, auto cbl) {
        using T = decltype(tag);
        return vq_launch("vq_quantize_fwd", vqb_fwd_kernel<T, decltype(dp)::value, decltype(cbl)::value>, nb, 256, lds, a->stream,
                          cptr<T>(a->x), a->code_book, M, D, L, a->sigma, a->hard_forward != 0 ? 1 : 0, vec, mptr<T>(a->y),
                          a->index, partial);
      }))
    return rc;
  if (partial == nullptr) return JPDSE_OK;
  return vq_launch("vq_quantize_fwd(pmf)", vq_pmf_final_kernel, 1, 256, 0, a->stream, partial, nb, L, (double)M, a->pmf);
}

int jpdse_vq_quantize_bwd(const jpdse_vq_quantize_bwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_quantize_bwd: null argument struct");
  if (int rc = vqb_common_check("vq_quantize_bwd", a->dtype, a->M, a->D, a->L, a->sigma)) return rc;
  return vqb_bwd_run("vq_quantize_bwd", a->dtype, a->M, a->D, a->L, 1, a->sigma, a->dy, a->x, a->code_book, a->dpmf, false, a->dx,
                     a->dcode_book, a->ws, a->ws_bytes, a->stream);
}

int jpdse_vq_quantize_bwd_grouped(const jpdse_vq_quantize_bwd_grouped_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_quantize_bwd_grouped: null argument struct");
  if (int rc = vqb_common_check("vq_quantize_bwd_grouped", a->dtype, a->M, a->D, a->L, a->sigma)) return rc;
  if (int rc = vqr_group_check("vq_quantize_bwd_grouped", a->M, a->L, a->G)) return rc;
  return vqb_bwd_run("vq_quantize_bwd_grouped", a->dtype, a->M, a->D, a->L, a->G, a->sigma, a->dy, a->x, a->code_book, a->dhist,
                     a->dhist != nullptr, a->dx, a->dcode_book, a->ws, a->ws_bytes, a->stream);
}

size_t jpdse_vq_rate_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G) {
  if (vq_shape_check("vq_rate_workspace_size", M, D, L) != JPDSE_OK) return 0;
  if (vqr_group_check("vq_rate_workspace_size", M, L, G) != JPDSE_OK) return 0;
  return vqr_workspace_bytes(M, L, G);
}

int jpdse_vq_rate_fwd(const jpdse_vq_rate_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_rate_fwd: null argument struct");
  if (int rc = vqb_common_check("vq_rate_fwd", a->dtype, a->M, a->D, a->L, a->sigma)) return rc;
  if (int rc = vqr_group_check("vq_rate_fwd", a->M, a->L, a->G)) return rc;
  JPDSE_REQUIRE(isfinite(a->scale), "vq_rate_fwd: scale is %g (a finite value)", (double)a->scale);
  JPDSE_REQUIRE(isfinite(a->denom) && a->denom > 0.f, "vq_rate_fwd: denom is %g (a finite value > 0)", (double)a->denom);
  JPDSE_REQUIRE(a->x && a->code_book && a->rate, "vq_rate_fwd: null pointer");
  const int M = a->M, D = a->D, L = a->L, G = a->G;
  if (int rc = vq_ws_check("vq_rate_fwd", a->ws, a->ws_bytes, vqr_workspace_bytes(M, L, G))) return rc;
  float* partial = mptr<float>(a->ws);
  const int waves = vqr_waves(D, L, G), nb = vqr_blocks(M, L, G);
  const int vec = vqb_vec(a->dtype, D, {a->x});
  const int hard = a->hard != 0 ? 1 : 0;
  const size_t lds = vqr_lds(D, L, G);
  if (int rc = vqb_dispatch(a->dtype, D, L, [&](auto tag, auto dp, auto cbl) {
        using T = decltype(tag);
        constexpr int DPv = decltype(dp)::value;
        constexpr bool CBLv = decltype(cbl)::value;
        if (waves > 0)
          return vq_launch("vq_rate_fwd", vqr_hist_kernel<T, DPv, CBLv>, nb, 64 * waves, lds, a->stream, cptr<T>(a->x),
                            a->code_book, M, D, L, G, a->sigma, hard, vec, partial);
        return vq_launch("vq_rate_fwd", vqr_hist_general_kernel<T, DPv, CBLv>, nb, 256, lds, a->stream, cptr<T>(a->x),
                          a->code_book, M, D, L, G, a->sigma, hard, vec, partial);
      }))
    return rc;
  return vq_launch("vq_rate_fwd(final)", vqr_final_kernel, 1, kVqrFinalThreads, 0, a->stream, partial, nb, G, L, (double)(M / G),
                    (double)a->scale, (double)a->denom, a->hist, a->rate, a->dhist);
}

}  // extern "C"
