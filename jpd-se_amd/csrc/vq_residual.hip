// Residual (multi-stage) soft-to-hard vector quantizer (ctu.quantizers.ResidualS2HVQ).
// Entry points: include/jpdse.h, "residual vector quantizer"; definition, surrogate gradient and measurements: DESIGN.md 4.23.
//   x [M][D] (fp32 or bf16), S code books fp32 [S][L][D], n <= S stages in use.  The chain (r_1 = x, k_s, r_{s+1} = r_s - C_s[k_s],
//   y = C_1[k_1] + .. + C_n[k_n]) and the barrier rule of the per-row kernels: vq_res_rows.h.  The group kernel scores with
//   vq.hip's direct score (vq_scores, lowest index on a tie) and forms the same r and y.
// Kernels:
//   vqres_fwd_kernel     a block walks tiles of 256 vectors whose residual sits in LDS as fp32 [256][D].  The S books do not fit
//       in LDS together (4 x 512 x 32 fp32 = 256 KiB), so the STAGE loop is the outer loop of a tile: stage book s transposed
//       (vq_stage_transposed), assign the tile's vectors in the group layout of vq_hard_fwd_kernel (the residual row takes the place
//       of x), synchronise, subtract the chosen centres (one thread per (vector, component), the book still in LDS) and sum the
//       squares of the new residual in fp64, synchronise, next book.  x is read once; y is summed at the end from the tile's
//       indices (LDS) and the books (L2) by the function the decoder uses; a residual is written only when asked for.
//   vqres_rows_fwd_kernel   index and y of the kernel above, bit for bit, by one THREAD per vector (vq_res_rows.h):
//       the chain's pieces in stage order and nothing else.  No sse, no residual.
//   vqres_decode_kernel  one thread per (vector, component): the same sum from the index planes.
//   vqres_bwd_kernel     one THREAD per vector (vq_rows.h), stages descending.  r_s is recomputed from x and the indices by the
//       chain's subtractions, a_s = dy - h_{s+1}, then the three sweeps and the code-book-gradient reduction of vqb_bwd_kernel
//       (vq_bottleneck.hip) at (r_s, a_s): u_s into registers, the stage's [L][D] share into the block's partial [n][L][D];
//       h_s = h_{s+1} + u_s; dx = h_1.  vq_merge_kernel (vq_core.h) adds the partials in block order.
//   vqres_sse_kernel     sse[s] = the blocks' fp64 partials in block order (vq_block_sum, vq_core.h).
//   DEP: a per-row stage depth on the three kernels above that work per row.  depth int32 [M / G], the cell of row m
//       is m / G, n_m = min(n, depth clamped to 1 .. S).  By the barrier rule (vq_res_rows.h) n_m is a PREDICATE inside the stage
//       loop: a row past its depth computes nothing and stores nothing but its -1 (forward) or the zeros of its LDS slots
//       (backward); a wave whose rows are all past their depth skips the score loops by ordinary divergence.
//   vqres_depth_map_kernel  the cell depths from a label map: one thread per cell, the maximum over its step x step pixels.
// No atomics; grids, tiles and chunks are functions of (M, D, L, n) alone: two calls give identical bits.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "vq_core.h"
#include "vq_res_rows.h"
#include "vq_rows.h"

namespace jpdse {

constexpr int kVqResMaxStages = JPDSE_VQ_RES_MAX_STAGES;
constexpr int kVqResTile = 256;              // vectors per tile of the forward
constexpr int kVqResFwdBlocks = 2048;        // cap of the blocks (= fp64 partials [n]) of the forward
constexpr int kVqResPartialWords = 1 << 26;  // cap of blocks * n * L * D of the backward: partials of at most 256 MiB

// ---- launch geometry: functions of (M, D, L, n) alone ---------------------------------------------------------------------------
static inline int vqres_fwd_blocks(int M) {
  const int tiles = (M + kVqResTile - 1) / kVqResTile;
  return tiles < kVqResFwdBlocks ? tiles : kVqResFwdBlocks;
}
// LDS of the forward: red fp64 [4] | bsse fp64 [8] | ct [D][L] | r [256][D] | it int32 [8][256]: at most 106592 bytes
static inline size_t vqres_fwd_lds(int D, int L) {
  return (4 + kVqResMaxStages) * sizeof(double) + ((size_t)D * L + (size_t)kVqResTile * D + (size_t)kVqResMaxStages * kVqResTile) * sizeof(float);
}
static inline int vqres_bwd_blocks(int M, int D, int L, int n) {
  const int nb = vqb_blocks(M, vqb_bwd_threads(D));
  int cap = kVqResPartialWords / (n * L * D);
  cap = cap < 1 ? 1 : cap;
  return nb < cap ? nb : cap;
}
// LDS of the backward: cb [L][DP] when staged | dq [G][L + 1] with a staged dhist | with a partial: pt, ddt [KC][V + 1] | xt, dyt [V][D] | red [max(V, KC D)]
// nq: the words of a staged slice of dhist, G (L + 1), or 0
static inline size_t vqres_bwd_lds(int D, int L, bool dc, size_t nq = 0) {
  const int V = vqb_bwd_threads(D), KC = vqb_chunk(L);
  size_t w = (vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) : 0) + nq;
  if (dc) w += 2 * (size_t)KC * (V + 1) + 2 * (size_t)V * D + (size_t)(KC * D > V ? KC * D : V);
  return w * sizeof(float);
}
size_t vq_res_workspace_bytes(int M, int D, int L, int n) {
  const size_t fwd = (size_t)vqres_fwd_blocks(M) * n * sizeof(double);
  const size_t bwd = (size_t)vqres_bwd_blocks(M, D, L, n) * n * L * D * sizeof(float);
  return fwd > bwd ? fwd : bwd;
}

// ---- device helpers ---------------------------------------------------------------------------------------------------------
// component j of C_1[k(0)] + .. + C_n[k(n - 1)]: fp32, stage order, starting FROM the first centre (n == 1: a bit-exact gather)
template <typename K>
__device__ __forceinline__ float vqres_sum(const float* __restrict__ books, int LD, int D, int n, int j, K k) {
  if (n == 0) return 0.f;
  float acc = books[k(0) * D + j];
  for (int s = 1; s < n; ++s) acc += books[(size_t)s * LD + k(s) * D + j];
  return acc;
}

// ---- per-row stage depth -------------------------------------------------------------------------------------
// The last parameter of the per-row kernels.  DEP false: an empty struct, n_m = n for every row, and the kernel's code is what it
// was without the parameter.
template <bool DEP>
struct VqDepth {};
template <>
struct VqDepth<true> {
  const int* depth;                              // [M / G]
  int G;
};
// n_m = min(n, depth[m / G] clamped to 1 .. S) = depth[m / G] clamped to 1 .. n (n <= S): a hostile map cannot reach past the books
template <bool DEP>
__device__ __forceinline__ int vqres_row_stages(const VqDepth<DEP>& dep, int m, int n) {
  if constexpr (DEP) {
    const int d = dep.depth[m / dep.G];
    return d < 1 ? 1 : (d < n ? d : n);
  } else {
    return n;
  }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// psse: this block's fp64 [n] sums of |r_{s+1}|^2, or nullptr.  index: [n][M].  residual: fp32 [M][D] = r_{n+1}, or nullptr
template <typename T>
__global__ __launch_bounds__(256) void vqres_fwd_kernel(const T* __restrict__ x, const float* __restrict__ books, int M, int D, int L,
                                                       int n, int GL, T* __restrict__ y, int* __restrict__ index,
                                                       double* __restrict__ psse, float* __restrict__ residual) {
  extern __shared__ double vqres_lds[];
  constexpr int V = kVqResTile;
  double* red = vqres_lds;
  double* bsse = red + 4;
  float* ct = reinterpret_cast<float*>(bsse + kVqResMaxStages);
  float* r = ct + D * L;
  int* it = reinterpret_cast<int*>(r + V * D);
  const int t = threadIdx.x, LD = L * D;
  const VqLanes ln(GL, L);
  const int lane = ln.lane, wave = ln.wave, kk = ln.kk;
  if (t < kVqResMaxStages) bsse[t] = 0.0;        // thread 0 adds to them after the barriers below
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    const size_t e0 = (size_t)m0 * D;
    for (int i = t; i < nv * D; i += 256) r[i] = ElemOps<T>::ld(x + e0 + i);
    for (int s = 0; s < n; ++s) {
      __syncthreads();                           // r is complete (the load, or the subtraction of stage s - 1); ct is free
      vq_stage_transposed(books + (size_t)s * LD, ct, D, L);
      __syncthreads();
      for (int vb = wave * ln.vpw; vb < nv; vb += 4 * ln.vpw) {
        const bool live = vb + ln.g < nv;
        const int v = live ? vb + ln.g : nv - 1;
        float d[kVqSlots];
        vq_scores(r, ct, v, D, ln, d);
        float best = INFINITY;
        int bk = kk < L ? kk : 0x7fffffff;
        if (kk < L) best = d[0];
#pragma unroll
        for (int i = 1; i < kVqSlots; ++i)
          if (ln.slot_live(i) && d[i] < best) {  // strict: the lower index keeps a tie
            best = d[i];
            bk = ln.centre(i);
          }
        vq_group_arg<true>(best, bk, GL);
        bk = __shfl(bk, lane & ~(GL - 1), 64);   // group lane 0 decides for the row
        bk = bk < L ? bk : L - 1;
        if (live && kk == 0) {
          it[s * V + v] = bk;
          index[(size_t)s * M + m0 + v] = bk;
        }
      }
      __syncthreads();
      double acc = 0.0;
      for (int i = t; i < nv * D; i += 256) {
        const int v = i / D, j = i - v * D;
        const float rv = r[i] - ct[j * L + it[s * V + v]];
        r[i] = rv;
        acc += (double)rv * (double)rv;
      }
      if (psse != nullptr) {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (t == 0) bsse[s] += ((red[0] + red[1]) + red[2]) + red[3];
      }
    }
    __syncthreads();                             // r and it are final
    for (int i = t; i < nv * D; i += 256) {
      const int v = i / D, j = i - v * D;
      ElemOps<T>::st(y + e0 + i, vqres_sum(books, LD, D, n, j, [&](int s) { return it[s * V + v]; }));
      if (residual != nullptr) residual[e0 + i] = r[i];
    }
    __syncthreads();                             // r and it are free again
  }
  if (psse != nullptr && t == 0)
    for (int s = 0; s < n; ++s) psse[(size_t)blockIdx.x * n + s] = bsse[s];
}

// ---- forward, one thread per vector ------------------------------------------------------------------------------
// The chain of vq_res_rows.h: r and the running sum a of a vector in DP registers each, the stage loop inside the thread.  LDS: cb
// [L][DP] when CBL.  index: [n][M], n >= 1.
// DEP: row m takes its first n_m stages and stores index[s][m] = -1 for the others.  The barrier rule: the loop bound is n for
// every thread, s < n_m is a predicate, and the `continue` of a row past its depth leads to the next stage's barriers.
template <typename T, int DP, bool CBL, bool DEP>
__global__ __launch_bounds__(256) void vqres_rows_fwd_kernel(const T* __restrict__ x, const float* __restrict__ books, int M, int D,
                                                            int L, int n, int vec, T* __restrict__ y, int* __restrict__ index,
                                                            VqDepth<DEP> dep) {
  extern __shared__ float vqresr_lds[];
  constexpr int V = 256;
  const int ld = CBL ? DP : D;
  const int LD = L * D;
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    float r[DP], a[DP];
    const VqResRow me = vqres_row_begin<T, DP>(x, M, D, tile * V, vec != 0, r, a);
    const int nm = me.live ? vqres_row_stages(dep, me.m, n) : 0; // DEP: a thread without a vector takes no stage
    for (int s = 0; s < n; ++s) {
      const float* cc = vqres_book<CBL>(books + (size_t)s * LD, vqresr_lds, D, L, DP);
      if constexpr (DEP) {
        if (s >= nm) {                           // past the row's depth: after this stage's barriers, before the next one's
          if (me.live) index[(size_t)s * M + me.m] = -1;
          continue;
        }
      }
      int bk;
      vqres_nearest<DP, CBL>(r, cc, ld, D, L, bk);
      vqres_advance<DP, CBL, true>(r, a, cc + bk * ld, D, s);
      if (me.live) index[(size_t)s * M + me.m] = bk;
    }
    if (me.live) vqb_store_row<T, DP>(y + me.row, D, vec != 0, a);
  }
}

__global__ __launch_bounds__(64) void vqres_sse_kernel(const double* __restrict__ psse, int nb, int n, double* __restrict__ sse) {
  const int s = threadIdx.x;
  if (s >= n) return;
  sse[s] = vq_block_sum(psse, nb, n, s);
}

// ---- decode -----------------------------------------------------------------------------------------------------------------
// DEP: the first n_m centres of row m; index[s][m] for s >= n_m is never read
template <typename T, bool DEP>
__global__ __launch_bounds__(256) void vqres_decode_kernel(const int* __restrict__ index, const float* __restrict__ books, int M, int D,
                                                          int L, int n, T* __restrict__ y, int* __restrict__ status, VqDepth<DEP> dep) {
  const long long total = (long long)M * D;
  const int LD = L * D;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / D), j = (int)(i - (long long)m * D);
    bool bad = false;
    const float v = vqres_sum(books, LD, D, vqres_row_stages(dep, m, n), j, [&](int s) {
      int k = index[(size_t)s * M + m];
      if ((unsigned)k >= (unsigned)L) {
        k = 0;
        bad = true;
      }
      return k;
    });
    if (bad && j == 0) *status = 1;              // every writer stores the same word
    ElemOps<T>::st(y + i, v);
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// blockDim.x = V vectors per tile.  partial: this block's [n][L][D] sums, or nullptr: no code-book gradient.
// GM: the rate term's share of dp[m][k].  0: none, dhist and G unused (jpdse_vq_res_bwd, and the grouped call without
// a dhist); 1: dhist [n][G][L], the stage's slice staged in LDS as dq [G][L + 1] where the stage's book is restaged (the odd stride:
// lanes of different groups on different banks) and read at the vector's group (m % G); 2: a slice too large for LDS, read from
// global memory.
// DEP (with GM 0): row m runs the recursion over its first n_m stages, h_{n_m + 1} = 0.  The barrier rule of the file's head: s runs
// over all n stages in every thread; at a stage s >= n_m the row reads neither x, dy nor index (index[s][m] is -1 there), skips the
// sweeps, keeps h = 0 and, with a partial, writes ZEROS into its slots of xt, dyt, pt and ddt, so the reduction adds exactly nothing
// for it (a stale slot could hold anything, and 0 * stale may be NaN).
template <typename T, int DP, bool CBL, int GM, bool DEP>
__global__ __launch_bounds__(256) void vqres_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ books,
                                                       const int* __restrict__ index, const float* __restrict__ dhist, int M, int D,
                                                       int L, int n, int G, float sigma, int vec, T* __restrict__ dx,
                                                       float* __restrict__ partial, VqDepth<DEP> dep) {
  extern __shared__ float vqresb_lds[];
  const int V = blockDim.x;
  const int KC = vqb_chunk(L);
  float* dq = vqresb_lds + (CBL ? L * DP : 0);
  float* pt = dq + (GM == 1 ? G * (L + 1) : 0);
  float* ddt = pt + KC * (V + 1);
  float* xt = ddt + KC * (V + 1);
  float* dyt = xt + V * D;
  float* red = dyt + V * D;
  const int ld = CBL ? DP : D;
  const int t = threadIdx.x, LD = L * D;
  const int ntiles = (M + V - 1) / V;
  float* mine = partial != nullptr ? partial + (size_t)blockIdx.x * n * LD : nullptr;
  const int parts = V / (KC * D) > 1 ? V / (KC * D) : 1, span = (V + parts - 1) / parts;
  bool first = true;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    const bool live = t < nv;
    const int m = live ? m0 + t : M - 1;
    const size_t row = (size_t)m * D;
    float h[DP];                                 // h_{s+1}: the gradient that the later stages sent back to r_{s+1}
#pragma unroll
    for (int j = 0; j < DP; ++j) h[j] = 0.f;
    const int nm = live ? vqres_row_stages(dep, m, n) : 0;
    for (int s = n - 1; s >= 0; --s) {
      const bool act = DEP ? s < nm : live;      // the row takes part in this stage
      const float* c = books + (size_t)s * LD;
      __syncthreads();                           // the staged book, xt, dyt and red of the stage before are free
      if (CBL) vqb_stage(c, vqresb_lds, D, L, DP);
      if constexpr (GM == 1) {
        const float* dh = dhist + (size_t)s * G * L;
        for (int i = t; i < G * L; i += V) dq[(i / L) * (L + 1) + i % L] = dh[i];
      }
      // this vector's row of the stage's slice (a vector past M reads group 0's row: inside the table, never used)
      const float* dqr = nullptr;
      if constexpr (GM == 1) dqr = dq + (live ? m % G : 0) * (L + 1);
      if constexpr (GM == 2) dqr = dhist + ((size_t)s * G + (live ? m % G : 0)) * L;
      float xr[DP], gr[DP], dxr[DP];
#pragma unroll
      for (int j = 0; j < DP; ++j) xr[j] = gr[j] = dxr[j] = 0.f;
      if (act) {
        vqb_load_row<T, DP>(x + row, D, vec != 0, xr);
        for (int u = 0; u < s; ++u) {            // r_s by the chain's subtractions (vq_res_rows.h), in its order
          const float* cu = books + (size_t)u * LD + index[(size_t)u * M + m] * D;
#pragma unroll
          for (int j = 0; j < DP; ++j)
            if (j < D) xr[j] = xr[j] - cu[j];
        }
        vqb_load_row<T, DP>(dy + row, D, vec != 0, gr);
#pragma unroll
        for (int j = 0; j < DP; ++j) gr[j] = gr[j] - h[j];        // a_s
        if (mine != nullptr) {
#pragma unroll
          for (int j = 0; j < DP; ++j)
            if (j < D) {
              xt[t * D + j] = xr[j];
              dyt[t * D + j] = gr[j];
            }
        }
      } else if constexpr (DEP) {
        if (live && mine != nullptr)             // a row of the tile past its depth: zeros, never a stale slot
          for (int j = 0; j < D; ++j) xt[t * D + j] = dyt[t * D + j] = 0.f;
      }
      __syncthreads();
      const float* cc = CBL ? vqresb_lds : c;
      float dmin = INFINITY;
      float sum = 0.f, pd = 0.f;
      if (!DEP || act) {
        int bk;                                  // the chain's sweep 1; the forward stored its centre
        dmin = vqres_nearest<DP, CBL>(xr, cc, ld, D, L, bk);
        for (int k = 0; k < L; ++k) {
          const float* ck = cc + k * ld;
          const float e = vq_weight(vqb_score<DP, CBL>(xr, ck, D), dmin, sigma);
          float q = vqb_dot<DP, CBL>(gr, ck, D);
          if constexpr (GM != 0) q += dqr[k];
          sum += e;
          pd = __fmaf_rn(e, q, pd);
        }
        pd = pd / sum;                           // <p, dp>
      }
      for (int k0 = 0; k0 < L; k0 += KC) {       // every thread: the reduction below holds barriers
        const int kc = L - k0 < KC ? L - k0 : KC;
        for (int kq = 0; kq < kc; ++kq) {
          if constexpr (DEP) {
            if (!act) {
              if (mine != nullptr && live) pt[kq * (V + 1) + t] = ddt[kq * (V + 1) + t] = 0.f;
              continue;
            }
          }
          const float* ck = cc + (k0 + kq) * ld;
          const float p = vq_weight(vqb_score<DP, CBL>(xr, ck, D), dmin, sigma) / sum;
          float q = vqb_dot<DP, CBL>(gr, ck, D);
          if constexpr (GM != 0) q += dqr[k0 + kq];
          const float dd = -sigma * (p * (q - pd));
#pragma unroll
          for (int j = 0; j < DP; ++j)
            if (CBL || j < D) dxr[j] = __fmaf_rn(dd, xr[j] - ck[j], dxr[j]);
          if (mine != nullptr && live) {
            pt[kq * (V + 1) + t] = p;
            ddt[kq * (V + 1) + t] = dd;
          }
        }
        if (mine != nullptr) {
          const int nown = kc * D;
          __syncthreads();
          for (int w = t; w < nown * parts; w += V) {
            const int part = w / nown, q = w - part * nown;
            const int kq = q / D, j = q - kq * D;
            const float ck = cc[(k0 + kq) * ld + j];
            const int v1 = (part + 1) * span < nv ? (part + 1) * span : nv;
            const float* pr = pt + kq * (V + 1);
            const float* dr = ddt + kq * (V + 1);
            float acc = 0.f;
            for (int v = part * span; v < v1; ++v) acc += pr[v] * dyt[v * D + j] - 2.f * (dr[v] * (xt[v * D + j] - ck));
            red[w] = acc;
          }
          __syncthreads();
          for (int q = t; q < nown; q += V) {
            float acc = 0.f;
            for (int part = 0; part < parts; ++part) acc += red[part * nown + q];
            vq_partial_put(mine + (size_t)s * LD, k0 * D + q, first, acc);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < DP; ++j) h[j] = h[j] + 2.f * dxr[j];    // h_s = h_{s+1} + u_s
    }
    if (live && dx != nullptr) vqb_store_row<T, DP>(dx + row, D, vec != 0, h);
    first = false;
  }
}

// the depth calls: G vectors per cell, depth [M / G]
static int vqres_depth_check(const char* who, int M, int G, const int32_t* depth) {
  JPDSE_REQUIRE(G >= 1, "%s: G = %d vectors per cell (at least 1)", who, G);
  JPDSE_REQUIRE(M % G == 0, "%s: G = %d does not divide M = %d", who, G, M);
  JPDSE_REQUIRE(depth != nullptr, "%s: null pointer (depth)", who);
  return JPDSE_OK;
}

// the backward entry points.  grouped: G is checked; dhist [n][G][L] or NULL: NULL is exactly jpdse_vq_res_bwd's launch.  deep: G is
// the cell size of depth [M / G] (no dhist)
static int vqres_bwd_run(const char* who, const jpdse_vq_res_bwd_args* a, int G, const float* dhist, bool grouped = false,
                         const int32_t* depth = nullptr, bool deep = false) {
  if (int rc = vq_res_check(who, a->dtype, a->M, a->D, a->L, a->S, a->n_stages, 1)) return rc;
  JPDSE_REQUIRE(isfinite(a->sigma) && a->sigma > 0.f, "%s: sigma is %g (a finite value > 0)", who, (double)a->sigma);
  if (deep)
    if (int rc = vqres_depth_check(who, a->M, G, depth)) return rc;
  if (grouped)                                   // after sigma, as ever: what it repeats of the check above has passed
    if (int rc = vq_res_grouped_check(who, a->dtype, a->M, a->D, a->L, a->S, a->n_stages, G)) return rc;
  JPDSE_REQUIRE(a->dy && a->x && a->books && a->index, "%s: null pointer", who);
  const int M = a->M, D = a->D, L = a->L, n = a->n_stages;
  const int V = vqb_bwd_threads(D), nb = vqres_bwd_blocks(M, D, L, n);
  float* partial = nullptr;
  if (a->dbooks != nullptr) {
    if (int rc = vq_ws_check(who, a->ws, a->ws_bytes, (size_t)nb * n * L * D * sizeof(float))) return rc;
    partial = mptr<float>(a->ws);
  }
  if (a->dx == nullptr && partial == nullptr) return JPDSE_OK;
  const int vec = vqb_vec(a->dtype, D, {a->x, a->dy, a->dx});
  // a stage's slice of dhist goes to LDS when the block's LDS stays below 64000 bytes with it (the rule of vqb_bwd_run,
  // vq_bottleneck.hip), otherwise it is read from global memory
  int gm = 0;
  if (dhist != nullptr) gm = vqres_bwd_lds(D, L, partial != nullptr, (size_t)G * (L + 1)) <= 64000 ? 1 : 2;
  const size_t lds = vqres_bwd_lds(D, L, partial != nullptr, gm == 1 ? (size_t)G * (L + 1) : 0);
  if (int rc = vqb_dispatch(a->dtype, D, L, [&](auto tag, auto dp, auto cbl) {
        using T = decltype(tag);
        constexpr int DPv = decltype(dp)::value;
        constexpr bool CBLv = decltype(cbl)::value;
        auto go = [&](auto kernel, auto dep) {
          return vq_launch(who, kernel, nb, V, lds, a->stream, cptr<T>(a->dy), cptr<T>(a->x), a->books, a->index, dhist, M, D, L, n, G,
                           a->sigma, vec, mptr<T>(a->dx), partial, dep);
        };
        if (deep) return go(vqres_bwd_kernel<T, DPv, CBLv, 0, true>, VqDepth<true>{depth, G});
        if (gm == 1) return go(vqres_bwd_kernel<T, DPv, CBLv, 1, false>, VqDepth<false>{});
        if (gm == 2) return go(vqres_bwd_kernel<T, DPv, CBLv, 2, false>, VqDepth<false>{});
        return go(vqres_bwd_kernel<T, DPv, CBLv, 0, false>, VqDepth<false>{});
      }))
    return rc;
  if (partial == nullptr) return JPDSE_OK;
  return vq_launch(who, vq_merge_kernel, ew_blocks(n * L * D), 256, 0, a->stream, partial, nb, n * L * D, 1.f, a->dbooks);
}

// jpdse_vq_res_rows_fwd and its depth form: the same grid, tile and LDS
static int vqres_rows_fwd_run(const char* who, const jpdse_vq_res_rows_fwd_args* a, int G, const int32_t* depth, bool deep) {
  if (int rc = vq_res_check(who, a->dtype, a->M, a->D, a->L, a->S, a->n_stages, 1)) return rc;
  if (deep)
    if (int rc = vqres_depth_check(who, a->M, G, depth)) return rc;
  JPDSE_REQUIRE(a->x && a->books && a->y && a->index, "%s: null pointer", who);
  const int M = a->M, D = a->D, L = a->L;
  const int vec = vqb_vec(a->dtype, D, {a->x, a->y});
  const size_t lds = vqb_cb_lds(D, L) ? (size_t)L * vqb_dp(D) * sizeof(float) : 0;
  return vqb_dispatch(a->dtype, D, L, [&](auto tag, auto dp, auto cbl) {
    using T = decltype(tag);
    auto go = [&](auto kernel, auto dep) {
      return vq_launch(who, kernel, vqb_blocks(M, 256), 256, lds, a->stream, cptr<T>(a->x), a->books, M, D, L, a->n_stages, vec,
                       mptr<T>(a->y), a->index, dep);
    };
    if (deep) return go(vqres_rows_fwd_kernel<T, decltype(dp)::value, decltype(cbl)::value, true>, VqDepth<true>{depth, G});
    return go(vqres_rows_fwd_kernel<T, decltype(dp)::value, decltype(cbl)::value, false>, VqDepth<false>{});
  });
}

static int vqres_decode_run(const char* who, const jpdse_vq_res_decode_args* a, int G, const int32_t* depth, bool deep) {
  if (int rc = vq_res_check(who, a->dtype, a->M, a->D, a->L, a->S, a->n_stages, 1)) return rc;
  if (deep)
    if (int rc = vqres_depth_check(who, a->M, G, depth)) return rc;
  JPDSE_REQUIRE(a->index && a->books && a->y && a->status, "%s: null pointer", who);
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    auto go = [&](auto kernel, auto dep) {
      return vq_launch(who, kernel, ew_blocks((long long)a->M * a->D), 256, 0, a->stream, a->index, a->books, a->M, a->D, a->L,
                       a->n_stages, mptr<T>(a->y), a->status, dep);
    };
    if (deep) return go(vqres_decode_kernel<T, true>, VqDepth<true>{depth, G});
    return go(vqres_decode_kernel<T, false>, VqDepth<false>{});
  });
}

// ---- the depth map -----------------------------------------------------------------------------------------------
// depth[n][cy][cx] = max over the step x step pixels of the cell of table[class], the class of a pixel by cost_class.h's rule (its
// label when that is an integer in [0, n_classes), NaN excluded); any other pixel takes def.  One thread per cell.
__global__ __launch_bounds__(256) void vqres_depth_map_kernel(const float* __restrict__ label, const int* __restrict__ table, int N, int H,
                                                             int W, int step, int n_classes, int def, int* __restrict__ depth) {
  const int h = H / step, w = W / step;
  const long long cells = (long long)N * h * w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long long)gridDim.x * 256) {
    const int cx = (int)(i % w), cy = (int)((i / w) % h), n = (int)(i / ((long long)w * h));
    const float* lab_n = label + (long long)n * H * W;
    int best = INT_MIN;
    for (int dy = 0; dy < step; ++dy)
      for (int dx = 0; dx < step; ++dx) {
        const float lab = lab_n[(long long)(cy * step + dy) * W + cx * step + dx];
        const int v = (lab >= 0.f && lab < (float)n_classes && lab == floorf(lab)) ? table[(int)lab] : def;
        best = v > best ? v : best;
      }
    depth[i] = best;
  }
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_res_workspace_size(int32_t M, int32_t D, int32_t L, int32_t S) {
  if (vq_res_check("vq_res_workspace_size", JPDSE_F32, M, D, L, S, S) != JPDSE_OK || S < 1) return 0;
  return vq_res_workspace_bytes(M, D, L, S);
}

int jpdse_vq_res_fwd(const jpdse_vq_res_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_fwd: null argument struct");
  if (int rc = vq_res_check("vq_res_fwd", a->dtype, a->M, a->D, a->L, a->S, a->n_stages)) return rc;
  JPDSE_REQUIRE(a->x && a->books && a->y && (a->index || a->n_stages == 0), "vq_res_fwd: null pointer");
  const int M = a->M, D = a->D, L = a->L, n = a->n_stages;
  const int nb = vqres_fwd_blocks(M);
  double* psse = nullptr;
  if (a->sse != nullptr && n > 0) {
    if (int rc = vq_ws_check("vq_res_fwd", a->ws, a->ws_bytes, (size_t)nb * n * sizeof(double))) return rc;
    JPDSE_REQUIRE(reinterpret_cast<uintptr_t>(a->ws) % 8 == 0, "vq_res_fwd: workspace not 8-byte aligned");
    psse = mptr<double>(a->ws);
  }
  const size_t lds = vqres_fwd_lds(D, L);
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        if (int rc = vq_lds_optin("vq_res_fwd", vqres_fwd_kernel<T>, lds)) return rc;
        return vq_launch("vq_res_fwd", vqres_fwd_kernel<T>, nb, 256, lds, a->stream, cptr<T>(a->x), a->books, M, D, L, n, vq_group(L),
                         mptr<T>(a->y), a->index, psse, a->residual);
      }))
    return rc;
  if (psse == nullptr) return JPDSE_OK;
  return vq_launch("vq_res_fwd(sse)", vqres_sse_kernel, 1, 64, 0, a->stream, psse, nb, n, a->sse);
}

int jpdse_vq_res_rows_fwd(const jpdse_vq_res_rows_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_rows_fwd: null argument struct");
  return vqres_rows_fwd_run("vq_res_rows_fwd", a, 1, nullptr, false);
}

int jpdse_vq_res_rows_fwd_depth(const jpdse_vq_res_rows_fwd_depth_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_rows_fwd_depth: null argument struct");
  return vqres_rows_fwd_run("vq_res_rows_fwd_depth", &a->fwd, a->G, a->depth, true);
}

int jpdse_vq_res_decode(const jpdse_vq_res_decode_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_decode: null argument struct");
  return vqres_decode_run("vq_res_decode", a, 1, nullptr, false);
}

int jpdse_vq_res_decode_depth(const jpdse_vq_res_decode_depth_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_decode_depth: null argument struct");
  return vqres_decode_run("vq_res_decode_depth", &a->dec, a->G, a->depth, true);
}

int jpdse_vq_res_bwd(const jpdse_vq_res_bwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_bwd: null argument struct");
  return vqres_bwd_run("vq_res_bwd", a, 1, nullptr);
}

int jpdse_vq_res_bwd_grouped(const jpdse_vq_res_bwd_grouped_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_bwd_grouped: null argument struct");
  return vqres_bwd_run("vq_res_bwd_grouped", &a->bwd, a->G, a->dhist, true);
}

int jpdse_vq_res_bwd_depth(const jpdse_vq_res_bwd_depth_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_res_bwd_depth: null argument struct");
  return vqres_bwd_run("vq_res_bwd_depth", &a->bwd, a->G, nullptr, false, a->depth, true);
}

int jpdse_vq_depth_map(const jpdse_vq_depth_map_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_depth_map: null argument struct");
  JPDSE_REQUIRE(a->N >= 1 && a->H >= 1 && a->W >= 1, "vq_depth_map: N, H, W = %d, %d, %d (at least 1 each)", a->N, a->H, a->W);
  JPDSE_REQUIRE(a->step >= 1 && a->H % a->step == 0 && a->W % a->step == 0, "vq_depth_map: step = %d does not divide H = %d and W = %d",
                a->step, a->H, a->W);
  JPDSE_REQUIRE((long long)a->N * a->H * a->W < (1LL << 31), "vq_depth_map: N * H * W = %lld (below 2^31)", (long long)a->N * a->H * a->W);
  JPDSE_REQUIRE(a->n_classes >= 0 && a->n_classes <= 65536, "vq_depth_map: n_classes = %d (0 .. 65536)", a->n_classes);
  JPDSE_REQUIRE(a->label && a->depth && (a->table || a->n_classes == 0), "vq_depth_map: null pointer");
  const long long cells = (long long)a->N * (a->H / a->step) * (a->W / a->step);
  return vq_launch("vq_depth_map", vqres_depth_map_kernel, ew_blocks(cells), 256, 0, a->stream, a->label, a->table, a->N, a->H, a->W,
                   a->step, a->n_classes, a->default_depth, a->depth);
}

}  // extern "C"
