// Soft-to-hard vector quantizer (ctu.quantizers.S2HVQ; reference ctu/quantizers/s2h_vq.py).
// Entry points: include/jpdse.h, "soft-to-hard vector quantizer"; definition: DESIGN.md 4.13.
//   M vectors x[m] of D components (fp32 or bf16), a code book c of L centres (fp32 [L][D]); arithmetic fp32
//   d[m][k] = sum_j (x[m][j] - c[k][j])^2, j ascending: the direct form, never |x|^2 - 2 x.c + |c|^2
// Kernels:
//   vq_soft_fwd_kernel / vq_hard_fwd_kernel / vq_argmax_kernel
//       a row of [M][L] belongs to a GROUP of G lanes of one wave, G = the power of two >= min(L, 64): lane kk of the group
//       owns the centres k = kk, kk + 64, ... (at most 8), a wave covers 64 / G consecutive vectors, so every wave-wide load or
//       store of p, dp or s is one contiguous run.  The code book is staged TRANSPOSED in LDS ([D][L]: the lanes of a group read
//       consecutive words, no bank conflict).  Row minimum, row sum and arg-min are xor butterflies inside the group.
//   vq_soft_bwd_kernel
//       a block walks tiles of V vectors: phase 1 (the group layout above) writes dd = -sigma p (dp - <p, dp>) of the tile to
//       LDS, phase 2a (one thread per (vector, component)) sums dx over k ascending, phase 2b (one thread per (centre,
//       component)) sums the tile's share of dC over the vectors ascending and adds it to the block's own fp32 partial.
//   vq_decode_kernel / vq_decode_bwd_kernel   gather of centres; its transpose with the same per-block partials
//   vq_pmf_partial_kernel / vq_pmf_bwd_kernel column means of [M][L], first stage, and their gradient
//   vq_core.h (shared with vq_bottleneck.hip and vq_fit.hip) the launcher, vq_weight, vq_partial_put, the group layout and its
//       score loop (VqLanes, vq_scores, vq_group_arg, vq_stage_transposed) and the two second stages: vq_merge_kernel
//       (out = scale * sum_b partial[b], b ascending, fp32) and vq_pmf_final_kernel (fp64)
// VqLanes states the group layout once (soft forward, the scores).  vq_hard_fwd_kernel, vq_argmax_kernel and vq_soft_bwd_kernel
// spell it out as before: with the struct the first two took one more VGPR and the third ran 5% slower in fp32.
// No atomics: every output element has one writer and every sum an order fixed by the grid, which depends on (M, D, L) alone,
// so two calls on the same buffers give identical bits.  LDS per block <= 64 KiB in every kernel.
#include <math.h>

#include "common.h"
#include "vq_core.h"

namespace jpdse {

constexpr int kVqPartialBlocks = 512;    // cap of the blocks (= fp32 partials) of the two code-book gradients
constexpr int kVqDecodeTile = 256;       // vectors per tile of vq_decode_bwd_kernel
constexpr int kVqPmfBlocks = 1024;       // cap of the blocks of vq_pmf_partial_kernel

// ---- launch geometry: functions of (M, D, L) alone, shared by the launchers and jpdse_vq_workspace_size -----------------
static inline int vq_bwd_tile(int L) {   // vectors per tile of vq_soft_bwd_kernel: dd tile [V][L + 1] of at most 24 KiB
  const int v = 6144 / (L + 1);
  return v > 64 ? 64 : v;
}
static inline int vq_bwd_blocks(int M, int L) {
  const int v = vq_bwd_tile(L);
  const int tiles = (M + v - 1) / v;
  return tiles < kVqPartialBlocks ? tiles : kVqPartialBlocks;
}
static inline int vq_decode_bwd_blocks(int M) {
  const int tiles = (M + kVqDecodeTile - 1) / kVqDecodeTile;
  return tiles < kVqPartialBlocks ? tiles : kVqPartialBlocks;
}
static inline int vq_pmf_rows(int L) { return L >= 256 ? 1 : 256 / L; }   // rows a block reads per pass
static inline int vq_pmf_blocks(int M, int L) {
  const long long per = 16LL * vq_pmf_rows(L);                            // at least 16 passes per block
  const long long b = (M + per - 1) / per;
  return b < 1 ? 1 : (b > kVqPmfBlocks ? kVqPmfBlocks : (int)b);
}
size_t vq_workspace_bytes(int M, int D, int L) {
  const size_t n = (size_t)L * D * sizeof(float);
  size_t need = (size_t)vq_bwd_blocks(M, L) * n;
  const size_t dec = (size_t)vq_decode_bwd_blocks(M) * n;
  const size_t pmf = (size_t)vq_pmf_blocks(M, L) * L * sizeof(float);
  if (dec > need) need = dec;
  if (pmf > need) need = pmf;
  return need;
}

// ---- device helpers ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vq_group_sum(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void vq_soft_fwd_kernel(const T* __restrict__ x, const float* __restrict__ c, int M, int D,
                                                         int L, int G, float sigma, float* __restrict__ p) {
  extern __shared__ float vq_lds[];
  vq_stage_transposed(c, vq_lds, D, L);
  __syncthreads();
  const VqLanes ln(G, L);
  for (long long base = ln.first(); base < M; base += ln.stride()) {
    const bool live = ln.live(base, M);
    const int m = ln.vector(base, M);
    float d[kVqSlots];
    vq_scores(x, vq_lds, m, D, ln, d);
    float dmin = INFINITY;
#pragma unroll
    for (int i = 0; i < kVqSlots; ++i)
      if (ln.slot_live(i)) dmin = fminf(dmin, d[i]);
    for (int off = G >> 1; off > 0; off >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, off, 64));
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kVqSlots; ++i) {
      d[i] = ln.slot_live(i) ? vq_weight(d[i], dmin, sigma) : 0.f;
      s += d[i];
    }
    s = vq_group_sum(s, G);
    if (live) {
      float* row = p + (size_t)m * L;
#pragma unroll
      for (int i = 0; i < kVqSlots; ++i)
        if (ln.slot_live(i)) row[ln.centre(i)] = d[i] / s;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vq_hard_fwd_kernel(const T* __restrict__ x, const float* __restrict__ c, int M, int D,
                                                         int L, int G, int* __restrict__ index, float* __restrict__ onehot) {
  extern __shared__ float vq_lds[];
  vq_stage_transposed(c, vq_lds, D, L);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = lane & (G - 1), g = lane / G, vpw = 64 / G, ni = (L + 63) >> 6;
  for (long long base = (long long)(blockIdx.x * 4 + wave) * vpw; base < M; base += (long long)gridDim.x * 4 * vpw) {
    const bool live = base + g < M;
    const int m = live ? (int)(base + g) : M - 1;
    float d[kVqSlots];
    vq_scores(x, vq_lds, m, D, VqLanes(G, L), d);
    float best = INFINITY;
    int bk = kk < L ? kk : 0x7fffffff;
    if (kk < L) best = d[0];
#pragma unroll
    for (int i = 1; i < kVqSlots; ++i)
      if (i < ni && kk + 64 * i < L && d[i] < best) {      // strict: the lower index keeps a tie
        best = d[i];
        bk = kk + 64 * i;
      }
    vq_group_arg<true>(best, bk, G);
    bk = __shfl(bk, lane & ~(G - 1), 64);                  // group lane 0 decides for the row
    bk = bk < L ? bk : L - 1;
    if (live) {
      if (kk == 0) index[m] = bk;
      if (onehot != nullptr) {
        float* row = onehot + (size_t)m * L;
#pragma unroll
        for (int i = 0; i < kVqSlots; ++i)
          if (i < ni && kk + 64 * i < L) row[kk + 64 * i] = kk + 64 * i == bk ? 1.f : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(256) void vq_argmax_kernel(const float* __restrict__ s, int M, int L, int G,
                                                       int* __restrict__ index) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = lane & (G - 1), g = lane / G, vpw = 64 / G, ni = (L + 63) >> 6;
  for (long long base = (long long)(blockIdx.x * 4 + wave) * vpw; base < M; base += (long long)gridDim.x * 4 * vpw) {
    const bool live = base + g < M;
    const int m = live ? (int)(base + g) : M - 1;
    const float* row = s + (size_t)m * L;
    float best = -INFINITY;
    int bk = kk < L ? kk : 0x7fffffff;
    if (kk < L) best = row[kk];
    for (int i = 1; i < ni; ++i) {
      const int k = kk + 64 * i;
      if (k < L) {
        const float v = row[k];
        if (v > best) {
          best = v;
          bk = k;
        }
      }
    }
    vq_group_arg<false>(best, bk, G);
    bk = bk < L ? bk : L - 1;
    if (live && kk == 0) index[m] = bk;
  }
}

// ---- backward of the soft assignment ---------------------------------------------------------------------------------------
// LDS: ddt [V][L + 1] | xt [V][D] | the code book [L][D] when c_lds.  partial: this block's [L][D] sums of dd (x - c), fp32,
// written (first tile) then added to by its single owner thread; nullptr: no code-book gradient.
template <typename T>
__global__ __launch_bounds__(256) void vq_soft_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ p,
                                                         const T* __restrict__ x, const float* __restrict__ c, int M, int D, int L,
                                                         int G, int V, int c_lds, float sigma, T* __restrict__ dx,
                                                         float* __restrict__ partial) {
  extern __shared__ float vq_lds[];
  const int ld = L + 1;
  float* ddt = vq_lds;
  float* xt = ddt + V * ld;
  const float* cc = c;
  if (c_lds) {
    float* cl = xt + V * D;
    for (int i = threadIdx.x; i < L * D; i += 256) cl[i] = c[i];
    cc = cl;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = lane & (G - 1), g = lane / G, vpw = 64 / G, ni = (L + 63) >> 6;
  const int ntiles = (M + V - 1) / V;
  float* mine = partial != nullptr ? partial + (size_t)blockIdx.x * L * D : nullptr;
  bool first = true;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    for (int i = threadIdx.x; i < nv * D; i += 256) xt[i] = ElemOps<T>::ld(x + (size_t)m0 * D + i);
    // phase 1: dd of the tile
    for (int vb = wave * vpw; vb < nv; vb += 4 * vpw) {
      const bool live = vb + g < nv;
      const int v = live ? vb + g : nv - 1;
      const size_t row = (size_t)(m0 + v) * L;
      float pv[kVqSlots], q[kVqSlots];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kVqSlots; ++i) {
        pv[i] = q[i] = 0.f;
        if (i < ni && kk + 64 * i < L) {
          pv[i] = p[row + kk + 64 * i];
          q[i] = dp[row + kk + 64 * i];
          s += pv[i] * q[i];
        }
      }
      s = vq_group_sum(s, G);
      if (live) {
#pragma unroll
        for (int i = 0; i < kVqSlots; ++i)
          if (i < ni && kk + 64 * i < L) ddt[v * ld + kk + 64 * i] = -sigma * (pv[i] * (q[i] - s));
      }
    }
    __syncthreads();
    // phase 2a: dx[m][j] = 2 sum_k dd[m][k] (x[m][j] - c[k][j]), k ascending
    if (dx != nullptr) {
      for (int i = threadIdx.x; i < nv * D; i += 256) {
        const int v = i / D, j = i - v * D;
        const float xv = xt[i];
        const float* dd = ddt + v * ld;
        float acc = 0.f;
        for (int k = 0; k < L; ++k) acc += dd[k] * (xv - cc[k * D + j]);
        ElemOps<T>::st(dx + (size_t)m0 * D + i, 2.f * acc);
      }
    }
    // phase 2b: the tile's share of sum_m dd[m][k] (x[m][j] - c[k][j]), m ascending
    if (mine != nullptr) {
      for (int q = threadIdx.x; q < L * D; q += 256) {
        const int k = q / D, j = q - k * D;
        const float ck = cc[q];
        float acc = 0.f;
        for (int v = 0; v < nv; ++v) acc += ddt[v * ld + k] * (xt[v * D + j] - ck);
        mine[q] = first ? acc : mine[q] + acc;
      }
    }
    first = false;
    __syncthreads();
  }
}

// ---- decode -----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void vq_decode_kernel(const int* __restrict__ index, const float* __restrict__ c, int M, int D,
                                                       int L, T* __restrict__ y, int* __restrict__ status) {
  const long long n = (long long)M * D;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / D), j = (int)(i - (long long)m * D);
    int k = index[m];
    if ((unsigned)k >= (unsigned)L) {
      k = 0;
      if (j == 0) *status = 1;           // every writer stores the same word
    }
    ElemOps<T>::st(y + i, c[k * D + j]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vq_decode_bwd_kernel(const int* __restrict__ index, const T* __restrict__ dy, int M, int D,
                                                           int L, float* __restrict__ partial, int* __restrict__ status) {
  __shared__ int it[kVqDecodeTile];
  const int ntiles = (M + kVqDecodeTile - 1) / kVqDecodeTile;
  float* mine = partial + (size_t)blockIdx.x * L * D;
  bool first = true;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * kVqDecodeTile;
    const int nv = M - m0 < kVqDecodeTile ? M - m0 : kVqDecodeTile;
    if ((int)threadIdx.x < nv) {
      int k = index[m0 + threadIdx.x];
      if ((unsigned)k >= (unsigned)L) {
        k = 0;
        *status = 1;
      }
      it[threadIdx.x] = k;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < L * D; q += 256) {
      const int k = q / D, j = q - k * D;
      float acc = 0.f;
      for (int v = 0; v < nv; ++v)
        if (it[v] == k) acc += ElemOps<T>::ld(dy + (size_t)(m0 + v) * D + j);
      vq_partial_put(mine, q, first, acc);
    }
    first = false;
    __syncthreads();
  }
}

// ---- pmf --------------------------------------------------------------------------------------------------------------------
// A block reads R = vq_pmf_rows(L) rows per pass: thread (r, k) sums its rows ascending, the R sums of a column are merged r
// ascending.  L > 256: R = 1 and a thread owns the columns k and k + 256.
__global__ __launch_bounds__(256) void vq_pmf_partial_kernel(const float* __restrict__ s, int M, int L, int R,
                                                            float* __restrict__ partial) {
  __shared__ float red[256];
  const int cols = L < 256 ? L : 256;
  const int r = threadIdx.x / cols, k = threadIdx.x - r * cols;
  for (int kb = 0; kb < L; kb += 256) {
    const int col = kb + k;
    float acc = 0.f;
    if (r < R && col < L)
      for (long long m = (long long)blockIdx.x * R + r; m < M; m += (long long)gridDim.x * R) acc += s[m * L + col];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (r == 0 && col < L) {
      for (int rr = 1; rr < R; ++rr) acc += red[rr * cols + k];
      partial[(size_t)blockIdx.x * L + col] = acc;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void vq_pmf_bwd_kernel(const float* __restrict__ dpmf, long long n, int L, float count,
                                                        float* __restrict__ ds) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    ds[i] = dpmf[(int)(i % L)] / count;
}

static inline int vq_row_blocks(int M, int G) { return ew_blocks((long long)M * G); }   // one lane per (row, group lane)

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_workspace_size(int32_t M, int32_t D, int32_t L) {
  if (vq_shape_check("vq_workspace_size", M, D, L) != JPDSE_OK) return 0;
  return vq_workspace_bytes(M, D, L);
}

int jpdse_vq_soft_fwd(const jpdse_vq_soft_fwd_args* a) {
  if (int rc = vq_soft_fwd_check(a)) return rc;
  const int G = vq_group(a->L);
  const size_t lds = (size_t)a->L * a->D * sizeof(float);
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    return vq_launch("vq_soft_fwd", vq_soft_fwd_kernel<T>, vq_row_blocks(a->M, G), 256, lds, a->stream, cptr<T>(a->x), a->code_book,
                     a->M, a->D, a->L, G, a->sigma, a->p);
  });
}

int jpdse_vq_hard_fwd(const jpdse_vq_hard_fwd_args* a) {
  if (int rc = vq_hard_fwd_check(a)) return rc;
  const int G = vq_group(a->L);
  const size_t lds = (size_t)a->L * a->D * sizeof(float);
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    return vq_launch("vq_hard_fwd", vq_hard_fwd_kernel<T>, vq_row_blocks(a->M, G), 256, lds, a->stream, cptr<T>(a->x), a->code_book,
                     a->M, a->D, a->L, G, a->index, a->onehot);
  });
}

int jpdse_vq_soft_bwd(const jpdse_vq_soft_bwd_args* a) {
  if (int rc = vq_soft_bwd_check(a)) return rc;
  if (a->dx == nullptr && a->dcode_book == nullptr) return JPDSE_OK;
  const int M = a->M, D = a->D, L = a->L;
  const int G = vq_group(L), V = vq_bwd_tile(L), nb = vq_bwd_blocks(M, L);
  const int c_lds = (size_t)L * D * sizeof(float) <= 32768 ? 1 : 0;
  const size_t lds = ((size_t)V * (L + 1) + (size_t)V * D + (c_lds ? (size_t)L * D : 0)) * sizeof(float);
  float* partial = a->dcode_book != nullptr ? mptr<float>(a->ws) : nullptr;
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        return vq_launch("vq_soft_bwd", vq_soft_bwd_kernel<T>, nb, 256, lds, a->stream, a->dp, a->p, cptr<T>(a->x), a->code_book, M, D,
                         L, G, V, c_lds, a->sigma, mptr<T>(a->dx), partial);
      }))
    return rc;
  if (partial == nullptr) return JPDSE_OK;
  return vq_launch("vq_soft_bwd(merge)", vq_merge_kernel, ew_blocks(L * D), 256, 0, a->stream, partial, nb, L * D, -2.f,
                   a->dcode_book);
}

int jpdse_vq_decode(const jpdse_vq_decode_args* a) {
  if (int rc = vq_decode_check(a)) return rc;
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    return vq_launch("vq_decode", vq_decode_kernel<T>, ew_blocks((long long)a->M * a->D), 256, 0, a->stream, a->index, a->code_book,
                     a->M, a->D, a->L, mptr<T>(a->y), a->status);
  });
}

int jpdse_vq_decode_bwd(const jpdse_vq_decode_bwd_args* a) {
  if (int rc = vq_decode_bwd_check(a)) return rc;
  const int nb = vq_decode_bwd_blocks(a->M), n = a->L * a->D;
  float* partial = mptr<float>(a->ws);
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        return vq_launch("vq_decode_bwd", vq_decode_bwd_kernel<T>, nb, 256, 0, a->stream, a->index, cptr<T>(a->dy), a->M, a->D, a->L,
                         partial, a->status);
      }))
    return rc;
  return vq_launch("vq_decode_bwd(merge)", vq_merge_kernel, ew_blocks(n), 256, 0, a->stream, partial, nb, n, 1.f, a->dcode_book);
}

int jpdse_vq_argmax(const jpdse_vq_argmax_args* a) {
  if (int rc = vq_argmax_check(a)) return rc;
  const int G = vq_group(a->L);
  return vq_launch("vq_argmax", vq_argmax_kernel, vq_row_blocks(a->M, G), 256, 0, a->stream, a->s, a->M, a->L, G, a->index);
}

int jpdse_vq_pmf(const jpdse_vq_pmf_args* a) {
  if (int rc = vq_pmf_check(a)) return rc;
  const int nb = vq_pmf_blocks(a->M, a->L);
  float* partial = mptr<float>(a->ws);
  if (int rc = vq_launch("vq_pmf", vq_pmf_partial_kernel, nb, 256, 0, a->stream, a->s, a->M, a->L, vq_pmf_rows(a->L), partial))
    return rc;
  return vq_launch("vq_pmf(final)", vq_pmf_final_kernel, 1, 256, 0, a->stream, partial, nb, a->L, (double)a->M, a->pmf);
}

int jpdse_vq_pmf_bwd(const jpdse_vq_pmf_bwd_args* a) {
  if (int rc = vq_pmf_bwd_check(a)) return rc;
  const long long n = (long long)a->M * a->L;
  return vq_launch("vq_pmf_bwd", vq_pmf_bwd_kernel, ew_blocks(n), 256, 0, a->stream, a->dpmf, n, a->L, (float)a->M, a->ds);
}

}  // extern "C"
