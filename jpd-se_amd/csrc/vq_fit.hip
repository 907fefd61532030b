// Code-book fit of the soft-to-hard vector quantizer: one Lloyd (k-means) iteration as a fused pass, with dead-centre reseeding.
// Entry points: include/jpdse.h, "code-book fit"; definitions, the determinism argument and measurements: DESIGN.md 4.21.
//   x [M][D] (fp32 or bf16), the code book c fp32 [L][D], arithmetic fp32, d[m][k] the direct score of vq.hip.
//   a(m) = the nearest centre of x[m], the lowest index on a tie: the score loop and butterfly of vq_hard_fwd_kernel (vq_core.h),
//   so the assignment is jpdse_vq_hard_fwd's index for index.
// Kernels:
//   vqf_accum_kernel     a block walks tiles of V vectors.  The tile's x goes to LDS once, as fp32 (the only read of x from HBM).
//       Assignment: the group layout of vq.hip reads the tile from LDS and leaves a(m) and d[m][a(m)] in LDS: the index never
//       leaves the block.  Gather: ONE THREAD PER CENTRE scans the tile's assignments in ascending order and adds the members'
//       components into registers (acc[D]), with the count, the sum of the distances and the farthest member (strictly greater
//       replaces: the earliest wins).  A scan step costs a compare; the D loads and adds are paid once per vector, by the one
//       lane whose centre it joined -- against L D per vector for the scan of vq_decode_bwd_kernel.  With L <= 128 the 256
//       threads split the tile into P = 4 or 2 parts of consecutive vectors, each with its own thread per centre; with L > 256
//       a thread owns the centres k and k + 256.  The sums stay in registers over all tiles of the block and are written once,
//       as the fp32 partial of the unit (block, part).  No atomics, LDS or global.
//   vqf_merge_kernel     second stage: the units are summed in ascending order in fp64, in 64 runs of consecutive units (a thread
//       each) that are then added in order, and the result initialises (first) or is added to the caller's running state.  The farthest member is
//       merged by (distance descending, m ascending): independent of the order.  far_vec is read from x at the winning m: at
//       most L rows.
//   vqf_update_kernel    one block: the means, the donor ranking (an O(L^2) count-rank) and the reseeding, in place in c.
//   vqf_transpose_kernel a code book of more than 32 KiB does not fit LDS beside the tile: the score loop then reads it
//       from a transposed copy [D][L] in the workspace (L2), with the same arithmetic.
// Every grid, tile and part is a function of (M, D, L) alone and every element has one writer: two calls on the same buffers give
// identical bits.  LDS per block: at most 51 KiB.
#include <math.h>

#include "common.h"
#include "vq_core.h"

namespace jpdse {

constexpr int kVqFitBlocks = 1024;       // cap of the blocks of vqf_accum_kernel
constexpr int kVqFitBookWords = 8192;    // a code book up to this many words (32 KiB) is staged in LDS

// ---- launch geometry: functions of (M, D, L) alone --------------------------------------------------------------------------
static inline int vqf_dp(int D) { return D <= 4 ? 4 : (D <= 8 ? 8 : (D <= 16 ? 16 : 32)); }
static inline int vqf_tile(int D) { return D <= 16 ? 256 : 128; }                 // vectors per tile
static inline bool vqf_book_lds(int D, int L) { return L * D <= kVqFitBookWords; }
static inline int vqf_parts(int L) { return L <= 64 ? 4 : (L <= 128 ? 2 : 1); }   // gather parts of a tile
static inline int vqf_blocks(int M, int D) {
  const int v = vqf_tile(D);
  const int tiles = (M + v - 1) / v;
  return tiles < kVqFitBlocks ? tiles : kVqFitBlocks;
}
// the workspace: ct [D][L] | per unit u = block * parts + part: sum [L][D] fp32 | count [L] int32 | sse [L] fp32 | far distance
// [L] fp32 | far m [L] int32
struct VqfWs {
  int units;
  size_t sum, cnt, sse, fd, fm, bytes;
};
static inline VqfWs vqf_ws(int M, int D, int L) {
  VqfWs w;
  w.units = vqf_blocks(M, D) * vqf_parts(L);
  const size_t per = (size_t)w.units * L * 4;
  w.sum = align_up((size_t)L * D * 4, 256);
  w.cnt = w.sum + per * D;
  w.sse = w.cnt + per;
  w.fd = w.sse + per;
  w.fm = w.fd + per;
  w.bytes = w.fm + per;
  return w;
}
size_t vq_lloyd_workspace_bytes(int M, int D, int L) { return vqf_ws(M, D, L).bytes; }

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vqf_transpose_kernel(const float* __restrict__ c, int D, int L, float* __restrict__ ct) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < L * D; i += gridDim.x * 256) {
    const int k = i / D, j = i - k * D;
    ct[j * L + k] = c[i];
  }
}

// LDS: ct [D][L] when CBL | xt [V][D] | it [V] | dt [V].  c: the code book [L][D] (CBL) or its transposed copy [D][L].
// Thread roles of the gather: P parts of V / P consecutive vectors; inside a part the 4 / P waves cover the centres
// (wave % (4 / P)) * 64 + lane (+ 256 for the second slot).
template <typename T, int DP, bool CBL>
__global__ __launch_bounds__(256) void vqf_accum_kernel(const T* __restrict__ x, const float* __restrict__ c, int M, int D, int L,
                                                       int G, int V, int P, float* __restrict__ psum, int* __restrict__ pcnt,
                                                       float* __restrict__ psse, float* __restrict__ pfd, int* __restrict__ pfm) {
  extern __shared__ float vqf_lds[];
  float* xt = vqf_lds + (CBL ? L * D : 0);
  int* it = reinterpret_cast<int*>(xt + V * D);
  float* dt = reinterpret_cast<float*>(it + V);
  const float* book = c;
  if constexpr (CBL) {
    vq_stage_transposed(c, vqf_lds, D, L);      // the first tile's barrier orders it before the scores
    book = vqf_lds;
  }
  const VqLanes ln(G, L);
  const int lane = ln.lane, wave = ln.wave, kk = ln.kk, ni = ln.ni;
  const int wp = 4 / P, part = wave / wp, span = V / P;
  const int kbase = (wave % wp) * 64 + lane;
  float acc[2][DP], sse[2], fd[2];
  int cnt[2], fm[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int j = 0; j < DP; ++j) acc[s][j] = 0.f;
    sse[s] = 0.f;
    fd[s] = -1.f;
    cnt[s] = 0;
    fm[s] = 0x7fffffff;
  }
  const int ntiles = (M + V - 1) / V;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * V;
    const int nv = M - m0 < V ? M - m0 : V;
    for (int i = threadIdx.x; i < nv * D; i += 256) xt[i] = ElemOps<T>::ld(x + (size_t)m0 * D + i);
    __syncthreads();
    // assignment: vq_hard_fwd_kernel's, on the tile in LDS
    for (int vb = wave * ln.vpw; vb < nv; vb += 4 * ln.vpw) {
      const bool live = vb + ln.g < nv;
      const int v = live ? vb + ln.g : nv - 1;
      float d[kVqSlots];
      vq_scores(xt, book, v, D, ln, d);
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
      best = __shfl(best, lane & ~(G - 1), 64);
      bk = bk < L ? bk : L - 1;
      if (live && kk == 0) {
        it[v] = bk;
        dt[v] = best;
      }
    }
    __syncthreads();
    // gather: this thread's centres against its part of the tile, vectors ascending
    const int v0 = part * span;
    const int v1 = nv < v0 + span ? nv : v0 + span;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int k = kbase + 256 * s;
      if ((wave % wp) * 64 + 256 * s < L) {                  // a wave without a centre skips the scan
        for (int v = v0; v < v1; ++v) {
          if (it[v] == k) {
            const float dv = dt[v];
            const float* xr = xt + v * D;
            ++cnt[s];
            sse[s] += dv;
            if (dv > fd[s]) {                                // strict: the earliest of equal distances stays
              fd[s] = dv;
              fm[s] = m0 + v;
            }
#pragma unroll
            for (int j = 0; j < DP; ++j)
              if (j < D) acc[s][j] += xr[j];
          }
        }
      }
    }
    __syncthreads();
  }
  const size_t u = (size_t)blockIdx.x * P + part;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = kbase + 256 * s;
    if (k < L) {
      float* ps = psum + (u * L + k) * D;
#pragma unroll
      for (int j = 0; j < DP; ++j)
        if (j < D) ps[j] = acc[s][j];
      pcnt[u * L + k] = cnt[s];
      psse[u * L + k] = sse[s];
      pfd[u * L + k] = fd[s];
      pfm[u * L + k] = fm[s];
    }
  }
}

// blocks [0, nA): kVqFitMergeEl elements of sums each; blocks [nA, ..): as many centres each.  Thread (el, ch) takes the units
// [ch cs, (ch + 1) cs), cs = ceil(nu / kVqFitMergeCh), ascending; the threads of run 0 add the runs in order and update the state.
constexpr int kVqFitMergeEl = 16, kVqFitMergeCh = 64;      // 1024 threads
template <typename T>
__global__ __launch_bounds__(1024) void vqf_merge_kernel(const T* __restrict__ x, const float* __restrict__ psum,
                                                        const int* __restrict__ pcnt, const float* __restrict__ psse,
                                                        const float* __restrict__ pfd, const int* __restrict__ pfm, int nu, int M,
                                                        int D, int L, int nA, int first, long long* __restrict__ counts,
                                                        double* __restrict__ sums, double* __restrict__ sse,
                                                        float* __restrict__ far_dist, float* __restrict__ far_vec) {
  __shared__ double red[kVqFitMergeCh][kVqFitMergeEl];
  __shared__ long long redc[kVqFitMergeCh][kVqFitMergeEl];
  __shared__ float redd[kVqFitMergeCh][kVqFitMergeEl];
  __shared__ int redm[kVqFitMergeCh][kVqFitMergeEl];
  const int el = threadIdx.x & (kVqFitMergeEl - 1), ch = threadIdx.x / kVqFitMergeEl;
  const int cs = (nu + kVqFitMergeCh - 1) / kVqFitMergeCh;
  const int u0 = ch * cs;
  const int u1 = nu < u0 + cs ? nu : u0 + cs;
  if ((int)blockIdx.x < nA) {
    const int n = L * D, e = blockIdx.x * kVqFitMergeEl + el;
    double a = 0.0;
    if (e < n) {
#pragma unroll 8
      for (int u = u0; u < u1; ++u) a += (double)psum[(size_t)u * n + e];
    }
    red[ch][el] = a;
    __syncthreads();
    if (ch == 0 && e < n) {
      double tot = red[0][el];
      for (int w = 1; w < kVqFitMergeCh; ++w) tot += red[w][el];
      sums[e] = first ? tot : sums[e] + tot;
    }
    return;
  }
  const int k = ((int)blockIdx.x - nA) * kVqFitMergeEl + el;
  double a = 0.0;
  long long n = 0;
  float bd = -1.f;
  int bm = 0x7fffffff;
  if (k < L) {
#pragma unroll 4
    for (int u = u0; u < u1; ++u) {
      const size_t i = (size_t)u * L + k;
      n += pcnt[i];
      a += (double)psse[i];
      const float d = pfd[i];
      const int m = pfm[i];
      if (d > bd || (d == bd && m < bm)) {
        bd = d;
        bm = m;
      }
    }
  }
  red[ch][el] = a;
  redc[ch][el] = n;
  redd[ch][el] = bd;
  redm[ch][el] = bm;
  __syncthreads();
  if (ch != 0 || k >= L) return;
  for (int w = 1; w < kVqFitMergeCh; ++w) {
    a += red[w][el];
    n += redc[w][el];
    const float d = redd[w][el];
    const int m = redm[w][el];
    if (d > bd || (d == bd && m < bm)) {
      bd = d;
      bm = m;
    }
  }
  const bool member = bd >= 0.f && (unsigned)bm < (unsigned)M;
  float* fv = far_vec + (size_t)k * D;
  if (first) {
    counts[k] = n;
    sse[k] = a;
    far_dist[k] = member ? bd : -1.f;
    for (int j = 0; j < D; ++j) fv[j] = member ? ElemOps<T>::ld(x + (size_t)bm * D + j) : 0.f;
  } else {
    counts[k] += n;
    sse[k] += a;
    if (member && bd > far_dist[k]) {                        // strict: an earlier call keeps an equal distance
      far_dist[k] = bd;
      for (int j = 0; j < D; ++j) fv[j] = ElemOps<T>::ld(x + (size_t)bm * D + j);
    }
  }
}

// One block.  Live centres take their mean; with reseed, the i-th dead centre (k ascending) takes far_vec of the i-th donor
// (n >= 2, far_dist > 0; ranked by sse descending, the lower k first on equal sse) while donors last.  Row k of c is written
// by the owner of k alone, from the state alone.
__global__ __launch_bounds__(256) void vqf_update_kernel(float* __restrict__ c, const long long* __restrict__ counts,
                                                        const double* __restrict__ sums, const double* __restrict__ sse,
                                                        const float* __restrict__ far_dist, const float* __restrict__ far_vec,
                                                        int D, int L, int reseed, int* __restrict__ report) {
  __shared__ double e[512];
  __shared__ int by_rank[512];
  __shared__ unsigned char dead[512], donor[512];
  for (int k = threadIdx.x; k < L; k += 256) {
    const long long n = counts[k];
    dead[k] = n == 0;
    donor[k] = n >= 2 && far_dist[k] > 0.f;
    e[k] = sse[k];
    by_rank[k] = -1;
  }
  __syncthreads();
  int n_dead = 0, n_donor = 0;
  for (int q = 0; q < L; ++q) {
    n_dead += dead[q];
    n_donor += donor[q];
  }
  for (int k = threadIdx.x; k < L; k += 256)
    if (donor[k]) {
      const double ek = e[k];
      int r = 0;
      for (int q = 0; q < L; ++q)
        if (donor[q] && (e[q] > ek || (e[q] == ek && q < k))) ++r;
      by_rank[r] = k;
    }
  __syncthreads();
  for (int k = threadIdx.x; k < L; k += 256) {
    float* ck = c + (size_t)k * D;
    if (!dead[k]) {
      const double n = (double)counts[k];
      for (int j = 0; j < D; ++j) ck[j] = (float)(sums[(size_t)k * D + j] / n);
    } else if (reseed) {
      int i = 0;
      for (int q = 0; q < k; ++q) i += dead[q];
      const int src = i < n_donor ? by_rank[i] : -1;
      if (src >= 0)
        for (int j = 0; j < D; ++j) ck[j] = far_vec[(size_t)src * D + j];
    }
  }
  if (threadIdx.x == 0) {
    report[0] = n_dead;
    report[1] = reseed ? (n_dead < n_donor ? n_dead : n_donor) : 0;
  }
}

template <typename T, int DP>
static int vqf_accum_launch(const jpdse_vq_lloyd_accum_args* a, bool cbl, const float* book, int nb, int G, int V, int P, size_t lds,
                            float* psum, int* pcnt, float* psse, float* pfd, int* pfm) {
  if (cbl)
    return vq_launch("vq_lloyd_accum", vqf_accum_kernel<T, DP, true>, nb, 256, lds, a->stream, cptr<T>(a->x), book, a->M, a->D, a->L,
                     G, V, P, psum, pcnt, psse, pfd, pfm);
  return vq_launch("vq_lloyd_accum", vqf_accum_kernel<T, DP, false>, nb, 256, lds, a->stream, cptr<T>(a->x), book, a->M, a->D, a->L, G,
                   V, P, psum, pcnt, psse, pfd, pfm);
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_lloyd_workspace_size(int32_t M, int32_t D, int32_t L) {
  if (vq_shape_check("vq_lloyd_workspace_size", M, D, L) != JPDSE_OK) return 0;
  return vq_lloyd_workspace_bytes(M, D, L);
}

int jpdse_vq_lloyd_accum(const jpdse_vq_lloyd_accum_args* a) {
  if (int rc = vq_lloyd_accum_check(a)) return rc;
  const int M = a->M, D = a->D, L = a->L;
  const VqfWs w = vqf_ws(M, D, L);
  const int G = vq_group(L), V = vqf_tile(D), P = vqf_parts(L), nb = vqf_blocks(M, D), dp = vqf_dp(D);
  const bool cbl = vqf_book_lds(D, L);
  char* base = mptr<char>(a->ws);
  float* ct = reinterpret_cast<float*>(base);
  float* psum = reinterpret_cast<float*>(base + w.sum);
  int* pcnt = reinterpret_cast<int*>(base + w.cnt);
  float* psse = reinterpret_cast<float*>(base + w.sse);
  float* pfd = reinterpret_cast<float*>(base + w.fd);
  int* pfm = reinterpret_cast<int*>(base + w.fm);
  if (!cbl)
    if (int rc = vq_launch("vq_lloyd_accum(transpose)", vqf_transpose_kernel, ew_blocks(L * D), 256, 0, a->stream, a->code_book, D, L,
                           ct))
      return rc;
  const float* book = cbl ? a->code_book : ct;
  const size_t lds = ((size_t)(cbl ? L * D : 0) + (size_t)V * D + 2 * (size_t)V) * sizeof(float);
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        switch (dp) {
          case 4: return vqf_accum_launch<T, 4>(a, cbl, book, nb, G, V, P, lds, psum, pcnt, psse, pfd, pfm);
          case 8: return vqf_accum_launch<T, 8>(a, cbl, book, nb, G, V, P, lds, psum, pcnt, psse, pfd, pfm);
          case 16: return vqf_accum_launch<T, 16>(a, cbl, book, nb, G, V, P, lds, psum, pcnt, psse, pfd, pfm);
          default: return vqf_accum_launch<T, 32>(a, cbl, book, nb, G, V, P, lds, psum, pcnt, psse, pfd, pfm);
        }
      }))
    return rc;
  const int nA = (L * D + kVqFitMergeEl - 1) / kVqFitMergeEl, nB = (L + kVqFitMergeEl - 1) / kVqFitMergeEl;
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    return vq_launch("vq_lloyd_accum(merge)", vqf_merge_kernel<T>, nA + nB, kVqFitMergeEl * kVqFitMergeCh, 0, a->stream, cptr<T>(a->x), psum, pcnt, psse, pfd, pfm,
                     w.units, M, D, L, nA, a->first ? 1 : 0, reinterpret_cast<long long*>(a->counts), a->sums, a->sse, a->far_dist,
                     a->far_vec);
  });
}

int jpdse_vq_lloyd_update(const jpdse_vq_lloyd_update_args* a) {
  if (int rc = vq_lloyd_update_check(a)) return rc;
  return vq_launch("vq_lloyd_update", vqf_update_kernel, 1, 256, 0, a->stream, a->code_book, reinterpret_cast<const long long*>(a->counts),
                   a->sums, a->sse, a->far_dist, a->far_vec, a->D, a->L, a->reseed ? 1 : 0, a->report);
}

}  // extern "C"
