// InstanceNorm2d(affine=False) fused with ReLU / LeakyReLU / residual add, forward and
// backward, NHWC (reference: networks.py:31 and the activation sites listed in jpdse.h).  HBM-bound.
//
// Forms, chosen per call by the host layer at the end of this file:
//   * two register-held kernels (the shipped default; any tensor with <= 64 pixel splits per image, everything up to 67 MB in
//     the bench step): a block keeps its pixels in registers, PHASE 1 writes a row of partial sums per block, PHASE 2 sums its
//     group's rows in its prologue and applies;
//   * three kernels (larger tensors; developer mode 27 everywhere): (1) a moment kernel in which each thread owns one 16-byte
//     channel vector column and walks pixels (coalesced: a pixel's channels are contiguous), partial sums per pixel split
//     written to the workspace; (2) a tiny finalize kernel (deterministic order, no atomics); (3) a fully parallel apply kernel;
//   * statistics from the slots a conv epilogue wrote (jpdse_inorm_fwd_from_moments / _bwd_from_sums): one register-held
//     kernel that merges the slots itself (PHASE 3), or a slot finalize kernel + the apply kernel of the three-kernel form.
#include "common.h"

namespace jpdse {

struct MomentGeom {
  int N, HW, Cs, cv;      // cv = Cs / VE vector columns
  int TX, TY;             // threads across columns / pixels (TX*TY = 256), TX a power of two
  int tx_shift;           // log2(TX)
  int splits, pix_per_split;
  int alias;              // backward: images >= alias read the saved x / stats of image n - alias (0 = off)
};

static MomentGeom moment_geom(int N, int HW, int Cs, int VE) {
  MomentGeom g;
  g.N = N; g.HW = HW; g.Cs = Cs; g.cv = Cs / VE; g.alias = 0;
  int tx = 1;
  while (tx < g.cv && tx < 256) tx <<= 1;
  g.TX = tx; g.TY = 256 / tx;
  g.tx_shift = 0;
  while ((1 << g.tx_shift) < tx) ++g.tx_shift;
  // aim for ~2048 blocks in total, at least 8 pixels per thread row
  const int col_blocks = (g.cv + g.TX - 1) / g.TX;
  long long want = 2048 / ((long long)N * col_blocks);
  if (want < 1) want = 1;
  long long max_splits = HW / ((long long)g.TY * 8);
  if (max_splits < 1) max_splits = 1;
  if (want > max_splits) want = max_splits;
  if (want > 256) want = 256;
  g.splits = (int)want;
  g.pix_per_split = (HW + g.splits - 1) / g.splits;
  g.splits = (HW + g.pix_per_split - 1) / g.pix_per_split;
  return g;
}

#ifndef JPDSE_NORM_ILP
#define JPDSE_NORM_ILP 2      // pixels per thread and loop trip of the streaming norm kernels (bytes in flight; A/B with -DJPDSE_NORM_ILP=1)
#endif

// ---- per-element functors -----------------------------------------------------------------
// forward moments: (x - shift), (x - shift)^2 with shift = x[n, pixel 0, c]
template <typename T> struct FwdMoments {
  const T* x;
  __device__ __forceinline__ void prep(int n, int HW, int Cs, int c0, float (&aux)[8]) const {
    float v[Vec16<T>::N];
    Vec16<T>::load(x + (long long)n * HW * Cs + c0, v);
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) aux[e] = v[e];
  }
  __device__ __forceinline__ void acc(const float (&v)[Vec16<T>::N], const float (&aux)[8], float (&s1)[8], float (&s2)[8]) const {
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) {
      const float d = v[e] - aux[e];
      s1[e] += d;
      s2[e] += d * d;
    }
  }
  __device__ __forceinline__ void at(long long off, const float (&aux)[8], float (&s1)[8], float (&s2)[8]) const {
    float v[Vec16<T>::N];
    Vec16<T>::load(x + off, v);
    acc(v, aux, s1, s2);
  }
};

__device__ __forceinline__ float act_grad(float yhat, int act, float slope) {
  if (act == JPDSE_ACT_RELU) return yhat > 0.f ? 1.f : 0.f;
  if (act == JPDSE_ACT_LRELU) return yhat > 0.f ? 1.f : slope;
  return 1.f;
}

// backward moments: dz, dz*yhat with dz = dy*act'(yhat), yhat = (x-mean)*rstd
template <typename T> struct BwdMoments {
  const T* x;
  const T* dy;
  const float* stats;  // [N][Cs][2]
  int act;
  float slope;
  __device__ __forceinline__ void acc2(const float (&v)[Vec16<T>::N], const float (&g)[Vec16<T>::N], const float (&mean)[Vec16<T>::N],
                                       const float (&rstd)[Vec16<T>::N], float (&s1)[8], float (&s2)[8]) const {
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) {
      const float yh = (v[e] - mean[e]) * rstd[e];
      const float dz = g[e] * act_grad(yh, act, slope);
      s1[e] += dz;
      s2[e] += dz * yh;
    }
  }
};

// partial[n][split][c][2]
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void moment_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                    const float* __restrict__ stats, int act, float slope,
                                                    float* __restrict__ partial, MomentGeom g) {
  constexpr int VE = Vec16<T>::N;
  __shared__ float red[256 * 2 * VE];
  const int tx = threadIdx.x & (g.TX - 1), ty = threadIdx.x >> g.tx_shift;
  const int col_blocks = (g.cv + g.TX - 1) / g.TX;
  const int cb = blockIdx.x % col_blocks;
  const int split = (blockIdx.x / col_blocks) % g.splits;
  const int n = blockIdx.x / (col_blocks * g.splits);
  const int col = cb * g.TX + tx;
  const bool on = col < g.cv;
  const int c0 = col * VE;
  float s1[8], s2[8], aux[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; aux[e] = 0.f; }
  if (on) {
    const int p0 = split * g.pix_per_split;
    int p1 = p0 + g.pix_per_split;
    p1 = p1 < g.HW ? p1 : g.HW;
    const long long base = (long long)n * g.HW * g.Cs + c0;
    if (!BWD) {
      FwdMoments<T> f{x};
      f.prep(n, g.HW, g.Cs, c0, aux);
      // JPDSE_NORM_ILP pixels per trip, all loads issued before the first use (same summation order: p ascending)
      int p = p0 + ty;
      for (; p + (JPDSE_NORM_ILP - 1) * g.TY < p1; p += JPDSE_NORM_ILP * g.TY) {
        float v[JPDSE_NORM_ILP][VE];
#pragma unroll
        for (int u = 0; u < JPDSE_NORM_ILP; ++u) Vec16<T>::load(x + base + (long long)(p + u * g.TY) * g.Cs, v[u]);
#pragma unroll
        for (int u = 0; u < JPDSE_NORM_ILP; ++u) f.acc(v[u], aux, s1, s2);
      }
      for (; p < p1; p += g.TY) f.at(base + (long long)p * g.Cs, aux, s1, s2);
    } else {
      BwdMoments<T> f{x, dy, stats, act, slope};
      float mean[VE], rstd[VE];
      const int nx = n >= g.alias ? n - g.alias : n;      // the saved forward image of gradient image n
      const long long xbase = (long long)nx * g.HW * g.Cs + c0;
      {
        const float* st = stats + ((long long)nx * g.Cs + c0) * 2;
#pragma unroll
        for (int e = 0; e < VE; ++e) { mean[e] = st[2 * e]; rstd[e] = st[2 * e + 1]; }
      }
      int p = p0 + ty;
      for (; p + (JPDSE_NORM_ILP - 1) * g.TY < p1; p += JPDSE_NORM_ILP * g.TY) {
        float v[JPDSE_NORM_ILP][VE], gr[JPDSE_NORM_ILP][VE];
#pragma unroll
        for (int u = 0; u < JPDSE_NORM_ILP; ++u) {
          const long long po = (long long)(p + u * g.TY) * g.Cs;
          Vec16<T>::load(x + xbase + po, v[u]);
          Vec16<T>::load(dy + base + po, gr[u]);
        }
#pragma unroll
        for (int u = 0; u < JPDSE_NORM_ILP; ++u) f.acc2(v[u], gr[u], mean, rstd, s1, s2);
      }
      for (; p < p1; p += g.TY) {
        float v[VE], gr[VE];
        Vec16<T>::load(x + xbase + (long long)p * g.Cs, v);
        Vec16<T>::load(dy + base + (long long)p * g.Cs, gr);
        f.acc2(v, gr, mean, rstd, s1, s2);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    red[(threadIdx.x * VE + e) * 2] = s1[e];
    red[(threadIdx.x * VE + e) * 2 + 1] = s2[e];
  }
  __syncthreads();
  if (ty == 0 && on) {
    float* out = partial + (((long long)n * g.splits + split) * g.Cs + c0) * 2;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      float a = 0.f, b = 0.f;
      for (int y = 0; y < g.TY; ++y) {
        a += red[((y * g.TX + tx) * VE + e) * 2];
        b += red[((y * g.TX + tx) * VE + e) * 2 + 1];
      }
      out[2 * e] = a;
      out[2 * e + 1] = b;
    }
  }
}

// Finalize kernels: 8 lanes cooperate on one (n,c) (strided over the pixel splits, then a
// shuffle reduction) -- a serial loop per thread was latency-bound (~40 us for 256 splits).
__device__ __forceinline__ void reduce_splits(const float* __restrict__ partial, int n, int c, int Cs, int splits,
                                              int sub, float& a, float& b) {
  a = 0.f;
  b = 0.f;
  // four partials per trip, loaded before any is added: the serial form (one L2 round trip per split) made these
  // tiny kernels ~8 us each, 72 of them per step
  const long long stride = (long long)Cs * 2;
  const float* p = partial + (((long long)n * splits + sub) * Cs + c) * 2;
  int s = sub;
  for (; s + 24 < splits; s += 32, p += 32 * stride) {
    const float2 v0 = *reinterpret_cast<const float2*>(p);
    const float2 v1 = *reinterpret_cast<const float2*>(p + 8 * stride);
    const float2 v2 = *reinterpret_cast<const float2*>(p + 16 * stride);
    const float2 v3 = *reinterpret_cast<const float2*>(p + 24 * stride);
    a += v0.x; b += v0.y;
    a += v1.x; b += v1.y;
    a += v2.x; b += v2.y;
    a += v3.x; b += v3.y;
  }
  for (; s < splits; s += 8, p += 8 * stride) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    a += v.x;
    b += v.y;
  }
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
}

// forward finalize: partial sums of shifted values -> (mean, rstd)
template <typename T>
__global__ void finalize_fwd_kernel(const T* __restrict__ x, const float* __restrict__ partial,
                                    float* __restrict__ stats, int N, int HW, int Cs, int splits, float eps) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int idx = gid >> 3, sub = gid & 7;
  const bool on = idx < N * Cs;
  const int n = on ? idx / Cs : 0, c = on ? idx % Cs : 0;
  float a, b;
  reduce_splits(partial, n, c, Cs, on ? splits : 0, sub, a, b);
  if (!on || sub != 0) return;
  const float shift = ElemOps<T>::ld(x + (long long)n * HW * Cs + c);
  const float inv = 1.f / (float)HW;
  const float dm = a * inv;
  float var = b * inv - dm * dm;
  var = var > 0.f ? var : 0.f;
  stats[2 * idx] = shift + dm;
  stats[2 * idx + 1] = rsqrtf(var + eps);
}

// backward finalize: (mean(dz), mean(dz*yhat))
__global__ void finalize_bwd_kernel(const float* __restrict__ partial, float* __restrict__ sums, int N, int HW,
                                    int Cs, int splits) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int idx = gid >> 3, sub = gid & 7;
  const bool on = idx < N * Cs;
  const int n = on ? idx / Cs : 0, c = on ? idx % Cs : 0;
  float a, b;
  reduce_splits(partial, n, c, Cs, on ? splits : 0, sub, a, b);
  if (!on || sub != 0) return;
  const float inv = 1.f / (float)HW;
  sums[2 * idx] = a * inv;
  sums[2 * idx + 1] = b * inv;
}

// y = act((x - mean) * rstd): the forward's per-element expression (the residual is added by the caller)
__device__ __forceinline__ float norm_act(float x, float mean, float rstd, int act, float slope) {
  float t = (x - mean) * rstd;
  if (act == JPDSE_ACT_RELU) t = t > 0.f ? t : 0.f;
  else if (act == JPDSE_ACT_LRELU) t = t > 0.f ? t : t * slope;
  return t;
}

// Apply kernels: same block decomposition as the moment kernel (one 16-byte channel-vector column per
// lane, pixels walked with stride TY), so the per-channel constants are loaded once per thread and the
// inner loop has no integer division; coalescing is along the contiguous channel axis.
template <typename T>
__global__ __launch_bounds__(256) void inorm_apply_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                            T* __restrict__ y, const float* __restrict__ stats,
                                                            int act, float slope, MomentGeom g) {
  constexpr int VE = Vec16<T>::N;
  const int tx = threadIdx.x & (g.TX - 1), ty = threadIdx.x >> g.tx_shift;
  const int col_blocks = (g.cv + g.TX - 1) / g.TX;
  const int cb = blockIdx.x % col_blocks;
  const int split = (blockIdx.x / col_blocks) % g.splits;
  const int n = blockIdx.x / (col_blocks * g.splits);
  const int col = cb * g.TX + tx;
  if (col >= g.cv) return;
  const int c0 = col * VE;
  float mean[VE], rstd[VE];
  const float* st = stats + ((long long)n * g.Cs + c0) * 2;
#pragma unroll
  for (int e = 0; e < VE; ++e) { mean[e] = st[2 * e]; rstd[e] = st[2 * e + 1]; }
  const int p0 = split * g.pix_per_split;
  int p1 = p0 + g.pix_per_split;
  p1 = p1 < g.HW ? p1 : g.HW;
  const long long base = (long long)n * g.HW * g.Cs + c0;
  // JPDSE_NORM_ILP pixels per trip: their loads are issued before the first store
  for (int p = p0 + ty; p < p1; p += JPDSE_NORM_ILP * g.TY) {
    float v[JPDSE_NORM_ILP][VE], r[JPDSE_NORM_ILP][VE];
#pragma unroll
    for (int u = 0; u < JPDSE_NORM_ILP; ++u) {
      const int pu = p + u * g.TY;
      if (pu < p1) {
        const long long off = base + (long long)pu * g.Cs;
        JPDSE_LOAD_LAST(T, x + off, v[u]);
        if (res != nullptr) Vec16<T>::load(res + off, r[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < JPDSE_NORM_ILP; ++u) {
      const int pu = p + u * g.TY;
      if (pu >= p1) break;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        float t = norm_act(v[u][e], mean[e], rstd[e], act, slope);
        if (res != nullptr) t += r[u][e];
        v[u][e] = t;
      }
      Vec16<T>::store(y + base + (long long)pu * g.Cs, v[u]);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void inorm_apply_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                            T* __restrict__ dx, const float* __restrict__ stats,
                                                            const float* __restrict__ sums, int act, float slope,
                                                            MomentGeom g) {
  constexpr int VE = Vec16<T>::N;
  const int tx = threadIdx.x & (g.TX - 1), ty = threadIdx.x >> g.tx_shift;
  const int col_blocks = (g.cv + g.TX - 1) / g.TX;
  const int cb = blockIdx.x % col_blocks;
  const int split = (blockIdx.x / col_blocks) % g.splits;
  const int n = blockIdx.x / (col_blocks * g.splits);
  const int col = cb * g.TX + tx;
  if (col >= g.cv) return;
  const int c0 = col * VE;
  float mean[VE], rstd[VE], s1[VE], s2[VE];
  const int nx = n >= g.alias ? n - g.alias : n;      // the saved forward image of gradient image n
  const long long sidx = ((long long)n * g.Cs + c0) * 2, xidx = ((long long)nx * g.Cs + c0) * 2;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    mean[e] = stats[xidx + 2 * e];
    rstd[e] = stats[xidx + 2 * e + 1];
    s1[e] = sums[sidx + 2 * e];
    s2[e] = sums[sidx + 2 * e + 1];
  }
  const int p0 = split * g.pix_per_split;
  int p1 = p0 + g.pix_per_split;
  p1 = p1 < g.HW ? p1 : g.HW;
  const long long base = (long long)n * g.HW * g.Cs + c0, xbase = (long long)nx * g.HW * g.Cs + c0;
  for (int p = p0 + ty; p < p1; p += JPDSE_NORM_ILP * g.TY) {
    float v[JPDSE_NORM_ILP][VE], gr[JPDSE_NORM_ILP][VE];
#pragma unroll
    for (int u = 0; u < JPDSE_NORM_ILP; ++u) {
      const int pu = p + u * g.TY;
      if (pu < p1) {
        JPDSE_LOAD_LAST(T, x + xbase + (long long)pu * g.Cs, v[u]);
        JPDSE_LOAD_LAST(T, dy + base + (long long)pu * g.Cs, gr[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < JPDSE_NORM_ILP; ++u) {
      const int pu = p + u * g.TY;
      if (pu >= p1) break;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float yh = (v[u][e] - mean[e]) * rstd[e];
        const float dz = gr[u][e] * act_grad(yh, act, slope);
        v[u][e] = rstd[e] * (dz - s1[e] - yh * s2[e]);
      }
      Vec16<T>::store(dx + base + (long long)pu * g.Cs, v[u]);
    }
  }
}


// ---- register-held forms ------------------------------------------------------------------
// Geometry: a block owns `span` = TY * P pixels of TX 16-byte channel columns of one image and holds them in registers; the
// `splits` blocks of one (image, channel block) = one GROUP are consecutive in the grid.
//   TWO kernels (default, any tensor with <= 64 splits): PHASE 1 writes one row of partial sums per block, PHASE 2 loads
//     its pixels, sums the group's rows itself (split order: deterministic; the rows are L2 hits and load under the
//     pixel loads), and applies.  Against moment -> finalize -> apply this drops a launch and the finalize round trip.
//   (ONE kernel whose blocks exchanged their rows inside the launch -- PHASE 0, developer mode 28 -- is retired: each
//     cross-XCD hop of the exchange cost ~2 us, which ate what the saved launch and re-read gave, profiles/r02_norm_forms.txt;
//     and it was the only place where workgroups waited on other workgroups of their own launch.)
static inline int norm_form() {
#ifdef JPDSE_DEV
  return g_norm_fused;     // 1 = two kernels (shipped default), 0 = moment -> finalize -> apply
#else
  return 1;
#endif
}
#ifdef JPDSE_DEV
int g_norm_fused = 1;
#endif

struct FusedGeom {
  int N, HW, Cs, cv;
  int TX, TY, tx_shift;          // threads across 16-byte channel columns / pixels (TX * TY = 256)
  int col_blocks, splits, span;  // blocks per image across channels / pixels; pixels per block (TY * P)
  int nv;                        // floats per partial row: TX * VE * 2
  int alias;                     // backward: images >= alias read the saved x / stats of image n - alias (0 = off)
};

static FusedGeom fused_geom(int N, int HW, int Cs, int VE, int P) {
  FusedGeom g;
  g.N = N; g.HW = HW; g.Cs = Cs; g.cv = Cs / VE; g.alias = 0;
  int tx = 1;
  while (tx < g.cv && tx < 16) tx <<= 1;       // <= 256 contiguous bytes per pixel and block
  g.TX = tx; g.TY = 256 / tx;
  g.tx_shift = 0;
  while ((1 << g.tx_shift) < tx) ++g.tx_shift;
  g.col_blocks = (g.cv + g.TX - 1) / g.TX;
  g.span = g.TY * P;
  g.splits = (HW + g.span - 1) / g.span;
  g.nv = g.TX * VE * 2;
  return g;
}

// Sum over the block's TY pixel rows: value j (< nv) of the block's partial row, returned in thread j.
template <int VE>
__device__ __forceinline__ float block_row(float* red, const float (&s1)[8], const float (&s2)[8], const FusedGeom& g) {
  const int tid = threadIdx.x;
  const int tx = tid & (g.TX - 1), ty = tid >> g.tx_shift;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    red[ty * g.nv + (tx * VE + e) * 2] = s1[e];
    red[ty * g.nv + (tx * VE + e) * 2 + 1] = s2[e];
  }
  __syncthreads();
  float tsum = 0.f;
  if (tid < g.nv)
    for (int yy = 0; yy < g.TY; ++yy) tsum += red[yy * g.nv + tid];
  __syncthreads();                                    // red[] is free again
  return tsum;
}

// Sum of the group's rows in split order (sixteen loads in flight, added in order).
__device__ __forceinline__ float sum_rows(const float* rows, int splits, int nv) {
  float total = 0.f;
  for (int s0 = 0; s0 < splits; s0 += 16) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float* q = rows + (long long)(s0 + k) * nv;
      v[k] = 0.f;
      if (s0 + k < splits) v[k] = *q;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) total += v[k];       // + 0.f for the absent rows changes nothing
  }
  return total;
}

// PHASE 2: on return red[j] holds the group total of value j, summed from the rows PHASE 1 wrote
__device__ __forceinline__ void group_totals(float* red, const float* partial, int grp, const FusedGeom& g) {
  const int tid = threadIdx.x;
  const float* rows = partial + (long long)grp * g.splits * g.nv;
  const float total = tid < g.nv ? sum_rows(rows + tid, g.splits, g.nv) : 0.f;
  if (tid < g.nv) red[tid] = total;
  __syncthreads();
}

template <typename T, int P, int PHASE>
__global__ __launch_bounds__(256, 4) void inorm_reg_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                             T* __restrict__ y, float* __restrict__ stats, float* partial,
                                                             unsigned* unused, int act, float slope, float eps, FusedGeom g,
                                                             int mslots = 0) {
  // PHASE 1: rows of partial sums; PHASE 2: apply from the group's rows.  (`unused`: the count words of the retired PHASE 0;
  // the slot keeps the argument layout, hence the code, of the kernels as they are.)
  static_assert(PHASE >= 1 && PHASE <= 3, "PHASE 0 (in-launch exchange) is retired");
  // PHASE 3: statistics from the per-block (mean, M2) slots a conv epilogue wrote (`partial` = moments[n][c][mslots][2],
  // common.h): one kernel per norm -- each block merges the slots of its channels itself (Chan's formula, slot order) and applies
  constexpr int VE = Vec16<T>::N;
  __shared__ float red[256 * VE * 2];
  const int tid = threadIdx.x;
  const int tx = tid & (g.TX - 1), ty = tid >> g.tx_shift;
  const int split = blockIdx.x % g.splits, grp = blockIdx.x / g.splits;
  const int cb = grp % g.col_blocks, n = grp / g.col_blocks;
  const int col = cb * g.TX + tx;
  const bool on = col < g.cv;
  const int c0 = (on ? col : 0) * VE;
  const long long base = (long long)n * g.HW * g.Cs + c0;
  const int p0 = split * g.span + ty;
  u32x4 xv[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int p = p0 + i * g.TY;
    if (on && p < g.HW) xv[i] = *reinterpret_cast<const u32x4*>(x + base + (long long)p * g.Cs);
  }
  float aux[8], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { aux[e] = 0.f; s1[e] = 0.f; s2[e] = 0.f; }
  if (on && PHASE != 3) {
    float v[VE];
    Vec16<T>::load(x + base, v);                      // shift = the image's first pixel, as in the three-kernel form
#pragma unroll
    for (int e = 0; e < VE; ++e) aux[e] = v[e];
  }
  if constexpr (PHASE == 3) {
    const int nch = g.TX * VE;
    if (tid < nch) {
      const int ch = cb * nch + tid;
      float mean = 0.f, var = 0.f;
      if (ch < g.Cs) {
        const float2* const src = reinterpret_cast<const float2*>(partial) + ((long long)n * g.Cs + ch) * mslots;
        float a = 0.f;
        for (int q = 0; q < mslots; ++q) a += src[q].x;
        mean = a / (float)mslots;
        const float ns = (float)g.HW / (float)mslots;
        float b = 0.f;
        for (int q = 0; q < mslots; ++q) {
          const float2 v = src[q];
          const float dm = v.x - mean;
          b += v.y + ns * dm * dm;
        }
        var = b / (float)g.HW;
        var = var > 0.f ? var : 0.f;
      }
      red[tid * 2] = mean;
      red[tid * 2 + 1] = var;
    }
    __syncthreads();
  } else if constexpr (PHASE == 2) {
    group_totals(red, partial, grp, g);
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int p = p0 + i * g.TY;
      if (on && p < g.HW) {
        float v[VE];
        Vec16<T>::unpack(xv[i], v);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const float d = v[e] - aux[e];
          s1[e] += d;
          s2[e] += d * d;
        }
      }
    }
    const float tsum = block_row<VE>(red, s1, s2, g);
    if (tid < g.nv) partial[((long long)grp * g.splits + split) * g.nv + tid] = tsum;
    return;
  }
  float mean[VE], rstd[VE];
  const float inv = 1.f / (float)g.HW;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if constexpr (PHASE == 3) {
      mean[e] = red[(tx * VE + e) * 2];
      rstd[e] = rsqrtf(red[(tx * VE + e) * 2 + 1] + eps);
    } else {
      const float dm = red[(tx * VE + e) * 2] * inv;
      float var = red[(tx * VE + e) * 2 + 1] * inv - dm * dm;
      var = var > 0.f ? var : 0.f;
      mean[e] = aux[e] + dm;
      rstd[e] = rsqrtf(var + eps);
    }
  }
  if (on && split == 0 && ty == 0) {
    float* st = stats + ((long long)n * g.Cs + c0) * 2;
#pragma unroll
    for (int e = 0; e < VE; ++e) { st[2 * e] = mean[e]; st[2 * e + 1] = rstd[e]; }
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int p = p0 + i * g.TY;
    if (on && p < g.HW) {
      const long long off = base + (long long)p * g.Cs;
      float v[VE], r[VE];
      Vec16<T>::unpack(xv[i], v);
      if (res != nullptr) Vec16<T>::load(res + off, r);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        float t = norm_act(v[e], mean[e], rstd[e], act, slope);
        if (res != nullptr) t += r[e];
        v[e] = t;
      }
      Vec16<T>::store(y + off, v);
    }
  }
}

template <typename T, int P, int PHASE>
__global__ __launch_bounds__(256, (P == 8 ? 3 : 2)) void inorm_reg_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                             T* __restrict__ dx,
                                                                             const float* __restrict__ stats, float* partial,
                                                                             unsigned* unused, int act, float slope,
                                                                             FusedGeom g, int mslots = 0) {
  static_assert(PHASE >= 1 && PHASE <= 3, "PHASE 0 (in-launch exchange) is retired");
  // PHASE 3 (round 4): the two sums come from the per-block slots that the epilogue of the data-gradient kernel producing dy
  // wrote (`partial` = sums[n][c][mslots][2], gemm_halo.h NSUM): ONE kernel per norm backward -- each block adds the slots of
  // its channels itself (slot order: deterministic) and applies
  constexpr int VE = Vec16<T>::N;
  __shared__ float red[256 * VE * 2];
  const int tid = threadIdx.x;
  const int tx = tid & (g.TX - 1), ty = tid >> g.tx_shift;
  const int split = blockIdx.x % g.splits, grp = blockIdx.x / g.splits;
  const int cb = grp % g.col_blocks, n = grp / g.col_blocks;
  const int col = cb * g.TX + tx;
  const bool on = col < g.cv;
  const int c0 = (on ? col : 0) * VE;
  const int nx = n >= g.alias ? n - g.alias : n;      // the saved forward image of gradient image n
  const long long base = (long long)n * g.HW * g.Cs + c0, xbase = (long long)nx * g.HW * g.Cs + c0;
  const int p0 = split * g.span + ty;
  u32x4 xv[P], gv[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int p = p0 + i * g.TY;
    if (on && p < g.HW) {
      xv[i] = *reinterpret_cast<const u32x4*>(x + xbase + (long long)p * g.Cs);
      gv[i] = *reinterpret_cast<const u32x4*>(dy + base + (long long)p * g.Cs);
    }
  }
  float mean[VE], rstd[VE], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  {
    const float* st = stats + ((long long)nx * g.Cs + c0) * 2;
#pragma unroll
    for (int e = 0; e < VE; ++e) { mean[e] = st[2 * e]; rstd[e] = st[2 * e + 1]; }
  }
  if constexpr (PHASE == 3) {
    const int nch = g.TX * VE;
    if (tid < nch) {
      const int ch = cb * nch + tid;
      float a = 0.f, b = 0.f;
      if (ch < g.Cs) {
        const float2* const src = reinterpret_cast<const float2*>(partial) + ((long long)n * g.Cs + ch) * mslots;
        for (int q = 0; q < mslots; ++q) {
          const float2 v = src[q];
          a += v.x;
          b += v.y;
        }
      }
      red[tid * 2] = a;
      red[tid * 2 + 1] = b;
    }
    __syncthreads();
  } else if constexpr (PHASE == 2) {
    group_totals(red, partial, grp, g);
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int p = p0 + i * g.TY;
      if (on && p < g.HW) {
        float v[VE], gr[VE];
        Vec16<T>::unpack(xv[i], v);
        Vec16<T>::unpack(gv[i], gr);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const float yh = (v[e] - mean[e]) * rstd[e];
          const float dz = gr[e] * act_grad(yh, act, slope);
          s1[e] += dz;
          s2[e] += dz * yh;
        }
      }
    }
    const float tsum = block_row<VE>(red, s1, s2, g);
    if (tid < g.nv) partial[((long long)grp * g.splits + split) * g.nv + tid] = tsum;
    return;
  }
  float m1[VE], m2[VE];
  const float inv = 1.f / (float)g.HW;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    m1[e] = red[(tx * VE + e) * 2] * inv;
    m2[e] = red[(tx * VE + e) * 2 + 1] * inv;
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int p = p0 + i * g.TY;
    if (on && p < g.HW) {
      float v[VE], gr[VE];
      Vec16<T>::unpack(xv[i], v);
      Vec16<T>::unpack(gv[i], gr);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float yh = (v[e] - mean[e]) * rstd[e];
        const float dz = gr[e] * act_grad(yh, act, slope);
        v[e] = rstd[e] * (dz - m1[e] - yh * m2[e]);
      }
      Vec16<T>::store(dx + base + (long long)p * g.Cs, v);
    }
  }
}

// Geometry of the register-held forms for a call: 8 pixels per thread -- with 16 (tensors of 17-34 MB) the two-kernel form
// measured equal or slower than the three-kernel form (profiles/r02_norm_forms.txt).  False: moment -> finalize -> apply.
template <typename T> static bool reg_geom(const jpdse_inorm_desc* d, FusedGeom* out) {
  const FusedGeom g = fused_geom(d->N, d->H * d->W, cpad(d->C), Vec16<T>::N, 8);
  if (g.splits > 64 || (long long)d->N * g.col_blocks * g.splits > (1ll << 30)) return false;
  *out = g;
  return true;
}

static size_t reg_ws_bytes(const jpdse_inorm_desc* d) {
  // Rows of the register-held form (8 pixels per thread); 0 when it does not apply.  The bound is 128 splits although
  // reg_geom admits 64: the retired one-kernel form could hold 16 pixels per thread, whose 64 splits are 128 at 8, and
  // jpdse_inorm_workspace_size reports this number, so it stays as it is.
  const FusedGeom g = fused_geom(d->N, d->H * d->W, cpad(d->C), vec_elems(d->dtype), 8);
  if (g.splits > 128) return 0;
  return align_up((size_t)d->N * g.col_blocks * g.splits * g.nv * sizeof(float), 256);
}

// Forward statistics from per-block moments written by a conv epilogue: moments[n][c][slot] = (mean, M2) of the block's
// (bf16-rounded) values, every slot over the same number of pixels HW / slots (common.h).  One wave per (n, c) merges them with
// Chan's parallel-variance formula in two passes over the slots (they are L2 hits): mean = average of the slot means, then
// M2 = sum_slots [M2_s + n_s (mean_s - mean)^2] -- no E[y^2] - mean^2 of un-shifted sums anywhere (the stand-alone moment
// kernels above shift by x[n,0,c] for the same reason).  Lane l takes slots l, l + 64, ... in order, then the fixed xor tree:
// deterministic.
__global__ __launch_bounds__(256) void finalize_slots_kernel(const float* __restrict__ mom, float* __restrict__ stats, int NC,
                                                            int slots, int HW, float eps) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pair >= NC) return;
  const float2* const src = reinterpret_cast<const float2*>(mom) + (long long)pair * slots;
  float a = 0.f;
  int s = lane;
  for (; s + 192 < slots; s += 256) {
    const float2 v0 = src[s], v1 = src[s + 64], v2 = src[s + 128], v3 = src[s + 192];
    a += v0.x;
    a += v1.x;
    a += v2.x;
    a += v3.x;
  }
  for (; s < slots; s += 64) a += src[s].x;
  const float mean = wave_sum(a) / (float)slots;
  const float ns = (float)HW / (float)slots;
  float b = 0.f;
  for (s = lane; s < slots; s += 64) {
    const float2 v = src[s];
    const float dm = v.x - mean;
    b += v.y + ns * dm * dm;
  }
  b = wave_sum(b);
  if (lane == 0) {
    float var = b / (float)HW;
    var = var > 0.f ? var : 0.f;
    stats[2 * pair] = mean;
    stats[2 * pair + 1] = rsqrtf(var + eps);
  }
}

// Backward sums from per-block slots written by the epilogue of the data-gradient kernel that produced dy:
// sums[n][c][slot] = (sum dz, sum dz * yhat) over the block's pixels.  (n, c) pairs are summed in slot order by 8 lanes each.
__global__ __launch_bounds__(256) void finalize_bwd_slots_kernel(const float* __restrict__ slots_in, float* __restrict__ sums, int NC,
                                                                int slots, int HW) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int idx = gid >> 3, sub = gid & 7;
  float a = 0.f, b = 0.f;
  if (idx < NC) {
    const float2* const src = reinterpret_cast<const float2*>(slots_in) + (long long)idx * slots;
    for (int q = sub; q < slots; q += 8) {
      const float2 v = src[q];
      a += v.x;
      b += v.y;
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if (idx >= NC || sub != 0) return;
  const float inv = 1.f / (float)HW;
  sums[2 * idx] = a * inv;
  sums[2 * idx + 1] = b * inv;
}

// ---- host layer -----------------------------------------------------------------------------------------------------------
// One norm call: forward in2 = the residual (or null) and out = y; backward in2 = dy and out = dx.
struct NormCall {
  const jpdse_inorm_desc* d;
  const void* x;
  const void* in2;
  void* out;
  float* stats;          // written by the forward, read by the backward
  void* stream;
  int alias;             // backward over more gradient images than saved ones: images >= alias read x / stats of image n - alias (0 = off)
};

// an aliased backward (d->alias != 0) splits the pixels as the call over the saved batch does: each image's sums are then added
// in that call's order
static MomentGeom moment_geom(const jpdse_inorm_desc* d) {
  MomentGeom g = moment_geom(d->N - d->alias, d->H * d->W, cpad(d->C), vec_elems(d->dtype));
  g.N = d->N;
  return g;
}
// grid of the MomentGeom kernels (moment_kernel, inorm_apply_*): a block per (image, pixel split, TX channel columns)
static dim3 moment_grid(const MomentGeom& g) { return dim3(g.N * g.splits * ((g.cv + g.TX - 1) / g.TX)); }
// grid of the kernels that give 8 lanes to each (image, channel): the finalize kernels
static dim3 lanes8_grid(const jpdse_inorm_desc* d) { return dim3((d->N * cpad(d->C) * 8 + 255) / 256); }
static dim3 fused_grid(const FusedGeom& g) { return dim3((unsigned)((size_t)g.N * g.col_blocks * g.splits)); }

// Workspace of moment -> finalize -> apply: the partials [N][splits][Cs][2], then the backward's sums [N][Cs][2], each region
// rounded up to 256 bytes.  jpdse_inorm_bwd_from_sums needs the sums region alone, at offset 0.
static size_t ws_sums_bytes(const jpdse_inorm_desc* d) { return align_up((size_t)d->N * cpad(d->C) * 2 * sizeof(float), 256); }
static size_t ws_sums_offset(const jpdse_inorm_desc* d, const MomentGeom& g) {
  return align_up((size_t)d->N * g.splits * g.Cs * 2 * sizeof(float), 256);
}
static size_t ws_bytes_for(const jpdse_inorm_desc* d) {
  const size_t three = ws_sums_offset(d, moment_geom(d)) + ws_sums_bytes(d), reg = reg_ws_bytes(d);
  return three > reg ? three : reg;
}

// inorm_reg_{fwd,bwd}_kernel<T, 8, PHASE>.  `part`: the partial rows (PHASE 1-2) or the producer's `mslots` slots (PHASE 3).
template <typename T, int PHASE, bool BWD>
static int launch_reg(const NormCall& c, FusedGeom fg, float* part, int mslots = 0) {
  static const char* const what[2][3] = {{"inorm rows fwd", "inorm apply-from-rows fwd", "inorm apply-from-slots fwd"},
                                         {"inorm rows bwd", "inorm apply-from-rows bwd", "inorm apply-from-slots bwd"}};
  const jpdse_inorm_desc* d = c.d;
  fg.alias = BWD ? c.alias : 0;
  if constexpr (BWD)
    return launch256(what[1][PHASE - 1], inorm_reg_bwd_kernel<T, 8, PHASE>, fused_grid(fg), c.stream, cptr<T>(c.x), cptr<T>(c.in2),
                     mptr<T>(c.out), c.stats, part, (unsigned*)nullptr, d->act, d->slope, fg, mslots);
  else
    return launch256(what[0][PHASE - 1], inorm_reg_fwd_kernel<T, 8, PHASE>, fused_grid(fg), c.stream, cptr<T>(c.x), cptr<T>(c.in2),
                     mptr<T>(c.out), c.stats, part, (unsigned*)nullptr, d->act, d->slope, d->eps, fg, mslots);
}

constexpr int kNoRegForm = 1;      // returned by the two routines below when the register-held forms do not cover the call

// The two-kernel form (rows, then apply-from-rows), or kNoRegForm: the caller runs moment -> finalize -> apply.
template <typename T, bool BWD> static int try_reg(const NormCall& c, void* ws) {
  FusedGeom fg;
  if (norm_form() == 0 || !reg_geom<T>(c.d, &fg)) return kNoRegForm;
  float* part = mptr<float>(ws);
  if (int rc = launch_reg<T, 1, BWD>(c, fg, part)) return rc;
  return launch_reg<T, 2, BWD>(c, fg, part);
}

// PHASE 3, ONE kernel per norm: every block merges the producer's slots of its channels itself and applies.  For tensors the
// two-kernel form covers with 8 pixels per thread (e.g. the ResnetBlock norms) and at most 64 slots per (image, channel).
template <typename T, bool BWD> static int try_reg_from_slots(const NormCall& c, const float* slots_in, int slots) {
  FusedGeom fg;
  if (norm_form() == 0 || slots > 64 || !reg_geom<T>(c.d, &fg)) return kNoRegForm;
  return launch_reg<T, 3, BWD>(c, fg, const_cast<float*>(slots_in), slots);
}

// third kernel of moment -> finalize -> apply; `sums`: backward only
template <typename T, bool BWD> static int launch_apply(const NormCall& c, MomentGeom g, const float* sums = nullptr) {
  g.alias = BWD ? c.alias : 0;
  if constexpr (BWD)
    return launch256("inorm apply bwd", inorm_apply_bwd_kernel<T>, moment_grid(g), c.stream, cptr<T>(c.x), cptr<T>(c.in2),
                     mptr<T>(c.out), c.stats, sums, c.d->act, c.d->slope, g);
  else
    return launch256("inorm apply fwd", inorm_apply_fwd_kernel<T>, moment_grid(g), c.stream, cptr<T>(c.x), cptr<T>(c.in2),
                     mptr<T>(c.out), c.stats, c.d->act, c.d->slope, g);
}

template <typename T> static int inorm_fwd_t(const NormCall& c, void* ws) {
  if (const int r = try_reg<T, false>(c, ws); r != kNoRegForm) return r;
  const jpdse_inorm_desc* d = c.d;
  const MomentGeom g = moment_geom(d);
  float* partial = mptr<float>(ws);
  if (int rc = launch256("inorm moment fwd", moment_kernel<T, false>, moment_grid(g), c.stream, cptr<T>(c.x), nullptr, nullptr, 0,
                         0.f, partial, g))
    return rc;
  if (int rc = launch256("inorm finalize fwd", finalize_fwd_kernel<T>, lanes8_grid(d), c.stream, cptr<T>(c.x), partial, c.stats,
                         d->N, g.HW, g.Cs, g.splits, d->eps))
    return rc;
  return launch_apply<T, false>(c, g);
}

template <typename T> static int inorm_bwd_t(const NormCall& c, void* ws) {
  if (const int r = try_reg<T, true>(c, ws); r != kNoRegForm) return r;
  const jpdse_inorm_desc* d = c.d;
  MomentGeom g = moment_geom(d);
  g.alias = c.alias;
  float* partial = mptr<float>(ws);
  float* sums = reinterpret_cast<float*>(mptr<char>(ws) + ws_sums_offset(d, g));
  if (int rc = launch256("inorm moment bwd", moment_kernel<T, true>, moment_grid(g), c.stream, cptr<T>(c.x), cptr<T>(c.in2),
                         c.stats, d->act, d->slope, partial, g))
    return rc;
  if (int rc = launch256("inorm finalize bwd", finalize_bwd_kernel, lanes8_grid(d), c.stream, partial, sums, d->N, g.HW, g.Cs,
                         g.splits))
    return rc;
  return launch_apply<T, true>(c, g, sums);
}

template <typename T> static int inorm_bwd_from_sums_t(const NormCall& c, const float* slot_sums, int slots, void* ws) {
  if (const int r = try_reg_from_slots<T, true>(c, slot_sums, slots); r != kNoRegForm) return r;
  const jpdse_inorm_desc* d = c.d;
  float* const sums = mptr<float>(ws);
  if (int rc = launch256("inorm finalize bwd from slots", finalize_bwd_slots_kernel, lanes8_grid(d), c.stream, slot_sums, sums,
                         d->N * cpad(d->C), slots, d->H * d->W))
    return rc;
  return launch_apply<T, true>(c, moment_geom(d), sums);
}

template <typename T> static int inorm_from_moments_t(const NormCall& c, const float* mom, int slots) {
  if (const int r = try_reg_from_slots<T, false>(c, mom, slots); r != kNoRegForm) return r;
  const jpdse_inorm_desc* d = c.d;
  const int NC = d->N * cpad(d->C);
  if (int rc = launch256("inorm finalize from moments", finalize_slots_kernel, dim3((NC + 3) / 4), c.stream, mom, c.stats, NC,
                         slots, d->H * d->W, d->eps))
    return rc;
  return launch_apply<T, false>(c, moment_geom(d));
}

static int validate(const jpdse_inorm_desc* d) {
  JPDSE_REQUIRE(d != nullptr, "inorm: null descriptor");
  JPDSE_REQUIRE(d->dtype == JPDSE_F32 || d->dtype == JPDSE_BF16, "inorm: bad dtype");
  JPDSE_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0, "inorm: non-positive shape");
  JPDSE_REQUIRE(d->act == JPDSE_ACT_NONE || d->act == JPDSE_ACT_RELU || d->act == JPDSE_ACT_LRELU,
                "inorm: unsupported activation %d", d->act);
  // images n < alias read image n, images n >= alias image n - alias, of tensors that hold N - alias images
  JPDSE_REQUIRE(d->alias >= 0 && 2 * (long long)d->alias <= d->N, "inorm: alias %d outside [0, N / 2 = %d / 2]", d->alias, d->N);
  return JPDSE_OK;
}

// Prologue of the four launching entry points: descriptor, the call's own pointer check (`args_ok`, refused as `args_what`),
// the residual (forward calls pass theirs: it comes back null unless the descriptor has one) and the workspace.
enum NormWs { WS_NONE, WS_FULL, WS_SUMS };
static int inorm_enter(const char* name, const jpdse_inorm_desc* d, bool args_ok, const char* args_what, const void** residual,
                       NormWs kind, const void* ws, size_t ws_bytes) {
  if (int rc = validate(d)) return rc;
  JPDSE_REQUIRE(args_ok, "%s: %s", name, args_what);
  if (residual != nullptr) {
    JPDSE_REQUIRE(!d->has_residual || *residual, "%s: has_residual set but residual is null", name);
    if (!d->has_residual) *residual = nullptr;
  }
  if (kind != WS_NONE) {
    const size_t need = kind == WS_FULL ? ws_bytes_for(d) : ws_sums_bytes(d);
    if (ws == nullptr || ws_bytes < need) return set_error(JPDSE_EWORKSPACE, "%s: workspace %zu < %zu", name, ws_bytes, need);
  }
  return JPDSE_OK;
}

// run(T{}) for the descriptor's dtype between hbm_prof_begin / _end (jpdse_prof_hbm_*): class `cls`, algorithmic bytes =
// `tensors` x one [N][H][W][CPAD(C)] tensor of that dtype
template <typename F> static int timed_by_dtype(const jpdse_inorm_desc* d, void* stream, int cls, double tensors, F&& run) {
  const int pslot = hbm_prof_begin(as_stream(stream));
  const int rc = by_dtype(d->dtype, run);
  hbm_prof_end(pslot, cls, (double)d->N * d->H * d->W * cpad(d->C) * (double)esize(d->dtype) * tensors, as_stream(stream));
  return rc;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_inorm_workspace_size(const jpdse_inorm_desc* d) {
  if (jpdse::validate(d)) return 0;
  return ws_bytes_for(d);
}

int jpdse_inorm_fwd(const jpdse_inorm_desc* d, const void* x, const void* residual, void* y, float* stats, void* ws,
                    size_t ws_bytes, void* stream) {
  if (int rc = inorm_enter("inorm_fwd", d, x && y && stats, "null pointer", &residual, WS_FULL, ws, ws_bytes)) return rc;
  JPDSE_REQUIRE(d->alias == 0, "inorm_fwd: the descriptor's alias is for jpdse_inorm_bwd alone");
  const NormCall c = {d, x, residual, y, stats, stream};
  return timed_by_dtype(d, stream, JPDSE_HBM_INORM_FWD, d->has_residual ? 4.0 : 3.0,
                        [&](auto tag) { return inorm_fwd_t<decltype(tag)>(c, ws); });
}

int jpdse_inorm_bwd(const jpdse_inorm_desc* d, const void* x, const float* stats, const void* dy, void* dx, void* ws,
                    size_t ws_bytes, void* stream) {
  if (int rc = inorm_enter("inorm_bwd", d, x && stats && dy && dx, "null pointer", nullptr, WS_FULL, ws, ws_bytes)) return rc;
  const NormCall c = {d, x, dy, dx, const_cast<float*>(stats), stream, d->alias};
  return timed_by_dtype(d, stream, JPDSE_HBM_INORM_BWD, 5.0, [&](auto tag) { return inorm_bwd_t<decltype(tag)>(c, ws); });
}

int jpdse_inorm_bwd_from_sums(const jpdse_inorm_desc* d, const void* x, const float* stats, const void* dy, const float* sums,
                              int32_t slots, void* dx, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = inorm_enter("inorm_bwd_from_sums", d, x && stats && dy && dx && sums && slots > 0, "null pointer / no slots",
                           nullptr, WS_SUMS, ws, ws_bytes))
    return rc;
  JPDSE_REQUIRE(d->alias == 0, "inorm_bwd_from_sums: the descriptor's alias is for jpdse_inorm_bwd alone");
  const NormCall c = {d, x, dy, dx, const_cast<float*>(stats), stream};
  return timed_by_dtype(d, stream, JPDSE_HBM_INORM_BWD, 3.0,        // x, dy read once, dx written
                        [&](auto tag) { return inorm_bwd_from_sums_t<decltype(tag)>(c, sums, slots, ws); });
}

int jpdse_inorm_fwd_from_moments(const jpdse_inorm_desc* d, const void* x, const float* moments, int32_t slots,
                                 const void* residual, void* y, float* stats, void* stream) {
  if (int rc = inorm_enter("inorm_fwd_from_moments", d, x && y && stats && moments && slots > 0, "null pointer / no slots",
                           &residual, WS_NONE, nullptr, 0))
    return rc;
  JPDSE_REQUIRE(d->alias == 0, "inorm_fwd_from_moments: the descriptor's alias is for jpdse_inorm_bwd alone");
  const NormCall c = {d, x, residual, y, stats, stream};
  return timed_by_dtype(d, stream, JPDSE_HBM_INORM_FWD, d->has_residual ? 3.0 : 2.0,
                        [&](auto tag) { return inorm_from_moments_t<decltype(tag)>(c, moments, slots); });
}

}  // extern "C"
