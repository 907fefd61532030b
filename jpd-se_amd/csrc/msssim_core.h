// The MS-SSIM machinery shared by the evaluation metrics (metrics.hip) and the training loss (msssim_loss.hip,
// DESIGN.md 4.6): 11x11 Gaussian window (sigma 1.5, "valid"), five scales linked by a 2x2 mean, blocks of 256 threads that
// own 64 x 16 positions of one plane pair.  Shared: the tile geometry, the window, the centred staging, the separable
// filter up to the filtered moments in registers, the downsample, the block sum and the host geometry.  NOT shared: what
// a kernel does with the moments -- the two per-position formulas round differently and each caller's bits are a contract.
#pragma once
#include "common.h"

namespace jpdse {

constexpr int kMsScales = 5;
constexpr int kWin = 11;                 // window taps
constexpr int kHalo = kWin - 1;
constexpr int kTW = 64, kTH = 16;        // outputs per block: one wave per 64-wide row, four rows per wave
constexpr int kSW = kTW + kHalo;         // staged columns (74)
constexpr int kSH = kTH + kHalo;         // staged rows (26)
constexpr double kMsWeights[kMsScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

struct GaussWin { float w[kWin]; };

static inline GaussWin gauss_window() {
  GaussWin g;
  double w[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    const double d = k - (kWin - 1) / 2;
    w[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += w[k];
  }
  for (int k = 0; k < kWin; ++k) g.w[k] = (float)(w[k] / sum);
  return g;
}

// ---- device side: the LDS arrays are the calling kernel's, every helper is called by the whole block --------------------------
// Stages the 26 x 74 tile + halo at (x0, y0) of the planes xp, yp [Hs][Ws], each centred about its pivot, the tile's first
// pixel (always inside the plane: x0 < Wo, y0 < Ho), which is returned.  Ends with a barrier.
__device__ __forceinline__ void stage_centred(const float* __restrict__ xp, const float* __restrict__ yp, int Hs, int Ws, int x0,
                                              int y0, float (&sx)[kSH][kSW], float (&sy)[kSH][kSW], float& pvx, float& pvy) {
  pvx = xp[(long long)y0 * Ws + x0];
  pvy = yp[(long long)y0 * Ws + x0];
  for (int i = threadIdx.x; i < kSH * kSW; i += 256) {
    const int r = i / kSW, c = i - r * kSW;
    const int gy = y0 + r, gx = x0 + c;
    float vx = 0.f, vy = 0.f;            // outside the plane: only feeds positions that the caller masks out
    if (gy < Hs && gx < Ws) {
      vx = xp[(long long)gy * Ws + gx] - pvx;
      vy = yp[(long long)gy * Ws + gx] - pvy;
    }
    sx[r][c] = vx;
    sy[r][c] = vy;
  }
  __syncthreads();
}

// horizontal pass over x, y, x^2, y^2, xy: 26 rows x 64 columns, one row per wave and iteration.  Ends with a barrier.
__device__ __forceinline__ void horizontal_pass5(const float (&sx)[kSH][kSW], const float (&sy)[kSH][kSW], const GaussWin& g,
                                                 float (&hq)[5][kSH][kTW]) {
  for (int i = threadIdx.x; i < kSH * kTW; i += 256) {
    const int r = i >> 6, c = i & 63;
    float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float a = sx[r][c + k], b = sy[r][c + k], w = g.w[k];
      const float wa = w * a, wb = w * b;
      ax += wa;
      ay += wb;
      axx = fmaf(wa, a, axx);
      ayy = fmaf(wb, b, ayy);
      axy = fmaf(wa, b, axy);
    }
    hq[0][r][c] = ax;
    hq[1][r][c] = ay;
    hq[2][r][c] = axx;
    hq[3][r][c] = ayy;
    hq[4][r][c] = axy;
  }
  __syncthreads();
}

// vertical pass over Q horizontally filtered planes: thread = (column threadIdx.x & 63, the 4 output rows from
// (threadIdx.x >> 6) * 4); 14 filtered rows feed its 4 outputs per plane.  The callers' epilogues recompute this mapping
// (their c, r0): change it here and there together.
template <int Q>
__device__ __forceinline__ void vertical_pass(const float (&h)[Q][kSH][kTW], const GaussWin& g, float (&acc)[Q][4]) {
  const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    float v[4 + kHalo];
#pragma unroll
    for (int j = 0; j < 4 + kHalo; ++j) v[j] = h[q][r0 + j][c];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; ++k) a = fmaf(g.w[k], v[o + k], a);
      acc[q][o] = a;
    }
  }
}

// block sums of a and b in a fixed order (wave shuffle, then the four waves pairwise).  True in thread 0 alone, whose a and b
// then hold the sums.  One barrier; a caller that sums again puts another one before it.
__device__ __forceinline__ bool block_sum_pair(double& a, double& b, double (&red)[2][4]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  return true;
}

// 2x2 mean, stride 2, odd last row / column dropped; one thread per output, both planes (exact in fp32 on the evaluation
// path: its scale-j values carry 8 + 2(j-1) bits).  static: each including source gets its own host stub.
static __global__ __launch_bounds__(256) void msssim_down_kernel(const float* __restrict__ x, const float* __restrict__ y, int Hs,
                                                                int Ws, float* __restrict__ ox, float* __restrict__ oy,
                                                                long long total) {
  const int Hd = Hs >> 1, Wd = Ws >> 1;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cx = (int)(i % Wd);
    const long long t = i / Wd;
    const int cy = (int)(t % Hd);
    const long long nc = t / Hd;
    const long long s = (nc * Hs + 2 * cy) * Ws + 2 * cx;
    ox[i] = ((x[s] + x[s + 1]) + (x[s + Ws] + x[s + Ws + 1])) * 0.25f;
    oy[i] = ((y[s] + y[s + 1]) + (y[s + Ws] + y[s + Ws + 1])) * 0.25f;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// where the scale kernels' partial pairs sit and what they cover: the head of both final kernels' argument structs
struct MsPartials {
  long long scale_off[kMsScales];   // first partial pair of the scale (in pairs), image 0
  int scale_cnt[kMsScales];         // pairs per image (3 channels x tiles)
  double pos[kMsScales];            // 3 * Ho * Wo: positions behind a per-scale mean
};

struct MsGeometry {
  int Hs[kMsScales], Ws[kMsScales], tx[kMsScales], ty[kMsScales];
  size_t plane_off[kMsScales];     // floats, from the start of the x planes (every other set of planes has the same layout)
  size_t plane_floats;             // all scales, one image of the pair
};

// fills g and part for N images of H x W; returns the number of partial pairs of the call
static inline long long ms_geometry(int N, int H, int W, MsGeometry& g, MsPartials& part) {
  size_t off = 0;
  long long pairs = 0;
  for (int j = 0; j < kMsScales; ++j) {
    g.Hs[j] = H >> j;
    g.Ws[j] = W >> j;
    g.tx[j] = (g.Ws[j] - kHalo + kTW - 1) / kTW;
    g.ty[j] = (g.Hs[j] - kHalo + kTH - 1) / kTH;
    g.plane_off[j] = off;
    off += align_up((size_t)N * 3 * g.Hs[j] * g.Ws[j], 64);
    part.scale_off[j] = pairs;
    part.scale_cnt[j] = 3 * g.tx[j] * g.ty[j];
    part.pos[j] = 3.0 * (double)(g.Hs[j] - kHalo) * (double)(g.Ws[j] - kHalo);
    pairs += (long long)N * part.scale_cnt[j];
  }
  g.plane_floats = off;
  return pairs;
}

// The shapes the five-scale pass and its launch grids can take: nullptr, or what is wrong, to follow "<caller's name>: ".
// grid_halo: the caller's largest grid at scale 1 has ceil((H - grid_halo) / 16) x ceil((W - grid_halo) / 64) tiles: kHalo
// where only the valid region is tiled, 0 where the full plane is as well.
static inline const char* ms_shape_error(int N, int H, int W, int C, int grid_halo) {
  if (N <= 0 || H <= 0 || W <= 0) return "bad shape";
  if (C != 3) return "3 channels only";
  if (H < 176 || W < 176) return "the shorter side must be at least 176 (five MS-SSIM scales of an 11x11 window)";
  if ((long long)N * 3 > 65535) return "more than 21845 images per call";
  if ((long long)H * W > (1LL << 28)) return "image beyond 2^28 pixels";
  if ((H - grid_halo + kTH - 1) / kTH > 65535 || (W - grid_halo + kTW - 1) / kTW > 65535) return "image side beyond the tile grid";
  return nullptr;
}

}  // namespace jpdse
