// Test-time distortion metrics of a reconstruction against its original, in one device pass (reference test.py:114-125:
// L1, MSE and MS-SSIM of the de-normalised, clipped, uint8-truncated images).  Entry points: include/jpdse.h,
// "evaluation metrics".  MS-SSIM is the definition of Wang, Simoncelli and Bovik 2003 as written out in DESIGN.md 4.5:
// 11x11 Gaussian window (sigma 1.5, "valid"), five scales linked by a 2x2 mean, per channel.
//
// Kernels, in launch order:
//   metrics_quant_kernel   both images -> quantised planar fp32 planes [N][3][H][W] (scale 1) + exact integer |d|, d^2 sums
//   msssim_scale_kernel    one per scale: LDS tile + halo of both planes, separable 11-tap filter of x, y, x^2, y^2, xy,
//                          cs / ssim per position, one (cs, ssim) partial pair per block
//   msssim_down_kernel     2x2 mean -> next scale's planes (exact in fp32: scale j values carry 8 + 2(j-1) bits)
//   metrics_final_kernel   per image: partials -> out[n][14], fixed order, no atomics: two runs are bit-identical
// With a label map (jpdse_eval_metrics_sem) the quantise pass also splits its two integer sums by semantic class -- one table
// per wave in LDS, one partial row per block -- and metrics_cls_final_kernel adds the rows into cls[n][n_classes + 1][3].
//
// Cancellation: every tile is filtered about its own pivot (the value of its first pixel, per image of the pair): the local
// statistics are shift invariant, E[(x-p)^2] - (mu-p)^2 is formed from values of the size of the tile's contrast instead
// of 0..255, and a constant tile gives variance exactly 0.  The filter runs in fp32; the per-position cs / ssim and every
// sum over positions are fp64.  The window, the staging, the filter passes, the downsample, the block sum and the geometry
// are in msssim_core.h, shared with msssim_loss.hip.
#include "msssim_core.h"

namespace jpdse {

constexpr int kQuantBlocksMax = 1024;    // per image
constexpr int kOutPerImage = 4 + 2 * kMsScales;
constexpr int kClassesMax = 256;         // jpdse_eval_metrics_sem

// fake: NHWC [N][H][W][cs] fp32 or bf16, real: NHWC fp32.  One thread per pixel; planes x (fake) / y (real): [N][3][H*W].
// kCls: label [N][H*W] fp32 is read as well and the two sums are split by class into cpartial[n][block][n_classes + 1][3]
// (|d| sum, d^2 sum, pixels; row n_classes = labels outside [0, n_classes) or not integers).  A wave first reduces over the
// lanes of one class (ballot on equality with the first open lane's class, then a shuffle sum: neighbouring pixels mostly
// share a class, so the loop runs once or twice), then lane 0 adds into the wave's OWN table in LDS: no atomics, no lanes
// meeting on one address.  Entries are 64-bit: a block of 2^18 pixels sums d^2 up to 5.1e10.  Dynamic LDS: 4 waves x
// (n_classes + 1) x 3 x 8 bytes (24.1 KB at 256 classes).
template <typename TF, bool kCls>
__global__ __launch_bounds__(256) void metrics_quant_kernel(const TF* __restrict__ fake, const float* __restrict__ real,
                                                           int cs, long long HW, QuantParams qp, float* __restrict__ px,
                                                           float* __restrict__ py,
                                                           unsigned long long* __restrict__ partial,
                                                           const float* __restrict__ label, int n_classes,
                                                           unsigned long long* __restrict__ cpartial) {
  __shared__ unsigned long long red[2][4];
  extern __shared__ unsigned long long ctab[];      // kCls: [4 waves][(n_classes + 1) * 3]
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int centries = (n_classes + 1) * 3;
  const TF* f = fake + (long long)n * HW * cs;
  const float* r = real + (long long)n * HW * cs;
  float* ox = px + (long long)n * 3 * HW;
  float* oy = py + (long long)n * 3 * HW;
  if constexpr (kCls) {
    for (int i = threadIdx.x; i < 4 * centries; i += 256) ctab[i] = 0;
    __syncthreads();
  }
  unsigned long long l1 = 0, se = 0;
  // the trip count is the same for the whole block (the class reduction below runs wave-wide); lanes past the end idle
  for (long long base = blockIdx.x * 256LL; base < HW; base += (long long)gridDim.x * 256) {
    const long long p = base + threadIdx.x;
    const bool valid = p < HW;
    unsigned pl1 = 0, pse = 0;
    if (valid) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int qa = quant_u8(ElemOps<TF>::ld(f + p * cs + c), qp.std[c], qp.mean[c]);
        const int qb = quant_u8(r[p * cs + c], qp.std[c], qp.mean[c]);
        const int d = qa - qb;
        pl1 += (unsigned)(d < 0 ? -d : d);
        pse += (unsigned)(d * d);
        ox[c * HW + p] = (float)qa;
        oy[c * HW + p] = (float)qb;
      }
    }
    l1 += pl1;
    se += pse;
    if constexpr (kCls) {
      int k = -1;                                   // idle lane: matches no class
      if (valid) {
        const float lab = label[(long long)n * HW + p];
        k = (lab >= 0.f && lab < (float)n_classes && lab == floorf(lab)) ? (int)lab : n_classes;   // NaN: the extra row
      }
      unsigned long long open = __ballot(valid);
      unsigned long long* tab = ctab + wave * centries;
      while (open) {                                // wave-uniform
        const int kc = __shfl(k, __ffsll((long long)open) - 1, 64);
        const bool mine = k == kc;
        const unsigned long long m = __ballot(mine);
        unsigned a = mine ? pl1 : 0u, b = mine ? pse : 0u;     // <= 64 * 765 and 64 * 195075: 32 bits hold the wave's sums
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          a += __shfl_xor(a, off, 64);
          b += __shfl_xor(b, off, 64);
        }
        if (lane == 0) {
          tab[kc * 3 + 0] += a;
          tab[kc * 3 + 1] += b;
          tab[kc * 3 + 2] += (unsigned)__popcll(m);
        }
        open &= ~m;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    l1 += __shfl_xor(l1, off, 64);
    se += __shfl_xor(se, off, 64);
  }
  if (lane == 0) {
    red[0][wave] = l1;
    red[1][wave] = se;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* o = partial + ((long long)n * gridDim.x + blockIdx.x) * 2;
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
  if constexpr (kCls) {
    unsigned long long* o = cpartial + ((long long)n * gridDim.x + blockIdx.x) * centries;
    for (int i = threadIdx.x; i < centries; i += 256)
      o[i] = ctab[i] + ctab[centries + i] + ctab[2 * centries + i] + ctab[3 * centries + i];
  }
}

// cpartial[n][qblocks][entries] -> cls[n][entries], entries = (n_classes + 1) * 3.  grid (ceil(entries / 64), N): lane =
// entry, the four waves take the blocks 4i + wave in order and are then added in order (integers: exact in any order).
__global__ __launch_bounds__(256) void metrics_cls_final_kernel(const unsigned long long* __restrict__ cpartial, int qblocks,
                                                               int entries, long long* __restrict__ cls) {
  __shared__ unsigned long long red[4][64];
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  unsigned long long a = 0;
  if (e < entries) {
    const unsigned long long* p = cpartial + (long long)n * qblocks * entries + e;
    for (int b = wave; b < qblocks; b += 4) a += p[(long long)b * entries];
  }
  red[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && e < entries)
    cls[(long long)n * entries + e] = (long long)(red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]);
}

// x, y: planes [NC][Hs][Ws]; grid (tiles_x, tiles_y, NC); partial: [NC][tiles_y][tiles_x][2] doubles (sum cs, sum ssim over
// the block's valid positions).  LDS: 2 staged tiles + 5 horizontally filtered planes = 48.7 KB, three blocks per CU.  Every
// LDS access of a wave is 64 consecutive dwords of one row (plus a tap offset): conflict free on the 64 banks.
__global__ __launch_bounds__(256) void msssim_scale_kernel(const float* __restrict__ x, const float* __restrict__ y, int Hs,
                                                          int Ws, GaussWin g, double c1, double c2,
                                                          double* __restrict__ partial) {
  __shared__ float sx[kSH][kSW];
  __shared__ float sy[kSH][kSW];
  __shared__ float hq[5][kSH][kTW];
  __shared__ double red[2][4];
  const int Ho = Hs - kHalo, Wo = Ws - kHalo;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const long long plane = (long long)blockIdx.z * Hs * Ws;
  float pvx, pvy, acc[5][4];          // pivots; filtered x, y, x^2, y^2, xy of the thread's 4 positions
  stage_centred(x + plane, y + plane, Hs, Ws, x0, y0, sx, sy, pvx, pvy);
  horizontal_pass5(sx, sy, g, hq);
  vertical_pass<5>(hq, g, acc);
  const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;   // acc[q][o] is position (r0 + o, c): must match vertical_pass
  // own epilogue, not msssim_loss.hip's: cs is written with plain operators here and these bits are jpdse_eval_metrics' contract
  double scs = 0.0, sss = 0.0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if (x0 + c < Wo && y0 + r0 + o < Ho) {
      const double mx = acc[0][o], my = acc[1][o];
      const double vxx = (double)acc[2][o] - mx * mx, vyy = (double)acc[3][o] - my * my;
      const double vxy = (double)acc[4][o] - mx * my;
      const double mux = (double)pvx + mx, muy = (double)pvy + my;
      const double cs = (2.0 * vxy + c2) / (vxx + vyy + c2);
      // unfused, so that identical images give num == den bit for bit (2 mu^2 is formed the same way on both sides)
      const double pxy = __dmul_rn(mux, muy);
      const double lum = __dadd_rn(__dadd_rn(pxy, pxy), c1) /
                         __dadd_rn(__dadd_rn(__dmul_rn(mux, mux), __dmul_rn(muy, muy)), c1);
      scs += cs;
      sss += cs * lum;
    }
  }
  if (block_sum_pair(scs, sss, red)) {
    double* o = partial + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    o[0] = scs;
    o[1] = sss;
  }
}

struct FinalArgs : MsPartials {
  double count;                     // 3 * H * W: the elements behind the two integer sums
  int qblocks;
};

// one block per image: every sum is thread-strided, then wave-reduced, then the four waves in order
__global__ __launch_bounds__(256) void metrics_final_kernel(const unsigned long long* __restrict__ qpartial,
                                                           const double* __restrict__ spartial, FinalArgs fa,
                                                           double* __restrict__ out) {
  __shared__ double red[2][4];
  const int n = blockIdx.x;
  for (int item = 0; item <= kMsScales; ++item) {
    double a = 0.0, b = 0.0;
    if (item == 0) {
      unsigned long long l1 = 0, se = 0;
      for (int i = threadIdx.x; i < fa.qblocks; i += 256) {
        l1 += qpartial[((long long)n * fa.qblocks + i) * 2];
        se += qpartial[((long long)n * fa.qblocks + i) * 2 + 1];
      }
      a = (double)l1;          // integers below 2^53: every double sum that follows is exact
      b = (double)se;
    } else {
      const int j = item - 1;
      const double* p = spartial + (fa.scale_off[j] + (long long)n * fa.scale_cnt[j]) * 2;
      for (int i = threadIdx.x; i < fa.scale_cnt[j]; i += 256) {
        a += p[2 * i];
        b += p[2 * i + 1];
      }
    }
    if (block_sum_pair(a, b, red)) {
      double* o = out + (long long)n * kOutPerImage;
      if (item == 0) {
        o[0] = a;
        o[1] = b;
        o[2] = fa.count;
        o[3] = 0.0;
      } else {
        o[4 + item - 1] = a / fa.pos[item - 1];
        o[4 + kMsScales + item - 1] = b / fa.pos[item - 1];
      }
    }
    __syncthreads();
  }
}

// ---- host side: geometry and workspace layout -------------------------------------------------------------------------------
struct MetricsPlan : MsGeometry {
  int qblocks;
  size_t off_y, off_qpartial, off_spartial, bytes;
  FinalArgs fa;
};

static int metrics_quant_blocks(long long HW) {
  long long b = (HW + 1023) / 1024;      // >= 4 pixels per thread
  if (b < 1) b = 1;
  if (b > kQuantBlocksMax) b = kQuantBlocksMax;
  return (int)b;
}

static void metrics_plan(int N, int H, int W, MetricsPlan& p) {
  const long long pairs = ms_geometry(N, H, W, p, p.fa);
  p.qblocks = metrics_quant_blocks((long long)H * W);
  p.fa.qblocks = p.qblocks;
  p.fa.count = 3.0 * (double)H * (double)W;
  p.off_y = align_up(p.plane_floats * sizeof(float), 256);
  p.off_qpartial = 2 * p.off_y;
  p.off_spartial = p.off_qpartial + align_up((size_t)N * p.qblocks * 2 * sizeof(unsigned long long), 256);
  p.bytes = p.off_spartial + align_up((size_t)pairs * 2 * sizeof(double), 256);
}

// the tile grid: msssim_scale_kernel at scale 1, ceil((H - 10) / 16) x ceil((W - 10) / 64) tiles
static const char* metrics_shape_error(int N, int H, int W, int C) { return ms_shape_error(N, H, W, C, kHalo); }

static size_t cls_partial_bytes(int N, int qblocks, int n_classes) {
  return align_up((size_t)N * qblocks * (n_classes + 1) * 3 * sizeof(unsigned long long), 256);
}

// both entry points: label == nullptr is jpdse_eval_metrics; with a label the class partials sit behind the plain workspace
static int metrics_run(int32_t dtype_fake, int32_t dtype_real, int32_t N, int32_t H, int32_t W, int32_t C, const void* fake,
                       const void* real, const float* label, int32_t n_classes, const double* mean, const double* std,
                       double* out, int64_t* cls, void* ws, size_t ws_bytes, void* stream) {
  JPDSE_REQUIRE(dtype_fake == JPDSE_F32 || dtype_fake == JPDSE_BF16, "eval_metrics: fake must be fp32 or bf16");
  JPDSE_REQUIRE(dtype_real == JPDSE_F32, "eval_metrics: real must be fp32");
  JPDSE_REQUIRE(fake && real && mean && std && out, "eval_metrics: null argument");
  if (const char* msg = metrics_shape_error(N, H, W, C))
    return set_error(JPDSE_EINVAL, "eval_metrics: %s (N %d, H %d, W %d, C %d)", msg, N, H, W, C);
  MetricsPlan p;
  metrics_plan(N, H, W, p);
  const size_t need = p.bytes + (label ? cls_partial_bytes(N, p.qblocks, n_classes) : 0);
  if (ws == nullptr || ws_bytes < need) return set_error(JPDSE_EWORKSPACE, "eval_metrics: workspace too small");
  JPDSE_REQUIRE(((uintptr_t)ws & 15) == 0, "eval_metrics: workspace not 16-byte aligned");
  hipStream_t s = as_stream(stream);
  char* base = reinterpret_cast<char*>(ws);
  float* px = reinterpret_cast<float*>(base);
  float* py = reinterpret_cast<float*>(base + p.off_y);
  unsigned long long* qpartial = reinterpret_cast<unsigned long long*>(base + p.off_qpartial);
  double* spartial = reinterpret_cast<double*>(base + p.off_spartial);
  unsigned long long* cpartial = reinterpret_cast<unsigned long long*>(base + p.bytes);

  QuantParams qp = {};
  for (int c = 0; c < 3; ++c) { qp.mean[c] = mean[c]; qp.std[c] = std[c]; }
  const GaussWin g = gauss_window();
  const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  const long long HW = (long long)H * W;
  const int cs = cpad(C);

  if (int rc = by_dtype(dtype_fake, [&](auto tag) {
        using T = decltype(tag);
        if (!label)
          return launch256("eval_metrics(quantise)", metrics_quant_kernel<T, false>, dim3(p.qblocks, N), stream,
                           cptr<T>(fake), cptr<float>(real), cs, HW, qp, px, py, qpartial, nullptr, 0, nullptr);
        const size_t lds = (size_t)4 * (n_classes + 1) * 3 * sizeof(unsigned long long);
        hipLaunchKernelGGL((metrics_quant_kernel<T, true>), dim3(p.qblocks, N), dim3(256), lds, s, cptr<T>(fake),
                           cptr<float>(real), cs, HW, qp, px, py, qpartial, label, n_classes, cpartial);
        return check_launch("eval_metrics_sem(quantise)");
      }))
    return rc;
  for (int j = 0; j < kMsScales; ++j) {
    const float* xj = px + p.plane_off[j];
    const float* yj = py + p.plane_off[j];
    hipLaunchKernelGGL(msssim_scale_kernel, dim3(p.tx[j], p.ty[j], N * 3), dim3(256), 0, s, xj, yj, p.Hs[j], p.Ws[j], g, c1,
                       c2, spartial + p.fa.scale_off[j] * 2);
    if (int rc = check_launch("eval_metrics(scale)")) return rc;
    if (j + 1 < kMsScales) {
      const long long total = (long long)N * 3 * p.Hs[j + 1] * p.Ws[j + 1];
      hipLaunchKernelGGL(msssim_down_kernel, dim3(ew_blocks(total)), dim3(256), 0, s, xj, yj, p.Hs[j], p.Ws[j],
                         px + p.plane_off[j + 1], py + p.plane_off[j + 1], total);
      if (int rc = check_launch("eval_metrics(downsample)")) return rc;
    }
  }
  hipLaunchKernelGGL(metrics_final_kernel, dim3(N), dim3(256), 0, s, qpartial, spartial, p.fa, out);
  if (int rc = check_launch("eval_metrics(final)")) return rc;
  if (label) {
    const int entries = (n_classes + 1) * 3;
    hipLaunchKernelGGL(metrics_cls_final_kernel, dim3((entries + 63) / 64, N), dim3(256), 0, s, cpartial, p.qblocks, entries,
                       reinterpret_cast<long long*>(cls));
    return check_launch("eval_metrics_sem(final)");
  }
  return JPDSE_OK;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_eval_metrics_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (metrics_shape_error(N, H, W, C)) return 0;
  MetricsPlan p;
  metrics_plan(N, H, W, p);
  return p.bytes;
}

size_t jpdse_eval_metrics_sem_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_classes) {
  if (metrics_shape_error(N, H, W, C) || n_classes < 1 || n_classes > kClassesMax) return 0;
  MetricsPlan p;
  metrics_plan(N, H, W, p);
  return p.bytes + cls_partial_bytes(N, p.qblocks, n_classes);
}

int jpdse_eval_metrics(int32_t dtype_fake, int32_t dtype_real, int32_t N, int32_t H, int32_t W, int32_t C, const void* fake,
                       const void* real, const double* mean, const double* std, double* out, void* ws, size_t ws_bytes,
                       void* stream) {
  return metrics_run(dtype_fake, dtype_real, N, H, W, C, fake, real, nullptr, 0, mean, std, out, nullptr, ws, ws_bytes, stream);
}

int jpdse_eval_metrics_sem(const jpdse_eval_metrics_sem_args* a) {
  JPDSE_REQUIRE(a != nullptr, "eval_metrics_sem: null argument struct");
  JPDSE_REQUIRE(a->label && a->cls, "eval_metrics_sem: null argument");
  JPDSE_REQUIRE(a->n_classes >= 1 && a->n_classes <= kClassesMax, "eval_metrics_sem: n_classes %d outside [1, %d]",
                a->n_classes, kClassesMax);
  return metrics_run(a->dtype_fake, a->dtype_real, a->N, a->H, a->W, a->C, a->fake, a->real, a->label, a->n_classes, a->mean,
                     a->std, a->out, a->cls, a->ws, a->ws_bytes, a->stream);
}

}  // extern "C"
