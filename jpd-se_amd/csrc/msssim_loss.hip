// MS-SSIM as a training distortion: G_Distortion = mean_n (1 - ms_ssim_n) on the de-normalised, UN-quantised images
// (u = v * std_c + mean_c, L = 1, C1 = 1e-4, C2 = 9e-4) and its gradient w.r.t. the generator's output.  Entry point:
// include/jpdse.h, "MS-SSIM training loss"; definition and derivation: DESIGN.md 4.6.  The structure is that of the
// evaluation pass (metrics.hip): 11x11 Gaussian window (sigma 1.5, "valid"), five scales linked by a 2x2
// mean, per channel.  The window, the tile geometry, the centred staging, the separable filter up to the filtered moments,
// the downsample, the block sum and the host geometry are those of metrics.hip, from msssim_core.h; the per-position
// arithmetic is this file's own (unfused throughout; jpdse_eval_metrics' differs in its bits, which are a contract).
//
// Kernels, in launch order (forward: 11 launches, with the gradient: 22):
//   msl_planes_kernel      fake, real (NHWC) -> planar fp32 planes of u, [N][3][H][W] (scale 1)
//   msl_scale_kernel<0>    one per scale: LDS tile + halo, separable 11-tap filter of x, y, x^2, y^2, xy, cs / ssim per
//                          position, one (cs, ssim) partial pair per block
//   msssim_down_kernel     2x2 mean -> next scale's planes (msssim_core.h)
//   msl_final_kernel       partials -> per-scale means, ms_ssim_n and the factors a_j / positions_j per image, in a fixed
//                          order; writes the loss slot
//   msl_scale_kernel<1|2>  (gradient) the same filter again, now writing three coefficient maps per position on the valid
//                          region: the partials of the position's cs (<1>) or ssim (<2>, scale 5) w.r.t. mu_x, E_w[x^2] and
//                          E_w[xy], times the image's factor of that scale
//   msl_back_kernel        (gradient) one per scale, coarsest first: the three maps correlated with the window in "full"
//                          mode (the transpose of the valid filter), dx = G_mu + 2 x G_xx + y G_xy, plus a quarter of the
//                          coarser scale's gradient (the transpose of the 2x2 mean) -> gradient plane of the scale
//   msl_pack_kernel        (gradient) scale-1 plane * (-std_c * scale / N) -> NHWC in fake's dtype, padding lanes 0
// No atomics: every output element has one writer and every sum a fixed order, so two calls are bit-identical.
//
// Cancellation: the forward / coefficient filter centres every tile about its own pivot (the tile's first pixel, per image of
// the pair), as the evaluation pass does: it costs two subtractions per staged pixel, identical images give cs = ssim = 1
// bit for bit and a constant tile variance exactly 0.  The coefficient maps themselves are absolute quantities (partials
// w.r.t. the un-shifted moments), so the back-correlation is not centred; its cancellation is eps_fp32 * mu / contrast.
// The filters run in fp32; the per-position cs / ssim, the coefficients and every sum over positions are fp64.
#include "msssim_core.h"

namespace jpdse {

constexpr int kStats = 11;               // per image: cs_1..5, ssim_1..5, ms_ssim

struct MslNorm { float mean[3]; float std[3]; };

// fake, real: NHWC [N][H][W][8] of T; one thread per pixel; planes x (fake) / y (real): [N][3][HW] of u = v * std + mean
template <typename T>
__global__ __launch_bounds__(256) void msl_planes_kernel(const T* __restrict__ fake, const T* __restrict__ real, long long HW,
                                                        long long total, MslNorm nm, float* __restrict__ px,
                                                        float* __restrict__ py) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    float a[Vec16<T>::N], b[Vec16<T>::N];
    Vec16<T>::load(fake + i * 8, a);       // the first 16 bytes of the pixel hold its three channels in either dtype
    Vec16<T>::load(real + i * 8, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      px[(n * 3 + c) * HW + p] = fmaf(a[c], nm.std[c], nm.mean[c]);
      py[(n * 3 + c) * HW + p] = fmaf(b[c], nm.std[c], nm.mean[c]);
    }
  }
}

// x, y: planes [NC][Hs][Ws]; grid (tiles_x, tiles_y, NC).  LDS: 2 staged tiles + 5 horizontally filtered planes = 48.7 KB,
// three blocks per CU.  Every LDS access of a wave is 64 consecutive dwords of one row (plus a tap offset): conflict free.
// kMode 0: partial[NC][tiles_y][tiles_x][2] doubles (sum cs, sum ssim over the block's valid positions).
// kMode 1 / 2: fac[n * 5 + scale] = a_j / positions_j of the image; coef: three maps [3][NC][Ho][Wo] (d/d mu_x, d/d E[x^2],
// d/d E[xy]) of fac * cs (1) or fac * ssim (2).
template <int kMode>
__global__ __launch_bounds__(256) void msl_scale_kernel(const float* __restrict__ x, const float* __restrict__ y, int Hs, int Ws,
                                                       GaussWin g, double c1, double c2, double* __restrict__ partial,
                                                       const double* __restrict__ fac, int scale, float* __restrict__ coef,
                                                       long long map_stride) {
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
  double f = 0.0;
  if constexpr (kMode != 0) f = fac[(blockIdx.z / 3) * kMsScales + scale];
  double scs = 0.0, sss = 0.0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if (x0 + c < Wo && y0 + r0 + o < Ho) {
      // own epilogue, not metrics.hip's: unfused throughout, so that identical images give numerator == denominator bit for bit
      const double mx = acc[0][o], my = acc[1][o];
      const double vxx = __dsub_rn((double)acc[2][o], __dmul_rn(mx, mx));
      const double vyy = __dsub_rn((double)acc[3][o], __dmul_rn(my, my));
      const double vxy = __dsub_rn((double)acc[4][o], __dmul_rn(mx, my));
      const double mux = (double)pvx + mx, muy = (double)pvy + my;
      const double B = __dadd_rn(__dadd_rn(vxx, vyy), c2);
      const double cs = __dadd_rn(__dadd_rn(vxy, vxy), c2) / B;
      const double pxy = __dmul_rn(mux, muy);
      const double Q = __dadd_rn(__dadd_rn(__dmul_rn(mux, mux), __dmul_rn(muy, muy)), c1);
      const double lum = __dadd_rn(__dadd_rn(pxy, pxy), c1) / Q;
      if constexpr (kMode == 0) {
        scs += cs;
        sss += cs * lum;
      } else {
        float gm = 0.f, gxx = 0.f, gxy = 0.f;     // an image under the zero rule (f == 0) gets exact zeros
        if (f != 0.0) {
          const double ib = f / B;
          // d cs / d mu_x = 2 (cs mu_x - mu_y) / B,  d cs / d E[x^2] = -cs / B,  d cs / d E[xy] = 2 / B
          double dm = 2.0 * (cs * mux - muy) * ib, dxx = -cs * ib, dxy = 2.0 * ib;
          if constexpr (kMode == 2) {
            // ssim = cs * lum:  d lum / d mu_x = 2 (mu_y - lum mu_x) / Q
            dm = lum * dm + cs * 2.0 * (muy - lum * mux) * (f / Q);
            dxx *= lum;
            dxy *= lum;
          }
          gm = (float)dm;
          gxx = (float)dxx;
          gxy = (float)dxy;
        }
        const long long at = ((long long)blockIdx.z * Ho + (y0 + r0 + o)) * Wo + (x0 + c);
        coef[at] = gm;
        coef[map_stride + at] = gxx;
        coef[2 * map_stride + at] = gxy;
      }
    }
  }
  if constexpr (kMode == 0) {
    if (block_sum_pair(scs, sss, red)) {
      double* o = partial + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
      o[0] = scs;
      o[1] = sss;
    }
  }
}

struct MslFinalArgs : MsPartials {
  double weight[kMsScales];
  int N;
};

// ONE block: per image and scale a thread-strided sum, wave-reduced, the four waves in order; then thread 0 forms ms_ssim_n,
// the factors and the loss.  stats (optional): [N][11]; fac: [N][5] = w_j ms_ssim_n / mean_j / positions_j, 0 under the zero rule
__global__ __launch_bounds__(256) void msl_final_kernel(const double* __restrict__ spartial, MslFinalArgs fa,
                                                       double* __restrict__ fac, double* __restrict__ stats,
                                                       float* __restrict__ out) {
  __shared__ double red[2][4];
  double loss = 0.0;                     // thread 0 only
  for (int n = 0; n < fa.N; ++n) {
    double mean[kMsScales], ssim5 = 0.0; // thread 0 only: cs_1..5
    for (int j = 0; j < kMsScales; ++j) {
      double a = 0.0, b = 0.0;
      const double* p = spartial + (fa.scale_off[j] + (long long)n * fa.scale_cnt[j]) * 2;
      for (int i = threadIdx.x; i < fa.scale_cnt[j]; i += 256) {
        a += p[2 * i];
        b += p[2 * i + 1];
      }
      if (block_sum_pair(a, b, red)) {
        const double cs = a / fa.pos[j];
        const double ss = b / fa.pos[j];
        mean[j] = cs;
        if (j == kMsScales - 1) ssim5 = ss;
        if (stats) {
          stats[(long long)n * kStats + j] = cs;
          stats[(long long)n * kStats + kMsScales + j] = ss;
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      mean[kMsScales - 1] = ssim5;       // the five means of the product: cs_1..4, ssim_5
      bool positive = true;
      for (int j = 0; j < kMsScales; ++j) positive = positive && mean[j] > 0.0;
      double ms = 0.0;
      if (positive) {
        ms = 1.0;
        for (int j = 0; j < kMsScales; ++j) ms *= pow(mean[j], fa.weight[j]);
      }
      for (int j = 0; j < kMsScales; ++j)
        fac[(long long)n * kMsScales + j] = positive ? fa.weight[j] * ms / mean[j] / fa.pos[j] : 0.0;
      if (stats) stats[(long long)n * kStats + 2 * kMsScales] = ms;
      loss += 1.0 - ms;
    }
  }
  if (threadIdx.x == 0) out[0] = (float)(loss / (double)fa.N);
}

// coef: three maps [3][NC][Ho][Wo] of the scale; x, y: its planes [NC][Hs][Ws]; up: the coarser scale's gradient plane
// [NC][Hu][Wu] or nullptr; dst: [NC][Hs][Ws].  grid (ceil(Ws / 64), ceil(Hs / 16), NC).  Pixel p receives sum_k w[k] g(p - k)
// over the positions p - k inside the valid region: the staged tile starts 10 positions before the block's first pixel and
// is zero outside [0, Ho) x [0, Wo); the window is symmetric, so the taps read forward as in the valid filter.
// LDS: 3 staged maps (23.1 KB) + 3 horizontally filtered ones (20.0 KB); row accesses as in msl_scale_kernel.
__global__ __launch_bounds__(256) void msl_back_kernel(const float* __restrict__ coef, long long map_stride,
                                                      const float* __restrict__ x, const float* __restrict__ y, int Hs, int Ws,
                                                      GaussWin g, const float* __restrict__ up, int Hu, int Wu,
                                                      float* __restrict__ dst) {
  __shared__ float sg[3][kSH][kSW];
  __shared__ float hg[3][kSH][kTW];
  const int Ho = Hs - kHalo, Wo = Ws - kHalo;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const long long nc = blockIdx.z;
  const float* cp = coef + nc * Ho * Wo;
  for (int i = threadIdx.x; i < kSH * kSW; i += 256) {
    const int r = i / kSW, c = i - r * kSW;
    const int qy = y0 - kHalo + r, qx = x0 - kHalo + c;
    float a = 0.f, b = 0.f, d = 0.f;
    if (qy >= 0 && qy < Ho && qx >= 0 && qx < Wo) {
      const long long at = (long long)qy * Wo + qx;
      a = cp[at];
      b = cp[map_stride + at];
      d = cp[2 * map_stride + at];
    }
    sg[0][r][c] = a;
    sg[1][r][c] = b;
    sg[2][r][c] = d;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSH * kTW; i += 256) {
    const int r = i >> 6, c = i & 63;
    float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float w = g.w[k];
      a = fmaf(w, sg[0][r][c + k], a);
      b = fmaf(w, sg[1][r][c + k], b);
      d = fmaf(w, sg[2][r][c + k], d);
    }
    hg[0][r][c] = a;
    hg[1][r][c] = b;
    hg[2][r][c] = d;
  }
  __syncthreads();
  float acc[3][4];
  vertical_pass<3>(hg, g, acc);
  const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;   // acc[q][o] is position (r0 + o, c): must match vertical_pass
  const int gx = x0 + c;
  if (gx >= Ws) return;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int gy = y0 + r0 + o;
    if (gy < Hs) {
      const long long at = (nc * Hs + gy) * Ws + gx;
      float d = acc[0][o] + 2.f * x[at] * acc[1][o] + y[at] * acc[2][o];
      // transpose of the 2x2 mean: a quarter to each of its four pixels, nothing to a dropped odd row or column
      if (up != nullptr && (gy >> 1) < Hu && (gx >> 1) < Wu) d += 0.25f * up[(nc * Hu + (gy >> 1)) * Wu + (gx >> 1)];
      dst[at] = d;
    }
  }
}

// scale-1 gradient plane [N][3][HW] -> NHWC [N][HW][8] of T, times k[c] = -std_c * scale / N; padding lanes 0
template <typename T>
__global__ __launch_bounds__(256) void msl_pack_kernel(const float* __restrict__ gp, long long HW, long long total, float k0,
                                                      float k1, float k2, T* __restrict__ dfake) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    const float* s = gp + n * 3 * HW + p;
    const float v0 = s[0] * k0, v1 = s[HW] * k1, v2 = s[2 * HW] * k2;
    if constexpr (Vec16<T>::N == 8) {
      const float v[8] = {v0, v1, v2, 0.f, 0.f, 0.f, 0.f, 0.f};
      Vec16<T>::store(dfake + i * 8, v);
    } else {
      const float lo[4] = {v0, v1, v2, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
      Vec16<T>::store(dfake + i * 8, lo);
      Vec16<T>::store(dfake + i * 8 + 4, hi);
    }
  }
}

// ---- host side: geometry and workspace layout -------------------------------------------------------------------------------
struct MslPlan : MsGeometry {
  size_t map_floats;               // one coefficient map of scale 1 (the largest)
  size_t off_y, off_spartial, off_fac, off_coef, off_grad, bytes;
  MslFinalArgs fa;
};

static void msl_plan(int N, int H, int W, bool with_grad, MslPlan& p) {
  const long long pairs = ms_geometry(N, H, W, p, p.fa);
  for (int j = 0; j < kMsScales; ++j) p.fa.weight[j] = kMsWeights[j];
  p.fa.N = N;
  p.map_floats = align_up((size_t)N * 3 * (H - kHalo) * (W - kHalo), 64);
  p.off_y = align_up(p.plane_floats * sizeof(float), 256);
  p.off_spartial = 2 * p.off_y;
  p.off_fac = p.off_spartial + align_up((size_t)pairs * 2 * sizeof(double), 256);
  p.off_coef = p.off_fac + align_up((size_t)N * kMsScales * sizeof(double), 256);
  p.off_grad = p.off_coef;
  p.bytes = p.off_coef;
  if (with_grad) {
    p.off_grad = p.off_coef + align_up(3 * p.map_floats * sizeof(float), 256);
    p.bytes = p.off_grad + p.off_y;
  }
}

// the tile grid: msl_back_kernel at scale 1 covers the full plane, ceil(H / 16) x ceil(W / 64) tiles
static const char* msl_shape_error(int N, int H, int W, int C) { return ms_shape_error(N, H, W, C, 0); }

// everything that can be refused before any launch
static int msl_check(const jpdse_msssim_loss_args* a) {
  JPDSE_REQUIRE(a != nullptr, "msssim_loss: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "msssim_loss: bad dtype %d (fake and real are both fp32 or both bf16)", a->dtype);
  JPDSE_REQUIRE(a->fake && a->real && a->mean && a->std && a->out, "msssim_loss: null argument");
  if (const char* msg = msl_shape_error(a->N, a->H, a->W, a->C))
    return set_error(JPDSE_EINVAL, "msssim_loss: %s (N %d, H %d, W %d, C %d)", msg, a->N, a->H, a->W, a->C);
  JPDSE_REQUIRE(a->dfake == nullptr || a->scale == a->scale, "msssim_loss: scale is NaN");
  return JPDSE_OK;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_msssim_loss_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C, int32_t with_grad) {
  if (msl_shape_error(N, H, W, C)) return 0;
  MslPlan p;
  msl_plan(N, H, W, with_grad != 0, p);
  return p.bytes;
}

int jpdse_msssim_loss(const jpdse_msssim_loss_args* a) {
  if (int rc = msl_check(a)) return rc;
  const int N = a->N, H = a->H, W = a->W;
  const bool with_grad = a->dfake != nullptr;
  MslPlan p;
  msl_plan(N, H, W, with_grad, p);
  if (a->ws == nullptr || a->ws_bytes < p.bytes)
    return set_error(JPDSE_EWORKSPACE, "msssim_loss: workspace too small (%zu bytes, %zu needed)", a->ws_bytes, p.bytes);
  JPDSE_REQUIRE(((uintptr_t)a->ws & 15) == 0, "msssim_loss: workspace not 16-byte aligned");
  hipStream_t s = as_stream(a->stream);
  char* base = reinterpret_cast<char*>(a->ws);
  float* px = reinterpret_cast<float*>(base);
  float* py = reinterpret_cast<float*>(base + p.off_y);
  double* spartial = reinterpret_cast<double*>(base + p.off_spartial);
  double* fac = reinterpret_cast<double*>(base + p.off_fac);
  float* coef = reinterpret_cast<float*>(base + p.off_coef);
  float* grad = reinterpret_cast<float*>(base + p.off_grad);

  MslNorm nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = (float)a->mean[c]; nm.std[c] = (float)a->std[c]; }
  const GaussWin g = gauss_window();
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  const long long HW = (long long)H * W, total = (long long)N * HW;

  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        return ew_launch("msssim_loss(planes)", msl_planes_kernel<T>, total, a->stream, cptr<T>(a->fake), cptr<T>(a->real), HW,
                         total, nm, px, py);
      }))
    return rc;
  for (int j = 0; j < kMsScales; ++j) {
    const float* xj = px + p.plane_off[j];
    const float* yj = py + p.plane_off[j];
    if (int rc = launch256("msssim_loss(scale)", msl_scale_kernel<0>, dim3(p.tx[j], p.ty[j], N * 3), a->stream, xj, yj, p.Hs[j],
                           p.Ws[j], g, c1, c2, spartial + p.fa.scale_off[j] * 2, nullptr, j, nullptr, 0))
      return rc;
    if (j + 1 < kMsScales) {
      const long long n_down = (long long)N * 3 * p.Hs[j + 1] * p.Ws[j + 1];
      if (int rc = ew_launch("msssim_loss(downsample)", msssim_down_kernel, n_down, a->stream, xj, yj, p.Hs[j], p.Ws[j],
                             px + p.plane_off[j + 1], py + p.plane_off[j + 1], n_down))
        return rc;
    }
  }
  if (int rc = launch256("msssim_loss(final)", msl_final_kernel, dim3(1), a->stream, spartial, p.fa, fac, a->stats, a->out))
    return rc;
  if (!with_grad) return JPDSE_OK;

  for (int j = kMsScales - 1; j >= 0; --j) {
    const float* xj = px + p.plane_off[j];
    const float* yj = py + p.plane_off[j];
    const long long stride = (long long)N * 3 * (p.Hs[j] - kHalo) * (p.Ws[j] - kHalo);
    auto* coef_kernel = j == kMsScales - 1 ? msl_scale_kernel<2> : msl_scale_kernel<1>;
    if (int rc = launch256("msssim_loss(coefficients)", coef_kernel, dim3(p.tx[j], p.ty[j], N * 3), a->stream, xj, yj, p.Hs[j],
                           p.Ws[j], g, c1, c2, nullptr, fac, j, coef, stride))
      return rc;
    const bool top = j == kMsScales - 1;
    const float* up = top ? nullptr : grad + p.plane_off[j + 1];
    if (int rc = launch256("msssim_loss(back)", msl_back_kernel, dim3((p.Ws[j] + kTW - 1) / kTW, (p.Hs[j] + kTH - 1) / kTH, N * 3),
                           a->stream, coef, stride, xj, yj, p.Hs[j], p.Ws[j], g, up, top ? 0 : p.Hs[j + 1], top ? 0 : p.Ws[j + 1],
                           grad + p.plane_off[j]))
      return rc;
  }
  const float k = -a->scale / (float)N;
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    return ew_launch("msssim_loss(pack)", msl_pack_kernel<T>, total, a->stream, grad, HW, total, k * nm.std[0], k * nm.std[1],
                     k * nm.std[2], mptr<T>(a->dfake));
  });
}

}  // extern "C"
