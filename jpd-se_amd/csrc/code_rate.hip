// Rate term of the learned codec's training (no reference counterpart: the reference has no coded stream and no rate term):
// the expected length of the code under a static, Laplace-smoothed form of the entropy coder's context model, and its
// gradient w.r.t. the binarizer's tanh output.  Definition: DESIGN.md 4.10.  Entry point: include/jpdse.h, "context-model
// rate term".
//
// The context of a symbol depends on the code alone (the coder's own rule, context_of of range_coder.h, over the bits b > 0
// of the same (image, channel) stream), so unlike the coder nothing here is serial.  Kernels, in launch order:
//   rate_count_kernel   lane = channel, as in entropy.hip: the 64 lanes of a wave read 64 neighbouring channels of a pixel.
//                       grid (row chunks, 64-channel groups, images), four waves, wave w takes the chunk's rows w, w + 4, ...
//                       Every lane counts (ctx, bit) pairs in an LDS column of its own; the four waves' columns are summed
//                       and added to counts[n][c][ctx][bit] with integer atomics: the counts do not depend on the order.
//   rate_cost_kernel    the same grid and walk.  The block turns the counts of its 64 streams into 32 costs per stream in
//                       LDS (cost = -log2 of the Laplace estimate), adds up the element costs, writes the gradient and one
//                       partial of the value per block.
//   rate_final_kernel   ONE block: the partials of an image in a fixed order (fp64), per_image and the value slot.
// Lanes c >= C of the last group hold no stream: they load nothing, count nothing, and write zeros into the padding lanes
// C <= c < CPAD(C) of the gradient.  Every loop is bounded by the shape.
#include "range_coder.h"

namespace jpdse {

constexpr int kRateRows = 8;              // rows of a block's chunk: two per wave
constexpr int kRateCol = 65;              // LDS row pitch in dwords: entry e of lane l at e * 65 + l, conflict free both when
                                          // a wave touches one entry of 64 lanes and when it reads 32 entries of one lane
constexpr long long kRateMaxHW = 1LL << 30;

static bool rate_shape_ok(int N, int H, int W, int C) {
  return N > 0 && H > 0 && W > 0 && C > 0 && N <= 65535 && C <= 64 * 65535 && (long long)H * W <= kRateMaxHW;
}
static inline int rate_chunks(int H) { return (H + kRateRows - 1) / kRateRows; }
static inline int rate_groups(int C) { return (C + 63) / 64; }
static inline size_t rate_counts_bytes(int N, int C) { return align_up((size_t)N * C * 32 * sizeof(int32_t), 256); }

// Row y of the stream whose first element is at `img` (lane's channel of image n, pixel pitch Cs): f(x, ctx, bit) for
// x = 0 .. W-1.  The row and the one above are read as words of 32 bits (independent loads); `active` == false: no load, all
// bits 0.  Wave-uniform control flow.
template <typename T, typename F>
__device__ __forceinline__ void rate_walk_row(const T* __restrict__ img, int y, int W, int Cs, bool active, F&& f) {
  const int nw = (W + 31) >> 5;
  auto word = [&](int yy, int j) -> uint32_t {
    uint32_t w = 0;
    if (active && yy >= 0 && j < nw) w = load_bit_word(img + ((long long)yy * W + 32 * j) * Cs, Cs, min(32, W - 32 * j));
    return w;
  };
  uint32_t upw = word(y - 1, 0), left = 0, ul = 0;
  for (int j = 0; j < nw; ++j) {
    const uint32_t nextw = word(y - 1, j + 1);
    const uint32_t urw = (upw >> 1) | (nextw << 31);
    const uint32_t inw = word(y, j);
    const int kmax = min(32, W - 32 * j);
    for (int k = 0; k < kmax; ++k) {
      const uint32_t bit = (inw >> k) & 1u, up = (upw >> k) & 1u;
      f(32 * j + k, context_of(left, up, ul, (urw >> k) & 1u), bit);
      ul = up;
      left = bit;
    }
    upw = nextw;
  }
}

// counts: int32 [N][C][16][2], zeroed by the host before the launch.  grid (chunks, groups, N)
template <typename T>
__global__ void __launch_bounds__(256) rate_count_kernel(const T* __restrict__ b, int32_t* __restrict__ counts, int H, int W,
                                                         int C, int Cs) {
  __shared__ uint32_t cnt[4][32 * kRateCol];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.y * 64, c = c0 + lane, n = blockIdx.z;
  const bool active = c < C;
  uint32_t* col = cnt[wave] + lane;
  for (int e = 0; e < 32; ++e) col[e * kRateCol] = 0;       // the lane's own column: no barrier needed before it is used
  const T* img = b + (long long)n * H * W * Cs + c;
  const int y0 = blockIdx.x * kRateRows, y1 = min(H, y0 + kRateRows);
  for (int y = y0 + wave; y < y1; y += 4)
    rate_walk_row(img, y, W, Cs, active, [&](int, uint32_t ctx, uint32_t bit) {
      if (active) col[(ctx * 2 + bit) * kRateCol] += 1;
    });
  __syncthreads();
  // the 64 x 32 counters of the block are contiguous in `counts`: thread i takes i, i + 256, ... (lane i >> 5, entry i & 31)
  int32_t* dst = counts + ((long long)n * C + c0) * 32;
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int l = i >> 5, e = i & 31;
    if (c0 + l < C) {
      const uint32_t v = (cnt[0][e * kRateCol + l] + cnt[1][e * kRateCol + l]) + (cnt[2][e * kRateCol + l] + cnt[3][e * kRateCol + l]);
      if (v != 0) atomicAdd(dst + i, (int32_t)v);
    }
  }
}

// t == nullptr: hard mode; grad == nullptr: value only.  partial: [N][groups][chunks] floats.  gk = scale / (2 N pixels)
template <typename T>
__global__ void __launch_bounds__(256) rate_cost_kernel(const T* __restrict__ b, const T* __restrict__ t, T* __restrict__ grad,
                                                        const int32_t* __restrict__ counts, float* __restrict__ partial,
                                                        int H, int W, int C, int Cs, float gk) {
  __shared__ float cost[32 * kRateCol];      // entry 2 ctx + bit of lane l at (2 ctx + bit) * 65 + l
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.y * 64, c = c0 + lane, n = blockIdx.z;
  const bool active = c < C, padding = !active && c < Cs;
  const int32_t* src = counts + ((long long)n * C + c0) * 32;
  const float inv_ln2 = 1.44269504088896340736f;
  for (int i = threadIdx.x; i < 64 * 16; i += 256) {
    const int l = i >> 4, k = i & 15;
    if (c0 + l < C) {
      // -log2((n1 + 1) / (n0 + n1 + 2)) = log2(1 + (n0 + 1) / (n1 + 1)): log1p keeps its relative accuracy when p -> 1
      const float a0 = (float)(src[2 * i] + 1), a1 = (float)(src[2 * i + 1] + 1);
      cost[(2 * k) * kRateCol + l] = log1pf(a1 / a0) * inv_ln2;
      cost[(2 * k + 1) * kRateCol + l] = log1pf(a0 / a1) * inv_ln2;
    }
  }
  __syncthreads();
  const long long base = (long long)n * H * W * Cs + c;
  const float* col = cost + lane;
  float acc = 0.f;
  const int y0 = blockIdx.x * kRateRows, y1 = min(H, y0 + kRateRows);
  for (int y = y0 + wave; y < y1; y += 4) {
    const long long row = base + (long long)y * W * Cs;
    rate_walk_row(b + base, y, W, Cs, active, [&](int x, uint32_t ctx, uint32_t bit) {
      const long long at = row + (long long)x * Cs;
      if (active) {
        const float k0 = col[(ctx * 2) * kRateCol], k1 = col[(ctx * 2 + 1) * kRateCol];
        const float tv = t != nullptr ? ElemOps<T>::ld(t + at) : (bit ? 1.f : -1.f);
        acc += 0.5f * ((1.f + tv) * k1 + (1.f - tv) * k0);
        if (grad != nullptr) ElemOps<T>::st(grad + at, (k1 - k0) * gk);
      } else if (padding && grad != nullptr) {
        ElemOps<T>::st(grad + at, 0.f);
      }
    });
  }
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[((long long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ONE block.  per image: a thread-strided fp64 sum of its `per` partials, wave-reduced, the four waves in order
__global__ void __launch_bounds__(256) rate_final_kernel(const float* __restrict__ partial, int N, int per, double pixels,
                                                         float* __restrict__ per_image, float* __restrict__ out) {
  __shared__ double red[4];
  double total = 0.0;                        // thread 0 only
  for (int n = 0; n < N; ++n) {
    const float* p = partial + (long long)n * per;
    double a = 0.0;
    for (int i = threadIdx.x; i < per; i += 256) a += (double)p[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double v = ((red[0] + red[1]) + (red[2] + red[3])) / pixels;
      if (per_image != nullptr) per_image[n] = (float)v;
      total += v;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(total / (double)N);
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_code_rate_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (!rate_shape_ok(N, H, W, C)) return 0;
  // the counts int32 [N][C][16][2] (also when the caller passes a buffer for them: one layout) and the block partials
  return rate_counts_bytes(N, C) + (size_t)N * rate_groups(C) * rate_chunks(H) * sizeof(float);
}

int jpdse_code_rate_loss(const jpdse_code_rate_args* a) {
  JPDSE_REQUIRE(a != nullptr, "code_rate_loss: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "code_rate_loss: bad dtype %d (b, t and grad are all fp32 or all bf16)", a->dtype);
  JPDSE_REQUIRE(a->b != nullptr, "code_rate_loss: null pointer b");
  JPDSE_REQUIRE(a->out != nullptr, "code_rate_loss: null pointer out");
  const int N = a->N, H = a->H, W = a->W, C = a->C;
  JPDSE_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "code_rate_loss: non-positive extent (N %d, H %d, W %d, C %d)", N, H, W, C);
  JPDSE_REQUIRE(a->pixels > 0, "code_rate_loss: non-positive pixels %lld", (long long)a->pixels);
  JPDSE_REQUIRE(rate_shape_ok(N, H, W, C),
                "code_rate_loss: shape beyond the limits (N %d <= 65535, C %d <= %d, H * W %lld <= 2^30)", N, C, 64 * 65535,
                (long long)H * W);
  JPDSE_REQUIRE(a->grad == nullptr || a->scale == a->scale, "code_rate_loss: scale is NaN");
  const size_t need = jpdse_code_rate_workspace_size(N, H, W, C);
  JPDSE_REQUIRE(a->ws != nullptr && a->ws_bytes >= need, "code_rate_loss: workspace too small (%zu bytes, %zu needed)",
                a->ws ? a->ws_bytes : (size_t)0, need);
  JPDSE_REQUIRE(((uintptr_t)a->ws & 15) == 0, "code_rate_loss: workspace not 16-byte aligned");

  const int Cs = cpad(C), groups = rate_groups(C), chunks = rate_chunks(H);
  int32_t* counts = mptr<int32_t>(a->ws);
  float* partial = reinterpret_cast<float*>(mptr<char>(a->ws) + rate_counts_bytes(N, C));
  const size_t count_bytes = (size_t)N * C * 32 * sizeof(int32_t);
  hipStream_t s = as_stream(a->stream);
  if (hipMemsetAsync(counts, 0, count_bytes, s) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "code_rate_loss: hipMemsetAsync failed");
  const dim3 grid(chunks, groups, N);
  const float gk = (float)((double)a->scale / (2.0 * (double)N * (double)a->pixels));
  if (int rc = by_dtype(a->dtype, [&](auto tag) {
        using T = decltype(tag);
        if (int rc = launch256("code_rate_loss(count)", rate_count_kernel<T>, grid, a->stream, cptr<T>(a->b), counts, H, W, C, Cs))
          return rc;
        return launch256("code_rate_loss(cost)", rate_cost_kernel<T>, grid, a->stream, cptr<T>(a->b), cptr<T>(a->t),
                         mptr<T>(a->grad), counts, partial, H, W, C, Cs, gk);
      }))
    return rc;
  if (a->counts != nullptr &&
      hipMemcpyAsync(a->counts, counts, count_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "code_rate_loss: hipMemcpyAsync failed");
  return launch256("code_rate_loss(final)", rate_final_kernel, dim3(1), a->stream, partial, N, groups * chunks,
                   (double)a->pixels, a->per_image, a->out);
}

}  // extern "C"
