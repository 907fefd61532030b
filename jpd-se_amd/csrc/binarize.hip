// Stochastic binarizer of the learned-codec encoder (reference ctu/quantizers/binarize.py:13-65), the statistics /
// export of the bitstream it produces (reference pix2pixHD_model.py:468-505) and the import of a stored bitstream (receiver side).  Entry points: include/jpdse.h, "learned codec".
//
// RNG contract: the noise of element e = (c*H + y)*W + x (logical NCHW index inside its image) of image
// n_global at training forward `draw` is word (e & 3) of Philox4x32-10(counter = (e >> 2, n_global, draw lo, draw hi),
// key = (seed lo, seed hi)), u = (word >> 8) * 2^-24.  A pure function of those inputs: the bits do not depend on how a
// batch is split over calls or ranks.
#include "common.h"

namespace jpdse {

#define GRID_STRIDE(idx, total)                                                         \
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < (total); \
       idx += (long long)gridDim.x * blockDim.x)

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) --------------------------------
__device__ __forceinline__ uint32_t philox4x32_10_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                       uint32_t k1, int word) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
}

// t, b: NHWC [N][H][W][Cs]; one thread per 16-byte vector.  train: b = ((1 - t) / 2 <= u) ? 1 : -1 (SoftSignFunction,
// binarize.py:19-24) on the stored t widened to fp32; eval: b = sign(t) (binarize.py:41-44, torch.sign: sign(0) = 0).
// u_override (fp32 NCHW [N][C][H][W]) replaces the generator when non-null.  Padding lanes of b are written as 0.
template <typename T>
__global__ void binarize_fwd_kernel(const T* __restrict__ t, T* __restrict__ b, int H, int W, int C, int Cs, int train,
                                    uint32_t k0, uint32_t k1, uint32_t d0, uint32_t d1, long long n_global0,
                                    const float* __restrict__ u_override, long long total_vec) {
  constexpr int VE = Vec16<T>::N;
  const int cv = Cs / VE;
  const long long HW = (long long)H * W;
  GRID_STRIDE(idx, total_vec) {
    const int c0 = (int)(idx % cv) * VE;
    const long long pix = idx / cv;              // n * HW + y * W + x
    const long long n = pix / HW;
    const long long p = pix - n * HW;            // y * W + x
    float v[VE];
    Vec16<T>::load(t + idx * VE, v);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const int c = c0 + j;
      float o = 0.f;
      if (c < C) {
        const float x = v[j];
        if (!train) {
          o = x > 0.f ? 1.f : (x < 0.f ? -1.f : x);            // NaN and +-0 pass through, as torch.sign
        } else {
          const long long e = (long long)c * HW + p;
          float u;
          if (u_override != nullptr) {
            u = u_override[n * (long long)C * HW + e];
          } else {
            const uint32_t w = philox4x32_10_word((uint32_t)(e >> 2), (uint32_t)(n_global0 + n), d0, d1, k0, k1,
                                                  (int)(e & 3));
            u = (float)(w >> 8) * 0x1p-24f;
          }
          const float h = (1.0f - x) / 2.0f;
          o = h <= u ? 1.f : -1.f;
        }
      }
      v[j] = o;
    }
    Vec16<T>::store(b + idx * VE, v);
  }
}

// Per-image counts of b == +1 and b == 0 over the C*H*W logical elements.  Stage 1: grid (blocks, N); every wave counts with
// __ballot + popcount (the count is wave-uniform, lane 0 keeps it), the block's four waves meet in LDS and the block writes
// its partial [N][blocks][2].  Stage 2 adds the partials of each image in block order.  Integers: exact and deterministic.
template <typename T>
__global__ void code_stats_kernel(const T* __restrict__ b, int32_t* __restrict__ partial, int C, int Cs,
                                  long long vec_per_image) {
  constexpr int VE = Vec16<T>::N;
  const int cv = Cs / VE;
  const int n = blockIdx.y;
  const T* base = b + (long long)n * vec_per_image * VE;
  int32_t pos = 0, zero = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < vec_per_image;
       i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cv) * VE;
    float v[VE];
    Vec16<T>::load(base + i * VE, v);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const bool live = c0 + j < C;
      // lane 0 holds the smallest index of the wave, so it is active in every iteration any lane of its wave runs
      pos += __popcll(__ballot(live && v[j] > 0.f));
      zero += __popcll(__ballot(live && v[j] == 0.f));
    }
  }
  __shared__ int32_t red[2][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = pos;
    red[1][wave] = zero;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t* out = partial + ((long long)n * gridDim.x + blockIdx.x) * 2;
    out[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    out[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ void code_stats_final_kernel(const int32_t* __restrict__ partial, int32_t* __restrict__ counts, int N,
                                        int blocks) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int32_t pos = 0, zero = 0;
  for (int k = 0; k < blocks; ++k) {
    pos += partial[((long long)n * blocks + k) * 2];
    zero += partial[((long long)n * blocks + k) * 2 + 1];
  }
  counts[2 * n] = pos;
  counts[2 * n + 1] = zero;
}

// (b + 1) / 2 as fp32 [N][C*H*W] in NCHW flatten order (pix2pixHD_model.py:562: code.view(N, -1)); one thread per output
template <typename T>
__global__ void code_export_kernel(const T* __restrict__ b, float* __restrict__ out, int C, int Cs, long long HW,
                                   long long total) {
  GRID_STRIDE(idx, total) {
    const long long p = idx % HW;
    const long long t = idx / HW;
    const int c = (int)(t % C);
    const long long n = t / C;
    out[idx] = (ElemOps<T>::ld(b + (n * HW + p) * Cs + c) + 1.f) * 0.5f;
  }
}

// the same bits packed MSB first (np.packbits order): byte k of image n holds elements 8k .. 8k+7, bit 7-j = (b > 0)
template <typename T>
__global__ void code_pack_kernel(const T* __restrict__ b, uint8_t* __restrict__ out, int C, int Cs, long long HW,
                                 long long nbytes, long long total) {
  const long long bits = (long long)C * HW;
  GRID_STRIDE(idx, total) {
    const long long n = idx / nbytes;
    const long long k = idx - n * nbytes;
    uint32_t byte = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long e = 8 * k + j;
      if (e < bits) {
        const int c = (int)(e / HW);
        const long long p = e - (long long)c * HW;
        if (ElemOps<T>::ld(b + (n * HW + p) * Cs + c) > 0.f) byte |= 0x80u >> j;
      }
    }
    out[idx] = (uint8_t)byte;
  }
}

// The inverse of the two export kernels: b = +1 / -1 from the stored code, never 0; padding lanes 0.  One thread per 16-byte
// vector of b (the mapping of binarize_fwd_kernel: a wave's stores are contiguous); its VE channels sit H*W elements apart in
// the code, so channel c of pixel p is element e = c*HW + p: bit 7 - (e & 7) of byte e >> 3 (a channel does not start on a byte
// when HW % 8 != 0), or in[e] > 0.5f of the fp32 form (NaN: -1).  Neighbouring pixels read neighbouring bits of the same
// bytes.  row = bytes (packed) or elements (fp32) per image; e < C*HW, so no read leaves the image's row.
template <typename T, bool PACKED>
__global__ void code_import_kernel(const void* __restrict__ in, T* __restrict__ b, int C, int Cs, long long HW, long long row,
                                   long long total_vec) {
  constexpr int VE = Vec16<T>::N;
  const int cv = Cs / VE;
  GRID_STRIDE(idx, total_vec) {
    const int c0 = (int)(idx % cv) * VE;
    const long long pix = idx / cv;              // n * HW + y * W + x
    const long long n = pix / HW;
    const long long p = pix - n * HW;
    float v[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const int c = c0 + j;
      float o = 0.f;
      if (c < C) {
        const long long e = (long long)c * HW + p;
        bool one;
        if constexpr (PACKED)
          one = (static_cast<const uint8_t*>(in)[n * row + (e >> 3)] >> (7 - (int)(e & 7))) & 1;
        else
          one = static_cast<const float*>(in)[n * row + e] > 0.5f;
        o = one ? 1.f : -1.f;
      }
      v[j] = o;
    }
    Vec16<T>::store(b + idx * VE, v);
  }
}

static int stats_blocks(int dtype, int H, int W, int C) {
  const long long vpi = (long long)H * W * (cpad(C) / vec_elems(dtype));
  long long blocks = (vpi + 1023) / 1024;           // >= 4 vectors per thread
  if (blocks < 1) blocks = 1;
  if (blocks > 256) blocks = 256;
  return (int)blocks;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

int jpdse_binarize_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* t, void* b, int32_t train,
                       uint64_t seed, uint64_t draw, int64_t n_global0, const float* u, void* stream) {
  JPDSE_REQUIRE(!bad_dtype(dtype) && t && b && N > 0 && H > 0 && W > 0 && C > 0 && n_global0 >= 0,
                "binarize_fwd: bad argument");
  JPDSE_REQUIRE(n_global0 + N <= 0xffffffffLL, "binarize_fwd: image index beyond 32 bits");
  const int Cs = cpad(C);
  const long long tv = (long long)N * H * W * (Cs / vec_elems(dtype));
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), d0 = (uint32_t)draw, d1 = (uint32_t)(draw >> 32);
  return by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return ew_launch("binarize_fwd", binarize_fwd_kernel<T>, tv, stream, cptr<T>(t), mptr<T>(b), H, W, C, Cs, train ? 1 : 0, k0,
                     k1, d0, d1, n_global0, u, tv);
  });
}

size_t jpdse_code_stats_workspace_size(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C) {
  if (bad_dtype(dtype) || N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (size_t)N * stats_blocks(dtype, H, W, C) * 2 * sizeof(int32_t);
}

int jpdse_code_stats(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* b, int32_t* counts, void* ws,
                     size_t ws_bytes, void* stream) {
  JPDSE_REQUIRE(!bad_dtype(dtype) && b && counts && N > 0 && H > 0 && W > 0 && C > 0, "code_stats: bad argument");
  JPDSE_REQUIRE((long long)C * H * W < (1LL << 31), "code_stats: more than 2^31 bits per image");
  if (ws == nullptr || ws_bytes < jpdse_code_stats_workspace_size(dtype, N, H, W, C))
    return set_error(JPDSE_EWORKSPACE, "code_stats: workspace too small");
  const int Cs = cpad(C);
  const long long vpi = (long long)H * W * (Cs / vec_elems(dtype));
  const int blocks = stats_blocks(dtype, H, W, C);
  int32_t* partial = mptr<int32_t>(ws);
  if (int rc = by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return launch256("code_stats", code_stats_kernel<T>, dim3(blocks, N), stream, cptr<T>(b), partial, C, Cs, vpi);
      }))
    return rc;
  hipLaunchKernelGGL(code_stats_final_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), partial, counts, N,
                     blocks);
  return check_launch("code_stats_final");
}

int jpdse_code_export(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* b, int32_t packed, void* out,
                      void* stream) {
  JPDSE_REQUIRE(!bad_dtype(dtype) && b && out && N > 0 && H > 0 && W > 0 && C > 0, "code_export: bad argument");
  const int Cs = cpad(C);
  const long long HW = (long long)H * W, bits = (long long)C * HW;
  const long long nbytes = (bits + 7) / 8, total = (long long)N * (packed ? nbytes : bits);
  return by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (packed)
      return ew_launch("code_export(packed)", code_pack_kernel<T>, total, stream, cptr<T>(b), mptr<uint8_t>(out), C, Cs, HW,
                       nbytes, total);
    return ew_launch("code_export", code_export_kernel<T>, total, stream, cptr<T>(b), mptr<float>(out), C, Cs, HW, total);
  });
}

int jpdse_code_import(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* in, int32_t packed, void* b,
                      void* stream) {
  if (int rc = code_import_check(dtype, N, H, W, C, in, b)) return rc;
  const int Cs = cpad(C);
  const long long HW = (long long)H * W, bits = (long long)C * HW;
  const long long row = packed ? (bits + 7) / 8 : bits;
  const long long tv = (long long)N * HW * (Cs / vec_elems(dtype));
  return by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (packed)
      return ew_launch("code_import(packed)", code_import_kernel<T, true>, tv, stream, in, mptr<T>(b), C, Cs, HW, row, tv);
    return ew_launch("code_import", code_import_kernel<T, false>, tv, stream, in, mptr<T>(b), C, Cs, HW, row, tv);
  });
}

}  // extern "C"
