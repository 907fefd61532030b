// Shared host/device helpers for libjpdse_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/jpdse.h"

namespace jpdse {

// ---- error plumbing ---------------------------------------------------------------------
int set_error(int code, const char* fmt, ...);
int check_launch(const char* what);

#define JPDSE_REQUIRE(cond, ...)                              \
  do {                                                        \
    if (!(cond)) return ::jpdse::set_error(JPDSE_EINVAL, __VA_ARGS__); \
  } while (0)

// argument checks of jpdse_code_import (api.cpp): JPDSE_EINVAL + message before any launch, JPDSE_OK otherwise
int code_import_check(int dtype, int N, int H, int W, int C, const void* in, const void* b);

// argument checks of the jpdse_vq_* calls (api.cpp; kernels: vq.hip): JPDSE_EINVAL + message before any launch.  The shape
// check is the limits 1 <= D <= 32, 2 <= L <= 512, M >= 1, M * L < 2^31; vq_workspace_bytes (vq.hip) is what
// jpdse_vq_workspace_size returns for a shape inside them.
int vq_shape_check(const char* who, int M, int D, int L);
size_t vq_workspace_bytes(int M, int D, int L);
int vq_soft_fwd_check(const jpdse_vq_soft_fwd_args* a);
int vq_hard_fwd_check(const jpdse_vq_hard_fwd_args* a);
int vq_soft_bwd_check(const jpdse_vq_soft_bwd_args* a);
int vq_decode_check(const jpdse_vq_decode_args* a);
int vq_decode_bwd_check(const jpdse_vq_decode_bwd_args* a);
int vq_argmax_check(const jpdse_vq_argmax_args* a);
int vq_pmf_check(const jpdse_vq_pmf_args* a);
int vq_pmf_bwd_check(const jpdse_vq_pmf_bwd_args* a);
// the code-book fit (kernels: vq_fit.hip): vq_lloyd_workspace_bytes (vq_fit.hip) is what
// jpdse_vq_lloyd_workspace_size returns for a shape inside the limits
size_t vq_lloyd_workspace_bytes(int M, int D, int L);
int vq_lloyd_accum_check(const jpdse_vq_lloyd_accum_args* a);
int vq_lloyd_update_check(const jpdse_vq_lloyd_update_args* a);
// shared with the bottleneck and the rate term (kernels: vq_bottleneck.hip): a workspace of at least `need` bytes; dtype, shape
// and sigma; the groups of the per-group histograms (G >= 1 divides M, G * L <= 65536)
int vq_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need);
int vqb_common_check(const char* who, int dtype, int M, int D, int L, float sigma);
int vqr_group_check(const char* who, int M, int L, int G);
// the residual quantizer (kernels: vq_residual.hip): dtype, the shape limits above, 1 <= S <= 8 books and
// lowest <= n <= S stages in use (lowest 0 or 1); vq_res_workspace_bytes (vq_residual.hip) is what jpdse_vq_res_workspace_size
// returns inside them.  vq_res_grouped_check: the same with lowest 1, vqr_group_check, and n * G * L <= kVqResCells (what
// ops.vq_ec_lengths takes as [n * G][L]): the calls with per-group tables (vq_res_ec.hip, vq_res_rate.hip, the grouped backward)
constexpr int kVqResCells = 65536;
int vq_res_check(const char* who, int dtype, int M, int D, int L, int S, int n, int lowest = 0);
int vq_res_grouped_check(const char* who, int dtype, int M, int D, int L, int S, int n, int G);
size_t vq_res_workspace_bytes(int M, int D, int L, int n);

// the same for the jpdse_vq_index_* calls (api.cpp; kernels: vq_coder.hip).  vq_index_bits: the decisions per
// symbol; the two sizes are 0 outside the limits 2 <= L <= 512, 1 <= S <= min(M, 65535), M * nb and the capacity below 2^31.
int vq_index_bits(int L);
long long vq_index_capacity_bytes(int M, int L, int S);
size_t vq_index_workspace_bytes(int M, int L, int S);
int vq_index_encode_check(const jpdse_vq_index_encode_args* a);
int vq_index_decode_check(const jpdse_vq_index_decode_args* a);

// and for the jpdse_vq_plane_* calls (api.cpp; kernels: vq_plane.hip).  vq_plane_streams: S = ceil(h /
// strip_rows) * G of a checked shape; the two sizes are 0 outside the limits 2 <= L <= 512, h, w, G, strip_rows >= 1,
// S <= 65535, h * w * G and the capacity below 2^31.
int vq_plane_streams(int h, int G, int strip_rows);
long long vq_plane_capacity_bytes(int h, int w, int G, int L, int strip_rows);
size_t vq_plane_workspace_bytes(int h, int w, int G, int L, int strip_rows);
int vq_plane_encode_check(const jpdse_vq_plane_encode_args* a);
int vq_plane_decode_check(const jpdse_vq_plane_decode_args* a);

// the cost table of jpdse_code_cost_table (api.cpp): 2049 entries, built once on the host in fp64
const uint32_t* code_cost_table_host();
// the label path of the code-length maps (code_cost.hip, vq_cost.hip; kernels: cost_class.h): its limits and its checks.  C: the
// symbols per cell.  *shift = log2(s) for H = s h, W = s w, s a power of two
constexpr int kCostClassesMax = 256;             // what jpdse_eval_metrics_sem takes
constexpr long long kCostMaxUnits = 1LL << 40;   // symbols (and image pixels x C): every 64-bit sum stays below 2^60
int cost_label_check(const char* who, const void* class_units, const void* class_pixels, int H, int W, int h, int w, int C,
                     int n_classes, int* shift);

// the jpdse_vq_*_cost calls (api.cpp; kernels: vq_cost.hip): the limits of the matching encode call, G >= 1
// dividing M, and the label path above.  The size is 0 outside them; *shift as above, 0 without a label
size_t vq_cost_workspace_bytes(long long M);
int vq_index_cost_check(const jpdse_vq_index_cost_args* a, int* shift);
int vq_plane_cost_check(const jpdse_vq_plane_cost_args* a, int* shift);

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// opt-in timer of the HBM-bound calls (api.cpp; jpdse_prof_hbm_select / _collect): begin returns a slot or -1 (off / full)
int hbm_prof_begin(hipStream_t s);
void hbm_prof_end(int slot, int cls, double algorithmic_bytes, hipStream_t s);   // cls: JPDSE_HBM_INORM_FWD / _BWD / _ADAM
static inline int cpad(int c) { return (c + 7) & ~7; }
static inline size_t esize(int dtype) { return dtype == JPDSE_BF16 ? 2 : 4; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int bad_dtype(int dtype) { return !(dtype == JPDSE_F32 || dtype == JPDSE_BF16); }
static inline int vec_elems(int dtype) { return 16 / (int)esize(dtype); }   // elements per 16-byte vector
template <typename T> static const T* cptr(const void* p) { return reinterpret_cast<const T*>(p); }
template <typename T> static T* mptr(void* p) { return reinterpret_cast<T*>(p); }

// Kernel-selection switches: compile-time constants in the shipped library, run-time variables in the developer build
// (libjpdse_hip_dev.so, -DJPDSE_DEV; set through include/jpdse_dev.h).
#ifdef JPDSE_DEV
#define JPDSE_SWITCH(type, name, value) static type name = value
extern int g_norm_fused;     // norm.hip: InstanceNorm form, 1 = two register-held kernels (default), 0 = three kernels (mode 27)
#else
#define JPDSE_SWITCH(type, name, value) static constexpr type name = value
#endif

// ---- device scalar types ------------------------------------------------------------------
typedef uint16_t bf16_t;  // raw bf16 bits

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

__device__ __forceinline__ float bf2f(bf16_t b) { return __uint_as_float(((uint32_t)b) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 h = (__bf16)f;  // v_cvt_pk_bf16_f32: round-to-nearest-even, NaN preserving
  return __builtin_bit_cast(bf16_t, h);
}

template <typename T> struct ElemOps;
template <> struct ElemOps<float> {
  static constexpr int kDtype = JPDSE_F32;
  static constexpr int kVec = 4;  // elements per 16-byte vector
  __device__ static __forceinline__ float ld(const float* p) { return *p; }
  __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct ElemOps<bf16_t> {
  static constexpr int kDtype = JPDSE_BF16;
  static constexpr int kVec = 8;
  __device__ static __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
  __device__ static __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
};

// 16-byte vector of T unpacked to floats and back
template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  __device__ static __forceinline__ void unpack(u32x4 t, float (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(t[i]);
  }
  __device__ static __forceinline__ u32x4 pack(const float (&v)[4]) {
    u32x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = __float_as_uint(v[i]);
    return t;
  }
  __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  __device__ static __forceinline__ void store(float* p, const float (&v)[4]) {
    f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  }
  // streaming forms (nontemporal hint): the last use of a tensor far larger than the caches
  __device__ static __forceinline__ void load_nt(const float* p, float (&v)[4]) {
    f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  __device__ static __forceinline__ void store_nt(float* p, const float (&v)[4]) {
    f32x4 t = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
  }
};
template <> struct Vec16<bf16_t> {
  static constexpr int N = 8;
  __device__ static __forceinline__ void unpack(u32x4 t, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(t[i] << 16);
      v[2 * i + 1] = __uint_as_float(t[i] & 0xffff0000u);
    }
  }
  __device__ static __forceinline__ u32x4 pack(const float (&v)[8]) {
    u32x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      t[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
    return t;
  }
  __device__ static __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    u32x4 t = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(t[i] << 16);
      v[2 * i + 1] = __uint_as_float(t[i] & 0xffff0000u);
    }
  }
  __device__ static __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
    u32x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      t[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
    *reinterpret_cast<u32x4*>(p) = t;
  }
  __device__ static __forceinline__ void load_nt(const bf16_t* p, float (&v)[8]) {
    unpack(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)), v);
  }
  __device__ static __forceinline__ void store_nt(bf16_t* p, const float (&v)[8]) {
    __builtin_nontemporal_store(pack(v), reinterpret_cast<u32x4*>(p));
  }
};

// last read of a large tensor in a streaming kernel (nontemporal hint; -DJPDSE_NO_NT builds the A/B variant without it)
#ifndef JPDSE_NO_NT
#define JPDSE_LOAD_LAST(T, ptr, v) Vec16<T>::load_nt(ptr, v)
#else
#define JPDSE_LOAD_LAST(T, ptr, v) Vec16<T>::load(ptr, v)
#endif

// ---- InstanceNorm moments written by conv epilogues (conv_rows.h, dgrad2_rows.h, thin_fwd.h -> norm.hip) ----------------
// Every block writes, per (image, channel), ONE slot = (mean, M2) of the values it produced -- of the bf16-ROUNDED values,
// the ones that are stored and that the norm's backward re-reads -- with M2 = sum (v - mean)^2.  Each lane sums about its own
// pilot (its first value; no cross-lane operation inside the hand-scheduled loops), lanes that share a channel are merged
// pairwise with Chan's formula after the loop, so neither the sums nor the merge of the slots
// (finalize_slots_kernel: Chan's parallel-variance formula, all slots cover the same number of pixels) ever forms
// E[v^2] - mean^2 of un-shifted values: a channel with |mean| >> std keeps its variance.
__device__ __forceinline__ float bf16_round(float v) { return bf2f(f2bf(v)); }
// Chan's merge of two (mean, M2) pairs that cover `n_each` values each: (mean, m2) <- merged over 2 n_each values
__device__ __forceinline__ void chan_merge_equal(float& mean, float& m2, float mean_o, float m2_o, float n_each) {
  const float d = mean_o - mean;
  m2 = m2 + m2_o + d * d * (0.5f * n_each);
  mean = mean + 0.5f * d;
}
// (sum, sum of squares) about `pilot` over `count` values -> (mean, M2)
__device__ __forceinline__ void shifted_to_mean_m2(float s1, float s2, float pilot, float count, float& mean, float& m2) {
  const float d = s1 / count;
  mean = pilot + d;
  m2 = fmaxf(s2 - s1 * d, 0.f);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// uint8 quantiser of the evaluation paths (elementwise.hip jpdse_quant_loss, metrics.hip jpdse_eval_metrics):
// q(x) = uint8(clip((double(x) * std[c] + mean[c]) * 255.0, 0, 255)), the IEEE double operations numpy performs, unfused
struct QuantParams { double mean[8]; double std[8]; };
__device__ __forceinline__ int quant_u8(float x, double sd, double mu) {
  double v = __dmul_rn(__dadd_rn(__dmul_rn((double)x, sd), mu), 255.0);
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (int)v;           // truncation, as ndarray.astype(np.uint8) on a value in [0, 255]
}

// grid-stride launch geometry for HBM-bound kernels: <= 256 CUs x 8 blocks
static inline int ew_blocks(int64_t work_items, int threads = 256) {
  int64_t b = (work_items + threads - 1) / threads;
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  return (int)b;
}

// ---- host-side launch helpers of the HBM-bound sources (norm, elementwise, binarize, metrics) -------------------------------
// The one bf16 / fp32 dispatch: f is a generic lambda that receives a value of the element type,
//   by_dtype(dtype, [&](auto tag) { using T = decltype(tag); return launch256("x", x_kernel<T>, grid, stream, ...); })
template <typename F> static inline auto by_dtype(int dtype, F&& f) { return dtype == JPDSE_BF16 ? f(bf16_t{}) : f(float{}); }

// kernel<<<grid, 256, 0, stream>>>(args...) + check_launch(what); args convert to the kernel's parameter types
template <typename... P, typename... A>
static inline int launch256(const char* what, void (*kernel)(P...), dim3 grid, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), static_cast<P>(args)...);
  return check_launch(what);
}
// the same over ew_blocks(work_items) blocks: the grid-stride kernels
template <typename... P, typename... A>
static inline int ew_launch(const char* what, void (*kernel)(P...), long long work_items, void* stream, A... args) {
  return launch256(what, kernel, dim3(ew_blocks(work_items)), stream, args...);
}

}  // namespace jpdse
