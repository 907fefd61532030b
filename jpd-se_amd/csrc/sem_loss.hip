// Semantics-weighted training distortion (--class_distortion_weights / --edge_distortion_weight; no reference counterpart).
// Entry point: include/jpdse.h, "semantics-weighted distortion"; definition: DESIGN.md 4.11.
//   w(p)   = cw[label(p)] * (ew if edge(p) else 1)          label outside [0, n_table): 1; a fractional label is truncated
//   edge(p): the instance id of p differs from that of its left, right, upper or lower neighbour inside the same image
//   out[0] = sum_p sum_c w(p) f(d) / (N H W C),  d = fake - real,  f = |d| (l1) or d^2 (mse)
//   dfake  = scale * w(p) * f'(d) / (N H W C)               sign(0) = 0, as jpdse_l1_fwd_bwd
// Kernels:
//   sem_loss_partial_kernel  one thread per pixel, grid-stride over a fixed grid (jpdse_loss_partial_count(pixels) blocks):
//                            label, own id and the four neighbour ids from global memory (the neighbours were or will be
//                            another lane's own id: L2 hits, no LDS tile), the pixel's 16-byte vectors of fake and real, the
//                            gradient vectors written with plain vector stores, one fp32 partial per block
//   sem_loss_final_kernel    ONE block: the partials in index order, summed in fp64, times 1 / count -> the slot
// The class table travels by value in the kernel arguments (1 KB) and is staged in LDS once per block.  No atomics: every
// output element has one writer and every sum a fixed order, so two calls are bit-identical.
// HBM-bound: per pixel fake + real + dfake (16 B each in bf16 with 8 stored lanes) + 4 B label + 8 B id.
#include <math.h>

#include "common.h"

namespace jpdse {

constexpr int kSemTable = JPDSE_SEM_TABLE;
constexpr int kSemPartials = 1024;       // the cap of jpdse_loss_partial_count

struct SemTable { float w[kSemTable]; };

// fake, real, dfake: [npix][cs] of T; label: [npix] float; inst: [npix] int64 or nullptr (no edge term).
// gscale = scale / count (read when dfake != nullptr).  npix < 2^31: the pixel index and its split into (row, x) are 32-bit.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void sem_loss_partial_kernel(const T* __restrict__ fake, const T* __restrict__ real,
                                                              const float* __restrict__ label,
                                                              const long long* __restrict__ inst, const SemTable tab,
                                                              int n_table, float ew, unsigned H, unsigned W, unsigned npix,
                                                              int cs, float gscale, T* __restrict__ dfake,
                                                              float* __restrict__ partial) {
  constexpr int VE = Vec16<T>::N;
  __shared__ float cw[kSemTable];
  __shared__ float red[4];
  cw[threadIdx.x] = tab.w[threadIdx.x];
  __syncthreads();
  const int vpp = cs / VE;               // 16-byte vectors per pixel
  const float top = (float)n_table;
  float acc = 0.f;
  for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npix; p += gridDim.x * 256u) {
    const float lab = label[p];
    // truncation toward zero: (-1, 0) -> 0.  NaN fails both compares and gets weight 1.
    float w = (lab > -1.f && lab < top) ? cw[(int)lab] : 1.f;
    if (inst != nullptr) {
      const unsigned row = p / W, x = p - row * W, y = row % H;
      const long long id = inst[p];
      bool edge = false;
      if (x > 0) edge |= inst[p - 1] != id;
      if (x + 1 < W) edge |= inst[p + 1] != id;
      if (y > 0) edge |= inst[p - W] != id;
      if (y + 1 < H) edge |= inst[p + W] != id;
      if (edge) w *= ew;
    }
    const float gw = gscale * w;
    float s = 0.f;                       // the pixel's sum of f(d): padding lanes are zero in both operands
    const long long base = (long long)p * cs;
    for (int v = 0; v < vpp; ++v) {
      float a[VE], b[VE];
      Vec16<T>::load(fake + base + v * VE, a);
      JPDSE_LOAD_LAST(T, real + base + v * VE, b);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float d = a[e] - b[e];
        if (KIND == JPDSE_SEM_L1) {
          s += fabsf(d);
          a[e] = d > 0.f ? gw : (d < 0.f ? -gw : 0.f);
        } else {
          s += d * d;
          a[e] = 2.f * d * gw;
        }
      }
      if (dfake != nullptr) Vec16<T>::store(dfake + base + v * VE, a);
    }
    acc += w * s;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sem_loss_final_kernel(const float* __restrict__ partial, int n, double inv_count,
                                                            float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double)partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) red[threadIdx.x] += red[threadIdx.x + step];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] * inv_count);
}

static size_t sem_loss_ws_bytes() { return kSemPartials * sizeof(float); }

// everything that can be refused before any launch
static int sem_loss_check(const jpdse_sem_loss_args* a) {
  JPDSE_REQUIRE(a != nullptr, "sem_weighted_loss: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "sem_weighted_loss: bad dtype %d (fake and real are both fp32 or both bf16)", a->dtype);
  JPDSE_REQUIRE(a->kind == JPDSE_SEM_L1 || a->kind == JPDSE_SEM_MSE, "sem_weighted_loss: bad kind %d (0 = l1, 1 = mse)", a->kind);
  JPDSE_REQUIRE(a->fake && a->real && a->label && a->table && a->out, "sem_weighted_loss: null argument");
  JPDSE_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->C > 0, "sem_weighted_loss: non-positive extent (N %d, H %d, W %d, C %d)",
                a->N, a->H, a->W, a->C);
  JPDSE_REQUIRE((long long)a->N * a->H * a->W <= 0x7fffffffLL, "sem_weighted_loss: N * H * W = %lld pixels exceed 2^31 - 1",
                (long long)a->N * a->H * a->W);
  JPDSE_REQUIRE(a->n_table > 0 && a->n_table <= kSemTable, "sem_weighted_loss: table of %d entries (1 .. %d)", a->n_table,
                kSemTable);
  for (int i = 0; i < a->n_table; ++i)
    JPDSE_REQUIRE(isfinite(a->table[i]) && a->table[i] >= 0.f, "sem_weighted_loss: class weight %d is %g (a finite value >= 0)", i,
                  (double)a->table[i]);
  JPDSE_REQUIRE(isfinite(a->edge_w) && a->edge_w >= 0.f, "sem_weighted_loss: edge weight is %g (a finite value >= 0)",
                (double)a->edge_w);
  JPDSE_REQUIRE(a->dfake == nullptr || a->scale == a->scale, "sem_weighted_loss: scale is NaN");
  JPDSE_REQUIRE(a->ws != nullptr && a->ws_bytes >= sem_loss_ws_bytes(),
                "sem_weighted_loss: workspace too small (%zu bytes, %zu needed)", a->ws ? a->ws_bytes : (size_t)0,
                sem_loss_ws_bytes());
  return JPDSE_OK;
}

template <int KIND>
static int sem_loss_run(const jpdse_sem_loss_args* a, const long long* inst, const SemTable& tab, int grid, unsigned npix,
                        float gscale) {
  return by_dtype(a->dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch256("sem_weighted_loss", sem_loss_partial_kernel<T, KIND>, dim3(grid), a->stream, cptr<T>(a->fake),
                     cptr<T>(a->real), a->label, inst, tab, a->n_table, a->edge_w, (unsigned)a->H, (unsigned)a->W, npix,
                     cpad(a->C), gscale, mptr<T>(a->dfake), mptr<float>(a->ws));
  });
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

int jpdse_sem_weighted_loss(const jpdse_sem_loss_args* a) {
  if (int rc = sem_loss_check(a)) return rc;
  const long long npix = (long long)a->N * a->H * a->W;
  const double count = (double)npix * a->C;
  SemTable tab;
  for (int i = 0; i < kSemTable; ++i) tab.w[i] = i < a->n_table ? a->table[i] : 1.f;
  // an edge weight of 1 leaves every weight as it is: the ids are not read
  const long long* inst = a->edge_w == 1.f ? nullptr : reinterpret_cast<const long long*>(a->inst);
  const int grid = jpdse_loss_partial_count(npix);
  const float gscale = a->dfake != nullptr ? a->scale / (float)(npix * a->C) : 0.f;
  if (int rc = a->kind == JPDSE_SEM_L1 ? sem_loss_run<JPDSE_SEM_L1>(a, inst, tab, grid, (unsigned)npix, gscale)
                                       : sem_loss_run<JPDSE_SEM_MSE>(a, inst, tab, grid, (unsigned)npix, gscale))
    return rc;
  return launch256("sem_weighted_loss(final)", sem_loss_final_kernel, dim3(1), a->stream, mptr<float>(a->ws), grid,
                   1.0 / count, a->out);
}

}  // extern "C"
