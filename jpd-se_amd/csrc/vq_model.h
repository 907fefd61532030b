// The modelling the two index coders of the vector quantizer (vq_coder.hip: DESIGN.md 4.14; vq_plane.hip: 4.19) share with
// their cost maps (vq_cost.hip: 4.20).  The order-0 index coder's model is stated ONCE, as a walk over a stream that hands its
// decisions to a sink (range_coder.h: model walks and their sinks): the encoder runs it with RcEncoder, the cost map runs the
// same walk with CostPricer, so the map prices what its coder codes by construction.  The tables' LDS columns, the slots of
// the encoders and the byte side stay with the kernels.
//
// The plane coder shares the geometry, the table init and plane_clean only: its encoder, its cost kernel and its decoder keep
// their own loops.  On the shared walk (both sink forms) and the shared entry functions the cost kernel was 1.3-1.5 % slower
// than the parent (0.527 -> 0.534 ms, parent's spread 0.001), the decoder 1-3 % (4.113 -> 4.256 ms at strip_rows 16, spread
// 0.039) and the encoder +1 % at strip_rows 16 though 5 % faster at 8: profiles/coder_walks_ab.txt.
#pragma once
#include "range_coder.h"

namespace jpdse {

// index coder: the symbols of stream s, M = q S + r: the first r streams hold q + 1
__device__ __forceinline__ int vq_stream_count(int s, int q, int r) { return q + (s < r ? 1 : 0); }

// The walk of stream s of the index coder: its symbols index[s], index[s + S], ..., each nb decisions, most significant bit
// first, through the bit tree of the lane's column prob (node m at entry m).  An index outside [0, L) is walked as 0 and sets
// bad to 2, the status bit of a bad index.  The sink travels by value: that form keeps the encoders on their measured code.
template <typename Sink>
__device__ __forceinline__ Sink vq_index_walk(const int32_t* __restrict__ index, uint16_t* prob, int s, int M, int L, int S,
                                               int nb, Sink sink, int& bad) {
  const int q = M / S, r = M - q * S, cnt = vq_stream_count(s, q, r);
  // every stream has at least one symbol (S <= M); the next index is loaded before the current one is visited
  int32_t next = index[s];
  for (int i = 0; i < cnt; ++i) {
    int32_t v = next;
    if (i + 1 < cnt) next = index[(long long)(i + 1) * S + s];
    if ((uint32_t)v >= (uint32_t)L) {
      v = 0;
      bad = 2;
    }
    uint32_t m = 1;
    for (int k = nb - 1; k >= 0; --k) {
      const uint32_t bit = ((uint32_t)v >> k) & 1u;
      sink.put(prob[m * 64], bit);
      m = m << 1 | bit;
    }
    sink.symbol_done((long long)i * S + s);
  }
  return sink;
}

// plane coder
constexpr int kPlaneUp = 8, kPlaneUpOnly = 10, kPlaneTree = 10;   // entries: 0 .. 7 left flag, 8 .. 9 / 10 upper flag, 10 + m

// the geometry of stream s: its group, its strip's first row and its rows.  Only the last strip is short
struct PlaneStream {
  int g, y0, rows;
};
__device__ __forceinline__ PlaneStream plane_stream(int s, int h, int G, int strip_rows) {
  const int k = s / G, y0 = k * strip_rows;
  return PlaneStream{s - k * G, y0, min(strip_rows, h - y0)};
}

__device__ __forceinline__ void plane_table_init(uint16_t* prob, int nb) {
  for (int e = 0; e < kPlaneTree + (1 << nb); ++e) prob[e * 64] = (uint16_t)kProbInit;
}

// an index as the coder sees it: a value outside [0, L) is 0, for the symbol itself and as a neighbour alike
__device__ __forceinline__ int plane_clean(int32_t v, int L, int& bad) {
  if ((uint32_t)v >= (uint32_t)L) {
    bad = 2;
    return 0;
  }
  return v;
}

// More than 64 KiB of dynamic LDS (the plane table at nb = 9: 66,816 bytes; either cost walk at nb = 9, its table plus the
// 8,448 bytes of the cost table) needs the kernel's opt-in; two such blocks still fit a CU's 160 KiB, the occupancy
// vq_coder.hip has at its 64 KiB.  Host only, idempotent.
template <typename K>
static int vq_plane_lds_optin(const char* what, K kernel, size_t lds) {
  if (lds <= 65536) return JPDSE_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return set_error(JPDSE_ELAUNCH, "%s: %zu bytes of LDS: %s", what, lds, hipGetErrorString(e));
  return JPDSE_OK;
}

}  // namespace jpdse
