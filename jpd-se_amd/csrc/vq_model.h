// The modelling the two index coders of the vector quantizer (vq_coder.hip: DESIGN.md 4.14; vq_plane.hip: 4.19) share with
// their cost walks (vq_cost.hip: 4.20): which symbols a stream holds, the entries of a plane stream's table, and what an index
// outside [0, L) counts as -- one statement each, so a walk prices what its coder codes.  The slots of the encoders and the
// byte side stay with the coders.
#pragma once
#include "range_coder.h"

namespace jpdse {

// index coder: the symbols of stream s, M = q S + r: the first r streams hold q + 1
__device__ __forceinline__ int vq_stream_count(int s, int q, int r) { return q + (s < r ? 1 : 0); }

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
