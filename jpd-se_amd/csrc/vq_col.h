// The LDS column of a lane's private probability table, shared by the two index coders of the vector quantizer (vq_coder.hip:
// DESIGN.md 4.14; vq_plane.hip: 4.19).  Entry m of lane l is the halfword m * 64 + vq_col(l): a row of 64 halfwords is 128
// bytes = the 32 banks of the 16- and 32-bit LDS instructions, so the bank of an access depends on the lane alone, whatever
// entry each lane has reached, and the 32 lanes of an LDS lane group (0-31, 32-63) sit on 32 different banks.
#pragma once
#include "common.h"

namespace jpdse {

// the halfword of lane l inside a row of 64: lanes l and l + 32 share a dword and belong to different LDS lane groups
__device__ __forceinline__ int vq_col(int lane) { return ((lane & 31) << 1) | (lane >> 5); }

}  // namespace jpdse
