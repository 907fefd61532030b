// LDS primitives of the hand-scheduled kernels: addresses, inline-asm loads and stores, LDS-DMA, counted vmcnt waits.
//
// Why inline asm.  hipcc tracks LDS-DMA (global_load_lds) with vmcnt, and it cannot prove that an ordinary LDS access does not
// overlap a DMA in flight.  So it puts `s_waitcnt vmcnt(0)` in front of every ordinary LDS STORE issued while a DMA is
// outstanding, which drains a row prefetch at the first store behind it; and it waits lgkmcnt(0) between an ordinary LDS
// READ and its first use, which exposes the whole LDS round trip where one wave per SIMD has nothing to hide it behind.  The asm
// forms are invisible to that wait insertion: the CALLER orders them -- a counted lgkmcnt before a read's value is used, and
// lgkmcnt(0) plus a barrier (or the in-order execution of one wave's LDS instructions) between a store and its readers.
// Data that reaches an asm store straight from MFMA accumulators must pass through a VALU instruction first, so that
// the compiler's own MFMA -> VALU wait states apply (head_fwd.h).
#pragma once
#include "common.h"

namespace jpdse {

__device__ __forceinline__ uint32_t lds_addr32(const void* p) {       // 32-bit LDS address of a generic pointer into LDS
  return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)p);
}

// LDS-DMA: 64 lanes x 16 bytes from per-lane global addresses to 1 KiB of LDS at a wave-uniform base (tracked by vmcnt)
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ void lds_store128(uint32_t addr, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_store32(uint32_t addr, float v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_store32u(uint32_t addr, uint32_t v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}

// ds_read_b128 whose wait is the caller's: s_waitcnt lgkmcnt(n) with the value as a "+v" operand before its first use
__device__ __forceinline__ s16x8 lds_read128_asm(uint32_t addr) {
  s16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_waitcnt vmcnt(BASE + k * STEP), k = 0 .. MAXK chosen at run time (the immediate must be a constant)
template <int BASE, int STEP, int MAXK = 8> __device__ __forceinline__ void wait_vmcnt_sel(int k) {
  static_assert(MAXK <= 8 && BASE + MAXK * STEP <= 63, "vmcnt is a 6-bit counter");
  constexpr auto at = [](int j) constexpr { return BASE + (j < MAXK ? j : MAXK) * STEP; };
  switch (k) {
    case 0: wait_vmcnt<at(0)>(); break;
    case 1: wait_vmcnt<at(1)>(); break;
    case 2: wait_vmcnt<at(2)>(); break;
    case 3: wait_vmcnt<at(3)>(); break;
    case 4: wait_vmcnt<at(4)>(); break;
    case 5: wait_vmcnt<at(5)>(); break;
    case 6: wait_vmcnt<at(6)>(); break;
    case 7: wait_vmcnt<at(7)>(); break;
    default: wait_vmcnt<at(8)>(); break;
  }
}

}  // namespace jpdse
