// What the row-streaming convolutions share (conv_rows.h, head_rows.h, thin_rows.h, thin_in_rows.h, dgrad2_rows.h,
// thin_dgrad2_rows.h): the filter lives in registers, a block of four waves walks down a strip of one image, and the input
// rows stream through LDS exactly once, by LDS-DMA into a ring of NR row slots, LA iterations ahead of their use.  Here are the
// two pieces of bookkeeping that every one of them depends on and that are easy to get wrong -- the counted vmcnt wait on
// the ring (wait_rows) and the counted lgkmcnt wait of the fragment pipeline (wait_unit) -- with the ring cursor and the
// bf16 pair pack of the epilogues.  Geometry, swizzle, row mapping, filter layout and epilogue stay with each kernel.
// (The DMA unit loop of `issue_row` and the four-line read-ahead loop around wait_unit stay in the kernels as well: behind
// a function boundary hipcc orders the same operations differently, and the kernels' code is held bit-identical.)
//
// One iteration i of a kernel's row loop, and what each step may rely on:
//
//   wait_rows<UNITS, B, STEP, MAXK>(wid, k)   (1) this wave's pieces of the rows that iteration i reads have landed
//   s_barrier                                 (2) every wave's pieces have; every wave is done with the reads of iteration i-1
//   issue_row(njr, nslot), ring_next          (3) rows of iteration i + LA -> the slots that iteration i-1 released
//   rd(t + DEPTH) / wait_unit(t) / MFMAs      (4) reads slots ring_slot(base, 0 .. rows in use - 1), written LA iterations ago
//   base = ring_slot / ring_next(base)        (5) the window moves on
//   epilogue                                      its global stores (and, fused, loads) are vmcnt traffic as well
//
// (1) What is in flight.  vmcnt counts a wave's own vector-memory instructions.  At the top of iteration i the youngest of them
// are, as (3) and the epilogues issued them: the rows of iterations i+1 .. i+LA-1 -- B rows, each U0 or U1 DMA
// instructions for this wave (RowUnits: the 1 KiB units of a row are dealt round-robin to the four waves, so the first EXTRA
// waves carry one more) -- and the epilogue stores of the last k iterations, STEP instructions each, k growing from 0 to MAXK
// over the first iterations.  The wait lets exactly that many stay outstanding.  It is counted, not vmcnt(0), because
// vmcnt(0) drains the look-ahead once per output row: what bounds these kernels is the number of bytes in flight per CU,
// and a drained ring pays the HBM latency again at every row.  A kernel whose store count per iteration is not a constant
// (a partly masked last strip) waits for the rows only, wait_rows<UNITS, B>(wid): its stores are older than the rows still
// allowed in flight, so the wait covers them too -- conservative, never wrong.  Every iteration must issue the same
// number of DMA instructions: a row outside the image is fetched from the zero page (which is also how zero padding is
// made), never skipped.
//
// (2) Which barrier protects which slot.  The barrier at the top of iteration i is both the "rows complete" and the "slot
// free" barrier: the DMA of (3) overwrites the slots whose last readers were the fragment reads of iteration i-1, and
// every wave finished those (the lgkmcnt(0) at the end of its pipeline) before it arrived here.  The ring therefore needs
// rows in use + rows in flight <= NR, which each geometry struct asserts or spells out.  The barrier is the raw builtin
// followed by a compiler-only memory clobber: __syncthreads() would add vmcnt(0).
//     Kernels whose epilogue goes through ONE tile per block (thin_rows, thin_in_rows, dgrad2_rows) have a second barrier
// B behind the MFMAs: the tile of row i-1 is copied out right behind barrier A of iteration i, and B keeps row i's
// accumulators from overwriting it before every thread has read.  Kernels with a tile per WAVE (conv_rows, head_rows,
// thin_dgrad2_rows) need none: the LDS executes one wave's instructions in order.
//
// (4) One wave per SIMD: nothing hides the LDS round trip, and hipcc's own schedule (read, lgkmcnt(0), MFMA) exposes it at
// every k-step.  So the fragment reads are inline asm (lds_read128_asm), issued DEPTH units ahead into a rotating
// fr[DEPTH + 1] buffer (a unit = the FR fragments that one step of MFMAs consumes).  LDS operations return in order and
// nothing else in the loop uses lgkmcnt (no scalar loads), so "unit t has arrived" is lgkmcnt(FR * units issued behind t).
// The waits carry the fragment registers as "+v" operands, which pins the MFMAs behind the wait that covers their operands.
//
// LDS stores near an in-flight LDS-DMA must be the inline-asm forms of lds_ops.h (hipcc puts vmcnt(0) in front of an ordinary
// one), followed by `s_waitcnt lgkmcnt(0)` before anything reads them back.  Ordinary LDS stores are fine only where no DMA
// has been issued yet (the zeroing of the fp32 row tiles of head_rows and thin_dgrad2_rows).
#pragma once
#include "common.h"
#include "lds_ops.h"

namespace jpdse {

// A row of UNITS 1 KiB DMA units: unit u belongs to wave u % 4, so a wave moves U0 units of every row and the first EXTRA
// waves one more.  col_off[k]: per lane, the source element offset inside a row of the wave's k-th unit (u = wid + 4 k), -1 =
// no source (the unit does not exist, padding, beyond the strip): the zero page is staged instead.
template <int UNITS> struct RowUnits {
  static constexpr int U0 = UNITS / 4, U1 = U0 + 1, EXTRA = UNITS % 4;
};

// s_waitcnt vmcnt: everything of this wave's has completed but its youngest ROWS rows of DMA ...
template <int UNITS, int ROWS> __device__ __forceinline__ void wait_rows(int wid) {
  typedef RowUnits<UNITS> RU;
  if (wid < RU::EXTRA) wait_vmcnt<ROWS * RU::U1>(); else wait_vmcnt<ROWS * RU::U0>();
}
// ... and k * STEP instructions behind them (epilogue stores), k = 0 .. MAXK at run time
template <int UNITS, int ROWS, int STEP, int MAXK> __device__ __forceinline__ void wait_rows(int wid, int k) {
  typedef RowUnits<UNITS> RU;
  if (wid < RU::EXTRA) wait_vmcnt_sel<ROWS * RU::U1, STEP, MAXK>(k); else wait_vmcnt_sel<ROWS * RU::U0, STEP, MAXK>(k);
}

// ring cursor: the slot behind `slot`, and the slot r < NR behind it
template <int NR> __device__ __forceinline__ int ring_next(int slot) { return slot + 1 == NR ? 0 : slot + 1; }
template <int NR> __device__ __forceinline__ int ring_slot(int slot, int r) {
  slot += r;
  return slot >= NR ? slot - NR : slot;
}

// s_waitcnt lgkmcnt(N) tied to the fragment registers it makes valid
template <int N> __device__ __forceinline__ void wait_lgkm(s16x8& a) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N));
}
template <int N> __device__ __forceinline__ void wait_lgkm(s16x8& a, s16x8& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
template <int N> __device__ __forceinline__ void wait_lgkm(s16x8& a, s16x8& b, s16x8& c, s16x8& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}

// The wait in front of the MFMAs of unit t, of T units that are read DEPTH units ahead, f...: the unit's fragment registers.
// t is a constant after unrolling.
template <int T, int DEPTH, class... F> __device__ __forceinline__ void wait_unit(int t, F&... f) {
  constexpr int FR = sizeof...(F);
  static_assert(DEPTH >= 1 && DEPTH < T && DEPTH <= 7 && DEPTH * FR <= 15, "lgkmcnt is a 4-bit counter");
  constexpr auto cnt = [](int b) constexpr { return (b <= DEPTH ? b : 0) * FR; };   // (never reached beyond DEPTH)
  const int behind = (T - 1 - t) < DEPTH ? (T - 1 - t) : DEPTH;        // units issued after unit t
  if (behind == 7) wait_lgkm<cnt(7)>(f...);
  else if (behind == 6) wait_lgkm<cnt(6)>(f...);
  else if (behind == 5) wait_lgkm<cnt(5)>(f...);
  else if (behind == 4) wait_lgkm<cnt(4)>(f...);
  else if (behind == 3) wait_lgkm<cnt(3)>(f...);
  else if (behind == 2) wait_lgkm<cnt(2)>(f...);
  else if (behind == 1) wait_lgkm<cnt(1)>(f...);
  else wait_lgkm<0>(f...);
}

// Accumulator rows e (v0) and e + 1 (v1) of this lane's column -> the dword (column, column + 1) of ONE of the rows: even
// lanes get row e (their v0 | the odd neighbour's v0), odd lanes row e + 1 (the even neighbour's v1 | their v1), and store
// it at the even lane's column.  The exchange is a DPP quad permutation [1,0,3,2]: __shfl_xor is a ds_bpermute round trip
// with nothing to hide it behind (one wave per SIMD).  odd = lane & 1.
__device__ __forceinline__ uint32_t pack_bf16_pair(float v0, float v1, int odd) {
  const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, odd ? v0 : v1), 0xB1, 0xF, 0xF, false));
  const float lo = odd ? recv : v0, hi = odd ? v1 : recv;
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}

}  // namespace jpdse
