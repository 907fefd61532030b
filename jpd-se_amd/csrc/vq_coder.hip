// Lossless coded stream of the S2HVQ indices (no reference counterpart: the reference never writes its code as bytes): an
// order-0 adaptive L-ary coder and its decoder.  Format: DESIGN.md 4.14.  Entry points: include/jpdse.h, "soft-to-hard vector
// quantizer: coded index stream"; argument checks and the closed forms of the sizes: api.cpp.
//
// The M indices are dealt to S streams by interleaving (stream s holds the symbols s, s + S, ...), so lane = stream: the 64
// lanes of a wave read (encoder) or write (decoder) 64 consecutive int32 words per step, and the loop over the steps is
// wave-uniform.  A symbol is nb = bit_length(L - 1) binary decisions, most significant bit first, through a bit tree of
// 2^nb adaptive probabilities per stream; every decision is range_coder.h's RcEncoder::encode / RcDecoder::decode, and the
// payload layout, stream_span and compact_stream are that header's too.  The encoder's loop over a stream is vq_model.h's
// vq_index_walk, which the cost map of vq_cost.hip runs too.  A lane's table is a column of 16-bit entries in
// LDS that no other lane touches (no barrier): entry m of lane l is the halfword m * 64 + vq_col(l), so the bank of an
// access depends on the lane alone, whatever node each lane's walk has reached, and the 32 lanes of an LDS lane group sit
// on 32 different banks.  One wave per block, 2^nb * 128 bytes of LDS: 64 KiB at L = 512, within the default limit.
#include "range_coder.h"
#include "vq_col.h"
#include "vq_model.h"

namespace jpdse {

// the slot (nb * count + 8 bytes) of stream s in the workspace; its count: vq_model.h
__device__ __forceinline__ long long vq_slot_offset(int s, int q, int r, int nb) {
  return (long long)s * (nb * (long long)q + 8) + (long long)nb * min(s, r);
}

// Phase 1 of the encoder: stream s into its slot; lens[s] = the bytes it needs (slot size + 1: it did not fit, unreachable by
// the bound of DESIGN.md 4.14), flags[s] = 2 when the stream held an index outside [0, L), which was coded as 0.
// grid ceil(S / 64), one wave per block, 2^nb * 128 bytes of dynamic LDS.
__global__ void __launch_bounds__(64) vq_index_encode_kernel(const int32_t* __restrict__ index, uint8_t* __restrict__ slots,
                                                             int32_t* __restrict__ lens, int32_t* __restrict__ flags, int M,
                                                             int L, int S, int nb) {
  extern __shared__ uint16_t vq_prob[];
  const int lane = threadIdx.x, s = blockIdx.x * 64 + lane;
  if (s >= S) return;                           // no cross-lane operation below
  uint16_t* prob = vq_prob + vq_col(lane);      // [2^nb][64]; entry 0 is unused
  for (int m = 1; m < (1 << nb); ++m) prob[m * 64] = (uint16_t)kProbInit;
  const int q = M / S, r = M - q * S, cnt = vq_stream_count(s, q, r);
  const int scap = nb * cnt + 8;
  RcEncoder rc;
  rc.init(slots + vq_slot_offset(s, q, r, nb), scap);
  int bad = 0;
  rc = vq_index_walk(index, prob, s, M, L, S, nb, rc, bad);
  lens[s] = rc.finish();
  flags[s] = bad;
}

// Phase 2: the S little-endian uint32 stream lengths, then the streams in order.  One wave per stream (compact_stream); the
// wave of the last stream also writes the payload's size and the status word (bit 0: a cut stream, bit 1: a bad index).
// grid ceil(S / 4), 256 threads.
__global__ void vq_index_compact_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens,
                                        const int32_t* __restrict__ flags, uint8_t* __restrict__ out, int32_t* __restrict__ size,
                                        int32_t* __restrict__ status, int M, int S, int nb) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;                           // wave-uniform
  const int q = M / S, r = M - q * S;
  // the host checked the room at `out` against 4 S + the sum of the slots
  const Compacted c = compact_stream(out, slots + vq_slot_offset(s, q, r, nb), lens, flags, S, s, lane,
                                     [=](int j) { return nb * vq_stream_count(j, q, r) + 8; });
  if (s == S - 1 && lane == 0) {
    *size = c.end;
    *status = c.status;
  }
}

// Decoder: lane s decodes exactly its count of symbols from its stream, whatever the bytes are, and writes them to
// index[s], index[s + S], ...  The length table is device data it does not trust: every stream is clipped to the `have`
// bytes of the payload (stream_span; 4 S <= have: checked by the host) and a byte past a stream's end reads as 0.  A value
// >= L (possible when L is no power of two) is written as L - 1 and sets bit 1 of *status with a plain store; the tree walk
// itself goes on with the decoded bits, whose node index stays below 2^nb.
// grid ceil(S / 64), one wave per block, 2^nb * 128 bytes of dynamic LDS.
__global__ void __launch_bounds__(64) vq_index_decode_kernel(const uint8_t* __restrict__ in, long long have,
                                                             int32_t* __restrict__ index, int32_t* __restrict__ status, int M,
                                                             int L, int S, int nb) {
  extern __shared__ uint16_t vq_prob[];
  const int lane = threadIdx.x, s0 = blockIdx.x * 64, s = s0 + lane;
  const StreamSpan span = stream_span(in, S, s0, lane, have);
  if (s >= S) return;
  uint16_t* prob = vq_prob + vq_col(lane);
  for (int m = 1; m < (1 << nb); ++m) prob[m * 64] = (uint16_t)kProbInit;
  const int q = M / S, r = M - q * S, cnt = vq_stream_count(s, q, r);
  RcDecoder rc;
  rc.init(in + span.start, (long long)(span.end - span.start));
  bool bad = false;
  for (int i = 0; i < cnt; ++i) {
    uint32_t m = 1;
    for (int k = 0; k < nb; ++k) {
      uint32_t p = prob[m * 64];
      const uint32_t bit = rc.decode(p);
      prob[m * 64] = (uint16_t)p;
      m = m << 1 | bit;
    }
    int v = (int)(m - (1u << nb));
    if (v >= L) {
      v = L - 1;
      bad = true;
    }
    index[(long long)i * S + s] = v;
  }
  if (bad) *status = 2;                         // every writer stores the same word
}

static inline size_t vq_index_lds_bytes(int nb) { return (size_t)(1 << nb) * 64 * sizeof(uint16_t); }

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_index_capacity(int32_t M, int32_t L, int32_t S) { return (size_t)vq_index_capacity_bytes(M, L, S); }

size_t jpdse_vq_index_workspace_size(int32_t M, int32_t L, int32_t S) { return vq_index_workspace_bytes(M, L, S); }

int jpdse_vq_index_encode(const jpdse_vq_index_encode_args* a) {
  if (int rc = vq_index_encode_check(a)) return rc;
  const int M = a->M, L = a->L, S = a->S, nb = vq_index_bits(L);
  // the workspace: the slots (nb M + 8 S bytes), then the lengths and the flags, int32 [S] each
  uint8_t* slots = mptr<uint8_t>(a->ws);
  int32_t* lens = reinterpret_cast<int32_t*>(slots + align_up((size_t)nb * M + 8 * (size_t)S, 16));
  int32_t* flags = lens + S;
  hipLaunchKernelGGL(vq_index_encode_kernel, dim3((S + 63) / 64), dim3(64), vq_index_lds_bytes(nb), as_stream(a->stream),
                     a->index, slots, lens, flags, M, L, S, nb);
  if (int rc = check_launch("vq_index_encode")) return rc;
  return launch256("vq_index_encode(compact)", vq_index_compact_kernel, dim3((S + 3) / 4), a->stream, slots, lens, flags, a->out,
                   a->size, a->status, M, S, nb);
}

int jpdse_vq_index_decode(const jpdse_vq_index_decode_args* a) {
  if (int rc = vq_index_decode_check(a)) return rc;
  const int nb = vq_index_bits(a->L);
  hipLaunchKernelGGL(vq_index_decode_kernel, dim3((a->S + 63) / 64), dim3(64), vq_index_lds_bytes(nb), as_stream(a->stream), a->in,
                     (long long)a->in_bytes, a->index, a->status, a->M, a->L, a->S, nb);
  return check_launch("vq_index_decode");
}

}  // extern "C"
