// The coder core of entropy.hip, shared in parts with semantics.hip, code_rate.hip and code_cost.hip: the
// binary range coder of LZMA (the "rc" scheme; I. Pavlov, LZMA SDK, public domain; 11-bit probabilities of bit 0, shift 5), the payload
// layout -- a table of little-endian uint32 stream lengths, then the streams -- as the encoders write it and as the decoders
// read it from data they do not trust, and the model of the code tensor's streams: the context rule and the walk over a stream
// (code_walk) that entropy.hip codes with and code_cost.hip prices with.  The models of the other sources stay with them
// (the index coders: vq_model.h).  Device code only; plain C++ loads and stores.
//
// A model walk is a function template over a SINK: it visits the decisions of a stream in coding order and hands each one to
// sink.put(p, bit) -- p: the decision's adaptive probability word in the lane's LDS column, which put updates -- and the end
// of each symbol to sink.symbol_done(at), at: the symbol's position in the walked tensor.  RcEncoder is the sink that codes;
// CostPricer (cost_class.h) is the one that prices.
#pragma once
#include "common.h"

namespace jpdse {

constexpr uint32_t kTop = 1u << 24;
constexpr uint32_t kProbInit = 1024, kProbOne = 2048;
constexpr int kMoveBits = 5;

// The adaptive probability of bit 0 after `bit` was coded with q -- the ONE statement of the update the coders, the decoders
// and the pricing sink share.
__device__ __forceinline__ uint32_t adapted(uint32_t q, uint32_t bit) {
  return bit ? q - (q >> kMoveBits) : q + ((kProbOne - q) >> kMoveBits);
}

// One lane codes one stream into its slot of `scap` bytes.  A probability is passed by reference: it may live in an LDS
// column (prob[ctx * 64]).
struct RcEncoder {
  uint64_t low;
  uint32_t range, cache, cache_size;
  int emitted;                                  // bytes emitted so far, the unstored first one included; saturates at scap + 2
  uint8_t* slot;
  int scap;

  __device__ __forceinline__ void init(uint8_t* slot_, int scap_) {
    low = 0, range = 0xFFFFFFFFu, cache = 0, cache_size = 1, emitted = 0, slot = slot_, scap = scap_;
  }
  // Clipped to the slot.  The counter stops at scap + 2, so finish() returns scap + 1 for every stream that did not fit,
  // whatever it would have needed: callers read the length through min(len, scap) and len > scap only, and a counter that
  // cannot run away keeps the cost of a hostile input bounded.  (A stream of entropy.hip cannot outgrow its H*W + 8 bytes
  // at all; semantics.hip's strip encoder, whose streams can, has the same emit in its local copy.)
  __device__ __forceinline__ void emit(uint32_t byte) {
    if (emitted >= 1 && emitted <= scap) slot[emitted - 1] = (uint8_t)byte;
    if (emitted <= scap + 1) ++emitted;
  }
  __device__ __forceinline__ void shift_low() {
    if ((uint32_t)low < 0xFF000000u || (low >> 32) != 0) {
      const uint32_t carry = (uint32_t)(low >> 32);
      emit(cache + carry);
      for (uint32_t k = 1; k < cache_size; ++k) emit(0xFFu + carry);              // bounded by the bytes pending
      cache_size = 0;
      cache = (uint32_t)(low >> 24) & 0xFFu;
    }
    ++cache_size;
    low = (low & 0x00FFFFFFull) << 8;
  }
  __device__ __forceinline__ void split(uint32_t bound, uint32_t bit) {
    if (bit == 0) {
      range = bound;
    } else {
      low += bound;
      range -= bound;
    }
    // 2^17 < bound < range - 2^17 for every probability in [31, 2017]: one shift reaches 2^24; range >= 1
    // in any case, so three always do
    for (int it = 0; it < 3 && range < kTop; ++it) {
      range <<= 8;
      shift_low();
    }
  }
  // an adaptive decision
  __device__ __forceinline__ void encode(uint32_t& p, uint32_t bit) {
    const uint32_t q = p;
    p = adapted(q, bit);
    split((range >> 11) * q, bit);
  }
  // as the sink of a model walk.  A halfword of the index coders' columns is widened around the decision: its store stays
  // behind the byte emission, where those encoders have always had it
  __device__ __forceinline__ void put(uint32_t& p, uint32_t bit) { encode(p, bit); }
  __device__ __forceinline__ void put(uint16_t& p, uint32_t bit) { uint32_t q = p; encode(q, bit); p = (uint16_t)q; }
  __device__ __forceinline__ void symbol_done(long long) {}
  // the flush; returns the bytes the stream needs, or scap + 1 when they are more than scap
  __device__ __forceinline__ int finish() {
    for (int k = 0; k < 5; ++k) shift_low();
    return emitted - 1;
  }
};

// One lane decodes the stream sp[0 .. slen), already clipped to the input: a byte past its end reads as 0, so whatever the
// bytes are a caller that decodes a fixed number of decisions reads nothing else.
struct RcDecoder {
  const uint8_t* sp;
  long long slen, rp;
  uint32_t buf, range, code;
  int nbuf;

  __device__ __forceinline__ uint32_t next_byte() {         // four bytes per refill: independent loads
    if (nbuf == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) buf = buf << 8 | (rp + i < slen ? (uint32_t)sp[rp + i] : 0u);
      rp += 4;
      nbuf = 4;
    }
    --nbuf;
    return (buf >> (8 * nbuf)) & 0xFFu;
  }
  __device__ __forceinline__ void init(const uint8_t* sp_, long long slen_) {
    sp = sp_, slen = slen_, rp = 0, buf = 0, nbuf = 0, range = 0xFFFFFFFFu, code = 0;
    for (int k = 0; k < 4; ++k) code = code << 8 | next_byte();
  }
  __device__ __forceinline__ uint32_t split(uint32_t bound) {
    uint32_t bit = 0;
    if (code < bound) {
      range = bound;
    } else {
      range -= bound;
      code -= bound;
      bit = 1;
    }
    for (int it = 0; it < 3 && range < kTop; ++it) {         // 0 < bound < range whatever `code` is: range >= 1
      range <<= 8;
      code = code << 8 | next_byte();
    }
    return bit;
  }
  __device__ __forceinline__ uint32_t decode(uint32_t& p) {
    const uint32_t q = p, bit = split((range >> 11) * q);
    p = adapted(q, bit);
    return bit;
  }
};

// Where stream first + lane lies in an UNTRUSTED payload of `count` streams of which `have` bytes exist at `image`: the
// lane's [start, end) inside [0, have).  A table entry j >= count or one that does not lie inside the bytes present
// (4 j + 4 > have) reads as 0 and every stream is clipped to `have`, so a table that lies cannot make a decoder read
// outside the payload.  `first` is a multiple of 64.  Called by the whole wave, before any lane leaves.
struct StreamSpan {
  unsigned long long start, end;
};
__device__ __forceinline__ StreamSpan stream_span(const uint8_t* image, int count, int first, int lane, long long have) {
  auto table = [&](int j) -> unsigned long long {
    if (j >= count || 4LL * j + 4 > have) return 0;
    const uint8_t* t = image + 4LL * j;
    return (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  };
  // the lengths of all streams in front of the lane's; sums of up to 2^31 values below 2^32 cannot wrap 64 bits
  unsigned long long before = 0;
  for (int j0 = 0; j0 < first; j0 += 64) {
    unsigned long long v = table(j0 + lane);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    before += v;
  }
  const unsigned long long mine = table(first + lane);
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  const unsigned long long uhave = (unsigned long long)have;
  const unsigned long long start = min(4ull * count + before + (incl - mine), uhave);
  return StreamSpan{start, min(start + mine, uhave)};
}

// Second phase of an encoder, one WAVE per stream: stream s of the `count` whose lengths are lens[] (as finish() returned
// them) goes from its slot to its place in the payload at `image`, behind the table, whose entry s the wave writes too.
// cap(j): the slot size of stream j; flags: per-stream status bits to OR in, or nullptr.  Returns the payload's bytes up to
// the end of stream s and the OR over the streams 0 .. s of (length > cap) | flags: for s = count - 1, the payload's size
// and the status of all its streams.  The caller has checked the room at `image` against 4 count + the sum of the slots.
struct Compacted {
  int end, status;
};
template <typename Cap>
__device__ __forceinline__ Compacted compact_stream(uint8_t* __restrict__ image, const uint8_t* __restrict__ slot,
                                                    const int32_t* __restrict__ lens, const int32_t* __restrict__ flags,
                                                    int count, int s, int lane, Cap cap) {
  int before = 0, st = 0;
  for (int j = lane; j <= s; j += 64) {
    const int c = cap(j), need = lens[j];
    if (j < s) before += min(need, c);
    st |= (need > c ? 1 : 0) | (flags != nullptr ? flags[j] : 0);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    before += __shfl_xor(before, off, 64);
    st |= __shfl_xor(st, off, 64);
  }
  const int len = min(lens[s], cap(s));
  if (lane < 4) image[4 * s + lane] = (uint8_t)((uint32_t)len >> (8 * lane));
  uint8_t* dst = image + 4LL * count + before;
  for (int i = lane; i < len; i += 64) dst[i] = slot[i];
  return Compacted{4 * count + before + len, st};
}

// The context of a symbol of a code stream from its coded neighbours, left | up << 1 | upleft << 2 | upright << 3 -- the ONE
// statement of the rule code_walk and the decoder code with and the rate term prices with.  Every argument is one bit, 0
// outside the frame.
__device__ __forceinline__ uint32_t context_of(uint32_t left, uint32_t up, uint32_t upleft, uint32_t upright) {
  return left | up << 1 | upleft << 2 | upright << 3;
}

// The bits (b > 0) of the kmax <= 32 symbols at px, px + Cs, ...: independent loads, one memory latency per word instead of
// one per symbol.  Bits from kmax on are 0: nothing is loaded for them.
template <typename T>
__device__ __forceinline__ uint32_t load_bit_word(const T* px, int Cs, int kmax) {
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (k < kmax) w |= (uint32_t)(ElemOps<T>::ld(px + (long long)k * Cs) > 0.f) << k;
  return w;
}

// The walk over one stream of the code tensor -- the ONE statement of its model for the encoder and the cost map: the H x W
// symbols (bit = b > 0) at src, src + Cs, ... in raster order, 32 per loaded word, each one decision in the entry context_of
// selects from its coded neighbours.  prob: the lane's 16 entries, row: the bits of its previous row ((W + 31) / 32 words, bit
// k of word j = the bit at x = 32 j + k), both LDS columns of stride 64 the caller initialised (kProbInit, 0).  A symbol's
// position is y * W + x.  The sink travels by value and comes back: that form keeps the encoder on its measured code.
template <typename T, typename Sink>
__device__ __forceinline__ Sink code_walk(const T* src, uint32_t* prob, uint32_t* row, int H, int W, int Cs, Sink sink) {
  const int nw = (W + 31) >> 5;
  for (int y = 0; y < H; ++y) {
    uint32_t upw = row[0], left = 0, ul = 0;
    for (int j = 0; j < nw; ++j) {
      const uint32_t nextw = j + 1 < nw ? row[(j + 1) * 64] : 0u;
      const uint32_t urw = (upw >> 1) | (nextw << 31);
      const int kmax = min(32, W - 32 * j);
      const long long at = (long long)y * W + 32 * j;
      // the word's 32 input symbols before any of them is visited
      const uint32_t inw = load_bit_word(src + at * Cs, Cs, kmax);
      for (int k = 0; k < kmax; ++k) {
        const uint32_t bit = (inw >> k) & 1u, up = (upw >> k) & 1u;
        sink.put(prob[context_of(left, up, ul, (urw >> k) & 1u) * 64], bit);
        sink.symbol_done(at + k);
        ul = up;
        left = bit;
      }
      row[j * 64] = inw;                        // bits beyond W stay 0
      upw = nextw;
    }
  }
  return sink;
}

}  // namespace jpdse
