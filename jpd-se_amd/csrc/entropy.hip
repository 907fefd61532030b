// Entropy-coded form of the learned codec's bitstream (no reference counterpart: the reference never writes a coded stream):
// a lossless, context-adaptive binary range coder for the code tensor, and its decoder.  Format: DESIGN.md 4.8.  Entry points:
// include/jpdse.h, "learned codec: entropy-coded bitstream".
//
// Every (image, channel) pair is one independent stream of H*W symbols (bit = b > 0, raster order) with its own 16 adaptive
// probabilities, selected by the four already-coded neighbours left | up << 1 | upleft << 2 | upright << 3.  The coder is the
// carry-propagating range coder of LZMA (I. Pavlov, LZMA SDK, public domain; 11-bit probabilities, shift 5): the work of one
// stream is serial, so one LANE codes one stream and lane = channel -- the 64 lanes of a wave read (or write) 64 neighbouring
// channels of one pixel of the NHWC tensor.  All streams of a call have the same H and W: the loops over y and x are
// wave-uniform, only the byte output (encoder) / input (decoder) diverges.  A lane's probability table and the bits of its
// previous row (32 per word) live in LDS columns that no other lane touches, so no barrier is needed.
#include "common.h"

namespace jpdse {

constexpr int kEntropyMaxW = 4096;             // 128 words of row bits per lane: (16 + 128) * 64 * 4 = 36 KiB of LDS
constexpr uint32_t kTop = 1u << 24;
constexpr uint32_t kProbInit = 1024, kProbOne = 2048;
constexpr int kMoveBits = 5;

static inline long long stream_cap(int H, int W) { return (long long)H * W + 8; }
// bytes of one image's payload at most: the table of C lengths and C full slots; 0: a shape the kernels do not take
static long long image_cap(int H, int W, int C) {
  if (H <= 0 || W <= 0 || C <= 0 || W > kEntropyMaxW) return 0;
  if (stream_cap(H, W) > 0x7fffffffLL / C) return 0;
  const long long cap = (4 + stream_cap(H, W)) * C;
  return cap <= 0x7fffffffLL ? cap : 0;
}
static inline size_t entropy_lds_bytes(int W) { return (size_t)(16 + (W + 31) / 32) * 64 * sizeof(uint32_t); }

// ctx of the symbol at bit k of the current word: upw = the row above (bit k = up), urw = the same shifted down by one
__device__ __forceinline__ uint32_t context_of(uint32_t left, uint32_t ul, uint32_t upw, uint32_t urw, int k) {
  return left | ((upw >> k) & 1u) << 1 | ul << 2 | ((urw >> k) & 1u) << 3;
}

// Phase 1 of the encoder: stream (n, c) into its slot of `scap` bytes; lens[n*C + c] = the bytes the stream needs (more than
// scap: it did not fit, the slot holds the first scap of them).  grid (ceil(C / 64), N), one wave per block.
template <typename T>
__global__ void __launch_bounds__(64) entropy_encode_kernel(const T* __restrict__ b, uint8_t* __restrict__ slots,
                                                            int32_t* __restrict__ lens, int H, int W, int C, int Cs,
                                                            int scap) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x, c = blockIdx.x * 64 + lane, n = blockIdx.y;
  if (c >= C) return;                           // no cross-lane operation below
  uint32_t* prob = lds + lane;                  // [16][64]
  uint32_t* row = lds + 16 * 64 + lane;         // [nw][64]: bit k of word j = the coded bit at x = 32 j + k of the row above
  const int nw = (W + 31) >> 5;
  for (int k = 0; k < 16; ++k) prob[k * 64] = kProbInit;
  for (int j = 0; j < nw; ++j) row[j * 64] = 0;
  const T* src = b + (long long)n * H * W * Cs + c;
  uint8_t* slot = slots + ((long long)n * C + c) * scap;

  uint64_t low = 0;
  uint32_t range = 0xFFFFFFFFu, cache = 0, cache_size = 1;
  int emitted = 0;                              // bytes emitted so far, the unstored first one included
  auto emit = [&](uint32_t byte) {
    if (emitted >= 1 && emitted <= scap) slot[emitted - 1] = (uint8_t)byte;      // clipped to the slot
    ++emitted;
  };
  auto shift_low = [&]() {
    if ((uint32_t)low < 0xFF000000u || (low >> 32) != 0) {
      const uint32_t carry = (uint32_t)(low >> 32);
      emit(cache + carry);
      for (uint32_t k = 1; k < cache_size; ++k) emit(0xFFu + carry);              // bounded by the bytes pending
      cache_size = 0;
      cache = (uint32_t)(low >> 24) & 0xFFu;
    }
    ++cache_size;
    low = (low & 0x00FFFFFFull) << 8;
  };

  for (int y = 0; y < H; ++y) {
    uint32_t upw = row[0], left = 0, ul = 0;
    for (int j = 0; j < nw; ++j) {
      const uint32_t nextw = j + 1 < nw ? row[(j + 1) * 64] : 0u;
      const uint32_t urw = (upw >> 1) | (nextw << 31);
      const int kmax = min(32, W - 32 * j);
      // the word's 32 input symbols first: independent loads, one memory latency per word instead of one per symbol
      const T* px = src + ((long long)y * W + 32 * j) * Cs;
      uint32_t inw = 0;
#pragma unroll
      for (int k = 0; k < 32; ++k)
        if (k < kmax) inw |= (uint32_t)(ElemOps<T>::ld(px + (long long)k * Cs) > 0.f) << k;
      for (int k = 0; k < kmax; ++k) {
        const uint32_t bit = (inw >> k) & 1u;
        const uint32_t ctx = context_of(left, ul, upw, urw, k);
        uint32_t p = prob[ctx * 64];
        const uint32_t bound = (range >> 11) * p;
        if (bit == 0) {
          range = bound;
          p += (kProbOne - p) >> kMoveBits;
        } else {
          low += bound;
          range -= bound;
          p -= p >> kMoveBits;
        }
        prob[ctx * 64] = p;
        // range >= 1 here (0 < bound < range), so three shifts always reach 2^24
        for (int it = 0; it < 3 && range < kTop; ++it) {
          range <<= 8;
          shift_low();
        }
        ul = (upw >> k) & 1u;
        left = bit;
      }
      row[j * 64] = inw;                        // bits beyond W stay 0: nothing is loaded for k >= kmax
      upw = nextw;
    }
  }
  for (int k = 0; k < 5; ++k) shift_low();
  lens[(long long)n * C + c] = emitted - 1;
}

// Phase 2: the payload of image n = C little-endian uint32 stream lengths, then the streams in channel order.  One wave per
// stream: it adds up the lengths in front of its own (C reads), writes its table entry and copies its slot.  The wave of the
// last channel also writes sizes[n] and status[n].  grid (ceil(C / 4), N), 256 threads.
__global__ void entropy_compact_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens,
                                       uint8_t* __restrict__ out, long long out_stride, int32_t* __restrict__ sizes,
                                       int32_t* __restrict__ status, int C, int scap) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
  if (c >= C) return;                           // wave-uniform
  const int32_t* ln = lens + (long long)n * C;
  int before = 0, overflow = 0;
  for (int j = lane; j < c; j += 64) {
    before += min(ln[j], scap);
    overflow |= ln[j] > scap;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    before += __shfl_xor(before, off, 64);
    overflow |= __shfl_xor(overflow, off, 64);
  }
  const int need = ln[c], len = min(need, scap);
  uint8_t* image = out + (long long)n * out_stride;
  if (lane < 4) image[4 * c + lane] = (uint8_t)((uint32_t)len >> (8 * lane));
  // 4 C + before + len <= (4 + scap) C, the capacity the host checked out_stride against
  uint8_t* dst = image + 4LL * C + before;
  const uint8_t* src = slots + ((long long)n * C + c) * scap;
  for (int i = lane; i < len; i += 64) dst[i] = src[i];
  if (c == C - 1 && lane == 0) {
    sizes[n] = 4 * C + before + len;
    status[n] = (overflow | (need > scap)) ? 1 : 0;
  }
}

// Decoder: lane c < C decodes stream (n, c) and writes +1 / -1 into its lane of b; the padding lanes C <= c < Cs write 0.
// The length table comes from the payload and is not trusted: every stream is clipped to its image's row of `stride` bytes,
// a byte past the end of a stream reads as 0, and the symbol count is H*W whatever the bytes are.
// grid (ceil(Cs / 64), N), one wave per block.
template <typename T>
__global__ void __launch_bounds__(64) entropy_decode_kernel(const uint8_t* __restrict__ in, long long stride,
                                                            T* __restrict__ b, int H, int W, int C, int Cs) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x, c0 = blockIdx.x * 64, c = c0 + lane, n = blockIdx.y;
  const uint8_t* image = in + (long long)n * stride;
  auto table = [&](int j) -> unsigned long long {            // 4 C <= stride: checked by the host
    if (j >= C) return 0;
    const uint8_t* t = image + 4LL * j;
    return (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  };
  // where the stream starts: the lengths of all channels in front of it (whole wave, before any lane leaves)
  unsigned long long base = 0;
  for (int j0 = 0; j0 < c0; j0 += 64) {
    unsigned long long v = table(j0 + lane);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    base += v;
  }
  const unsigned long long mine = table(c);
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (c >= Cs) return;
  T* dst = b + (long long)n * H * W * Cs + c;
  if (c >= C) {
    for (long long p = 0; p < (long long)H * W; ++p) ElemOps<T>::st(dst + p * Cs, 0.f);
    return;
  }
  // sums of up to C values below 2^32 cannot wrap 64 bits
  const unsigned long long ustride = (unsigned long long)stride;
  const unsigned long long start = min(4ull * C + base + (incl - mine), ustride);
  const unsigned long long end = min(start + mine, ustride);
  const uint8_t* sp = image + start;
  const long long slen = (long long)(end - start);
  long long rp = 0;
  uint32_t buf = 0;
  int nbuf = 0;
  auto next_byte = [&]() -> uint32_t {          // four bytes per refill: independent loads, zeros past the stream's end
    if (nbuf == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) buf = buf << 8 | (rp + i < slen ? (uint32_t)sp[rp + i] : 0u);
      rp += 4;
      nbuf = 4;
    }
    --nbuf;
    return (buf >> (8 * nbuf)) & 0xFFu;
  };

  uint32_t* prob = lds + lane;
  uint32_t* row = lds + 16 * 64 + lane;
  const int nw = (W + 31) >> 5;
  for (int k = 0; k < 16; ++k) prob[k * 64] = kProbInit;
  for (int j = 0; j < nw; ++j) row[j * 64] = 0;
  uint32_t range = 0xFFFFFFFFu, code = 0;
  for (int k = 0; k < 4; ++k) code = code << 8 | next_byte();

  for (int y = 0; y < H; ++y) {
    uint32_t upw = row[0], left = 0, ul = 0;
    for (int j = 0; j < nw; ++j) {
      const uint32_t nextw = j + 1 < nw ? row[(j + 1) * 64] : 0u;
      const uint32_t urw = (upw >> 1) | (nextw << 31);
      const int kmax = min(32, W - 32 * j);
      T* px = dst + ((long long)y * W + 32 * j) * Cs;
      uint32_t outw = 0;
      for (int k = 0; k < kmax; ++k) {
        const uint32_t ctx = context_of(left, ul, upw, urw, k);
        uint32_t p = prob[ctx * 64];
        const uint32_t bound = (range >> 11) * p;
        uint32_t bit;
        if (code < bound) {
          range = bound;
          p += (kProbOne - p) >> kMoveBits;
          bit = 0;
        } else {
          range -= bound;
          code -= bound;
          p -= p >> kMoveBits;
          bit = 1;
        }
        prob[ctx * 64] = p;
        for (int it = 0; it < 3 && range < kTop; ++it) {      // 0 < bound < range whatever `code` is: range >= 1
          range <<= 8;
          code = code << 8 | next_byte();
        }
        ElemOps<T>::st(px + (long long)k * Cs, bit ? 1.f : -1.f);
        outw |= bit << k;
        ul = (upw >> k) & 1u;
        left = bit;
      }
      row[j * 64] = outw;
      upw = nextw;
    }
  }
}

static int entropy_shape_check(const char* who, int dtype, int N, int H, int W, int C) {
  JPDSE_REQUIRE(!bad_dtype(dtype), "%s: bad dtype %d", who, dtype);
  JPDSE_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "%s: non-positive extent (N %d, H %d, W %d, C %d)", who, N, H, W, C);
  JPDSE_REQUIRE(N <= 65535 && image_cap(H, W, C) > 0,
                "%s: shape beyond the coder's limits (N %d <= 65535, W %d <= %d, payload capacity below 2^31 bytes)", who, N, W,
                kEntropyMaxW);
  return JPDSE_OK;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_code_entropy_capacity(int32_t H, int32_t W, int32_t C) { return (size_t)image_cap(H, W, C); }

size_t jpdse_code_entropy_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (N <= 0 || N > 65535 || image_cap(H, W, C) == 0) return 0;
  // the slots [N][C][H*W + 8] and the lengths int32 [N][C]
  return align_up((size_t)N * C * stream_cap(H, W), 16) + (size_t)N * C * sizeof(int32_t);
}

int jpdse_code_entropy_encode(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* b, uint8_t* out,
                              int64_t out_stride, int32_t* sizes, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = entropy_shape_check("code_entropy_encode", dtype, N, H, W, C)) return rc;
  JPDSE_REQUIRE(b && out && sizes && status, "code_entropy_encode: null pointer");
  const long long cap = image_cap(H, W, C);
  JPDSE_REQUIRE(out_stride >= cap, "code_entropy_encode: row stride %lld below the payload capacity %lld", (long long)out_stride,
                cap);
  if (ws == nullptr || ws_bytes < jpdse_code_entropy_workspace_size(N, H, W, C))
    return set_error(JPDSE_EWORKSPACE, "code_entropy_encode: workspace too small");
  const int Cs = cpad(C), scap = (int)stream_cap(H, W);
  uint8_t* slots = mptr<uint8_t>(ws);
  int32_t* lens = reinterpret_cast<int32_t*>(slots + align_up((size_t)N * C * scap, 16));
  if (int rc = by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(entropy_encode_kernel<T>, dim3((C + 63) / 64, N), dim3(64), entropy_lds_bytes(W), as_stream(stream),
                           cptr<T>(b), slots, lens, H, W, C, Cs, scap);
        return check_launch("code_entropy_encode");
      }))
    return rc;
  return launch256("code_entropy_encode(compact)", entropy_compact_kernel, dim3((C + 3) / 4, N), stream, slots, lens, out,
                   (long long)out_stride, sizes, status, C, scap);
}

int jpdse_code_entropy_decode(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const uint8_t* in, int64_t in_stride,
                              const int32_t* sizes, void* b, void* stream) {
  if (int rc = entropy_shape_check("code_entropy_decode", dtype, N, H, W, C)) return rc;
  JPDSE_REQUIRE(in && sizes && b, "code_entropy_decode: null pointer");
  JPDSE_REQUIRE(in_stride >= 4LL * C, "code_entropy_decode: row stride %lld below the %d-byte length table", (long long)in_stride,
                4 * C);
  for (int n = 0; n < N; ++n)
    JPDSE_REQUIRE(sizes[n] >= 4 * C && sizes[n] <= in_stride,
                  "code_entropy_decode: payload %d of %d bytes, outside [%d (its length table), %lld (the row stride)]", n,
                  sizes[n], 4 * C, (long long)in_stride);
  const int Cs = cpad(C);
  return by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(entropy_decode_kernel<T>, dim3((Cs + 63) / 64, N), dim3(64), entropy_lds_bytes(W), as_stream(stream), in,
                       (long long)in_stride, mptr<T>(b), H, W, C, Cs);
    return check_launch("code_entropy_decode");
  });
}

}  // extern "C"
