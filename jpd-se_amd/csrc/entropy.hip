// Entropy-coded form of the learned codec's bitstream (no reference counterpart: the reference never writes a coded stream):
// a lossless, context-adaptive binary range coder for the code tensor, and its decoder.  Format: DESIGN.md 4.8.  Entry points:
// include/jpdse.h, "learned codec: entropy-coded bitstream".
//
// Every (image, channel) pair is one independent stream of H*W symbols (bit = b > 0, raster order) with its own 16 adaptive
// probabilities, selected by the four already-coded neighbours.  The coder core, the payload layout, the context rule and the
// encoder's walk over a stream (code_walk, shared with the cost map of code_cost.hip) are range_coder.h's; this file is the
// kernels around them and the decoder's loop.  The work of one stream is serial, so one LANE codes one
// stream and lane = channel -- the 64 lanes of a wave read (or write) 64 neighbouring channels of one pixel of the NHWC
// tensor.  All streams of a call have the same H and W: the loops over y and x are wave-uniform, only the byte output
// (encoder) / input (decoder) diverges.  A lane's probability table and the bits of its previous row (32 per word) live in
// LDS columns that no other lane touches, so no barrier is needed.
#include "range_coder.h"

namespace jpdse {

constexpr int kEntropyMaxW = 4096;             // 128 words of row bits per lane: (16 + 128) * 64 * 4 = 36 KiB of LDS

static inline long long stream_cap(int H, int W) { return (long long)H * W + 8; }
// bytes of one image's payload at most: the table of C lengths and C full slots; 0: a shape the kernels do not take
static long long image_cap(int H, int W, int C) {
  if (H <= 0 || W <= 0 || C <= 0 || W > kEntropyMaxW) return 0;
  if (stream_cap(H, W) > 0x7fffffffLL / C) return 0;
  const long long cap = (4 + stream_cap(H, W)) * C;
  return cap <= 0x7fffffffLL ? cap : 0;
}
static inline size_t entropy_lds_bytes(int W) { return (size_t)(16 + (W + 31) / 32) * 64 * sizeof(uint32_t); }

// Phase 1 of the encoder: stream (n, c) into its slot of `scap` bytes; lens[n*C + c] = the bytes the stream needs (scap + 1:
// it did not fit, the slot holds the first scap of them -- unreachable).  grid (ceil(C / 64), N), one wave
// per block.
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
  RcEncoder rc;
  rc.init(slots + ((long long)n * C + c) * scap, scap);
  rc = code_walk(src, prob, row, H, W, Cs, rc);
  lens[(long long)n * C + c] = rc.finish();
}

// Phase 2: the payload of image n = C little-endian uint32 stream lengths, then the streams in channel order.  One wave per
// stream (compact_stream); the wave of the last channel also writes sizes[n] and status[n].  grid (ceil(C / 4), N), 256
// threads.
__global__ void entropy_compact_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens,
                                       uint8_t* __restrict__ out, long long out_stride, int32_t* __restrict__ sizes,
                                       int32_t* __restrict__ status, int C, int scap) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
  if (c >= C) return;                           // wave-uniform
  // the host checked out_stride against (4 + scap) C
  const Compacted r = compact_stream(out + (long long)n * out_stride, slots + ((long long)n * C + c) * scap,
                                     lens + (long long)n * C, nullptr, C, c, lane, [=](int) { return scap; });
  if (c == C - 1 && lane == 0) {
    sizes[n] = r.end;
    status[n] = r.status;
  }
}

// Decoder: lane c < C decodes stream (n, c) and writes +1 / -1 into its lane of b; the padding lanes C <= c < Cs write 0.
// The length table comes from the payload and is not trusted: every stream is clipped to its image's row of `stride` bytes
// (stream_span; 4 C <= stride: checked by the host), a byte past the end of a stream reads as 0, and the symbol count is
// H*W whatever the bytes are.
// grid (ceil(Cs / 64), N), one wave per block.
template <typename T>
__global__ void __launch_bounds__(64) entropy_decode_kernel(const uint8_t* __restrict__ in, long long stride,
                                                            T* __restrict__ b, int H, int W, int C, int Cs) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x, c0 = blockIdx.x * 64, c = c0 + lane, n = blockIdx.y;
  const uint8_t* image = in + (long long)n * stride;
  const StreamSpan span = stream_span(image, C, c0, lane, stride);
  if (c >= Cs) return;
  T* dst = b + (long long)n * H * W * Cs + c;
  if (c >= C) {
    for (long long p = 0; p < (long long)H * W; ++p) ElemOps<T>::st(dst + p * Cs, 0.f);
    return;
  }
  uint32_t* prob = lds + lane;
  uint32_t* row = lds + 16 * 64 + lane;
  const int nw = (W + 31) >> 5;
  for (int k = 0; k < 16; ++k) prob[k * 64] = kProbInit;
  for (int j = 0; j < nw; ++j) row[j * 64] = 0;
  RcDecoder rc;
  rc.init(image + span.start, (long long)(span.end - span.start));

  for (int y = 0; y < H; ++y) {
    uint32_t upw = row[0], left = 0, ul = 0;
    for (int j = 0; j < nw; ++j) {
      const uint32_t nextw = j + 1 < nw ? row[(j + 1) * 64] : 0u;
      const uint32_t urw = (upw >> 1) | (nextw << 31);
      const int kmax = min(32, W - 32 * j);
      T* px = dst + ((long long)y * W + 32 * j) * Cs;
      uint32_t outw = 0;
      for (int k = 0; k < kmax; ++k) {
        const uint32_t up = (upw >> k) & 1u;
        const uint32_t bit = rc.decode(prob[context_of(left, up, ul, (urw >> k) & 1u) * 64]);
        ElemOps<T>::st(px + (long long)k * Cs, bit ? 1.f : -1.f);
        outw |= bit << k;
        ul = up;
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
