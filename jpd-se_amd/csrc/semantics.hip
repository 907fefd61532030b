// Coded label and instance maps (no reference counterpart: the reference hands the receiver its semantics for free): a
// lossless, context-adaptive coder for the two integer maps of a batch, and its decoder.  Format: DESIGN.md 4.9.  Entry
// points: include/jpdse.h, "learned codec: coded label and instance maps".
//
// Plane 0 is the label map (float32 [N][H][W] in, values 0..255, 8-bit literal), plane 1 the instance map (int64 [N][H][W],
// values 0..2^31-1, 32-bit literal): the tensors the input builder reads.  Every plane of every image is cut into strips of
// `strip_rows` rows; a strip is one independent stream with 11 adaptive probabilities that never looks above its first row.
// A pixel is "equal to the left one", else "equal to the upper one", else a literal; the binary decisions go through the
// range coder of 4.8 (LZMA's rc; I. Pavlov, LZMA SDK, public domain).  The work of a stream is serial, so one LANE codes one
// strip: lane = strip, blockIdx.y = image, blockIdx.z = plane.  Lanes of a wave sit strip_rows * W elements apart, so every
// lane reads its row in chunks of 16 pixels with independent (and, where the row pitch allows, 16-byte) loads and stages them
// in an LDS column of its own next to its probabilities: no other lane touches a column, so no barrier is needed.  The row
// above comes from the input (encoder) or from what the same lane has already written to the output (decoder).
//
// The coder's constants and the second phase of the encoder (compact_stream) are range_coder.h's.  The strip encoder and
// decoder keep the coder's arithmetic and the reader of the length table as local code, a second copy of what RcEncoder,
// RcDecoder and stream_span hold: each is one serial, latency-bound loop, and through the shared structs its time moved by
// -6 % to +9 % with the input and with where the compiler put the same instructions (profiles/rc_refactor_ab.txt).  They
// stay on the form whose machine code is the measured one; the tests hold both copies to the same bytes.
#include "range_coder.h"

namespace jpdse {

constexpr int kSemProbs = 11;                  // 8 contexts of "== left", 3 of "== up"
constexpr int kSemChunk = 16;                  // pixels per staged chunk
constexpr int kSemLdsWords = (kSemProbs + 2 * kSemChunk) * 64;      // probabilities, the chunk, the chunk above it
constexpr int kSemMaxN = 65535, kSemMaxStrips = 65535;

struct SemLabel {
  typedef float Elem;
  static constexpr int kBits = 8, kRaw = 1, kId = 0;
  // the value coded for f, and whether f is a label at all (an integer in [0, 255]; NaN is not)
  __device__ static __forceinline__ uint32_t get(float f, uint32_t& bad) {
    const bool ok = f >= 0.f && f <= 255.f && f == truncf(f);
    bad |= ok ? 0u : 2u;
    return (uint32_t)fminf(fmaxf(f, 0.f), 255.f);
  }
  __device__ static __forceinline__ uint32_t back(float f) { return (uint32_t)f; }       // of a value `put` wrote
  __device__ static __forceinline__ float put(uint32_t v) { return (float)v; }
};
struct SemInst {
  typedef long long Elem;
  static constexpr int kBits = 32, kRaw = 4, kId = 1;
  __device__ static __forceinline__ uint32_t get(long long v, uint32_t& bad) {
    bad |= (v >= 0 && v < (1LL << 31)) ? 0u : 2u;
    return (uint32_t)v & 0x7fffffffu;
  }
  __device__ static __forceinline__ uint32_t back(long long v) { return (uint32_t)v; }
  __device__ static __forceinline__ long long put(uint32_t v) { return (long long)v; }
};

struct SemGeom {
  int N, H, W, sr, S;                          // sr: rows of a full strip (clipped to H); S: strips per image
  __host__ __device__ int rows(int s) const { return min(sr, H - s * sr); }
  // the slot of strip s of a plane with `raw` bytes per pixel: its raw size + 8
  __host__ __device__ int scap(int s, int raw) const { return rows(s) * W * raw + 8; }
};
struct SemEncPlane {
  int id;                                      // 0 label, 1 instance
  int vec;                                     // the rows of this plane can be read with 16-byte loads
  uint8_t* slots;                              // [N][S][slot_stride]
  int32_t* lens;                               // [N][S]
  long long slot_stride, out_off;              // out_off: where the plane's payload starts in an image's row of `out`
};
struct SemEncArgs {
  SemGeom g;
  const float* label;
  const long long* inst;
  SemEncPlane p[2];
};
struct SemDecArgs {
  SemGeom g;
  const uint8_t* in;
  long long stride;
  const int32_t* sizes;                        // [N][2], untrusted
  long long off[2], len[2];                    // the region of plane id inside a row, checked by the host
  int id[2], vec[2];
  float* label;
  long long* inst;
  int32_t* bad;                                // [N]
  int num_labels;
};

static inline int sem_strips(int H, int strip_rows) { return (int)(((long long)H + strip_rows - 1) / strip_rows); }
// bytes of one plane's payload at most: S table entries and S slots
static inline long long sem_plane_cap(int H, int W, int S, int raw) { return (long long)H * W * raw + 12LL * S; }
// 0: a shape the kernels do not take
static long long sem_image_cap(int H, int W, int strip_rows, int mask) {
  if (H <= 0 || W <= 0 || strip_rows <= 0 || mask < 1 || mask > 3) return 0;
  const long long S = sem_strips(H, strip_rows);
  if (S > kSemMaxStrips || (long long)H * W > 0x7fffffffLL / 5) return 0;
  const long long cap = ((mask & 1) ? sem_plane_cap(H, W, (int)S, 1) : 0) + ((mask & 2) ? sem_plane_cap(H, W, (int)S, 4) : 0);
  return cap <= 0x7fffffffLL ? cap : 0;
}
static inline long long sem_slot_stride(int H, int W, int strip_rows, int raw) {
  return (long long)min(strip_rows, H) * W * raw + 8;
}

// CH elements from p (cnt of them exist) with independent loads -- 16-byte ones when `vec` -- handed to sink(k, value)
template <typename T, typename F>
__device__ __forceinline__ void sem_load_chunk(const T* p, int cnt, bool vec, F&& sink) {
  constexpr int VN = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VN)));
  if (vec) {                                   // W is a multiple of VN and the plane is 16-byte aligned: so is cnt, so is p
#pragma unroll
    for (int i = 0; i < kSemChunk / VN; ++i)
      if (i * VN < cnt) {
        const VT t = *reinterpret_cast<const VT*>(p + i * VN);
#pragma unroll
        for (int j = 0; j < VN; ++j) sink(i * VN + j, t[j]);
      }
  } else {
#pragma unroll
    for (int k = 0; k < kSemChunk; ++k)
      if (k < cnt) sink(k, p[k]);
  }
}

// Phase 1 of the encoder: strip s of image n of plane P into its slot; lens = the bytes the stream needs, or scap + 1 when
// they are more than the slot's scap (the slot then holds the first scap of them).  Returns the out-of-range flag (2 or 0).
template <typename P>
__device__ __forceinline__ uint32_t sem_encode_strip(const typename P::Elem* __restrict__ img, const SemGeom& g, int s, bool vec,
                                                     uint8_t* __restrict__ slot, int32_t* __restrict__ len_out, uint32_t* lds) {
  typedef typename P::Elem T;
  const int lane = threadIdx.x, W = g.W, rows = g.rows(s), scap = g.scap(s, P::kRaw);
  uint32_t* prob = lds + lane;                                   // [11][64]
  uint32_t* cur = lds + kSemProbs * 64 + lane;                   // [16][64]: the chunk being coded
  uint32_t* upc = lds + (kSemProbs + kSemChunk) * 64 + lane;     // [16][64]: the same columns of the row above
  for (int k = 0; k < kSemProbs; ++k) prob[k * 64] = kProbInit;

  uint64_t low = 0;
  uint32_t range = 0xFFFFFFFFu, cache = 0, cache_size = 1, bad = 0;
  int emitted = 0;                              // bytes emitted so far, the unstored first one included; saturates at scap + 2
  auto emit = [&](uint32_t byte) {
    if (emitted >= 1 && emitted <= scap) slot[emitted - 1] = (uint8_t)byte;      // clipped to the slot
    if (emitted <= scap + 1) ++emitted;
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
  auto split = [&](uint32_t bound, uint32_t bit) {
    if (bit == 0) {
      range = bound;
    } else {
      low += bound;
      range -= bound;
    }
    // 2^17 < bound < range - 2^17 for every probability in [31, 2017]: one shift reaches 2^24
    for (int it = 0; it < 3 && range < kTop; ++it) {
      range <<= 8;
      shift_low();
    }
  };
  auto code = [&](int ctx, uint32_t bit) {
    uint32_t p = prob[ctx * 64];
    const uint32_t bound = (range >> 11) * p;
    p = bit ? p - (p >> kMoveBits) : p + ((kProbOne - p) >> kMoveBits);
    prob[ctx * 64] = p;
    split(bound, bit);
  };

  const int nch = (W + kSemChunk - 1) / kSemChunk;
  const T* base = img + (long long)s * g.sr * W;
  uint32_t rv[kSemChunk] = {}, ru[kSemChunk] = {};
  // the loads of chunk (sy, j): the pixels and, below the strip's first row, the pixels above them
  auto fetch = [&](int sy, int j) {
    const T* px = base + (long long)sy * W + j * kSemChunk;
    const int cnt = min(kSemChunk, W - j * kSemChunk);
    sem_load_chunk(px, cnt, vec, [&](int k, T v) { rv[k] = P::get(v, bad); });
    uint32_t ignored = 0;                       // a row above is also some chunk's own row: flagged there
    if (sy > 0) sem_load_chunk(px - W, cnt, vec, [&](int k, T v) { ru[k] = P::get(v, ignored); });
  };
  if (rows > 0) fetch(0, 0);
  for (int sy = 0; sy < rows; ++sy) {
    uint32_t L = 0, UL = 0;
    for (int j = 0; j < nch; ++j) {
      const int cnt = min(kSemChunk, W - j * kSemChunk);
#pragma unroll
      for (int k = 0; k < kSemChunk; ++k) {
        cur[k * 64] = rv[k];
        upc[k * 64] = ru[k];
      }
      // the next chunk's loads are in flight while this one is coded
      if (j + 1 < nch) fetch(sy, j + 1);
      else if (sy + 1 < rows) fetch(sy + 1, 0);
      for (int k = 0; k < cnt; ++k) {
        const uint32_t v = cur[k * 64], U = upc[k * 64];
        const bool hasL = (j | k) != 0, hasU = sy > 0, both = hasL && hasU;
        const bool lu = both && L == U, ull = both && UL == L, ulu = both && UL == U;
        bool done = false;
        if (hasL) {
          code((int)lu | (int)ull << 1 | (int)ulu << 2, v == L);
          done = v == L;
        }
        if (!done && hasU && !lu) {
          code(hasL ? 8 + (int)ull : 10, v == U);
          done = v == U;
        }
        if (!done) {
          for (int b = P::kBits - 1; b >= 0; --b) split((range >> 11) << 10, (v >> b) & 1u);
        }
        UL = U;
        L = v;
      }
    }
  }
  for (int k = 0; k < 5; ++k) shift_low();
  *len_out = emitted - 1;
  return bad;
}

// grid (ceil(S / 64), N, planes), one wave per block.  oor[(n * 2 + plane) * S + s] = the strip's out-of-range flag.
__global__ void __launch_bounds__(64) semantics_encode_kernel(SemEncArgs a, int32_t* __restrict__ oor) {
  __shared__ uint32_t lds[kSemLdsWords];
  const SemGeom& g = a.g;
  const int s = blockIdx.x * 64 + threadIdx.x, n = blockIdx.y;
  if (s >= g.S) return;                         // no cross-lane operation below
  const SemEncPlane& pl = a.p[blockIdx.z];
  const long long at = (long long)n * g.S + s;
  uint32_t bad;
  if (pl.id == 0)
    bad = sem_encode_strip<SemLabel>(a.label + (long long)n * g.H * g.W, g, s, pl.vec != 0, pl.slots + at * pl.slot_stride,
                                     pl.lens + at, lds);
  else
    bad = sem_encode_strip<SemInst>(a.inst + (long long)n * g.H * g.W, g, s, pl.vec != 0, pl.slots + at * pl.slot_stride,
                                    pl.lens + at, lds);
  oor[((long long)n * 2 + pl.id) * g.S + s] = (int32_t)bad;
}

// Phase 2: the payload of plane p of image n = S little-endian uint32 stream lengths, then the streams in strip order, at
// out_off of the image's row.  One wave per stream (compact_stream); the wave of the last strip also writes sizes[n][plane]
// and status[n][plane].  grid (ceil(S / 4), N, planes), 256 threads.
__global__ void semantics_compact_kernel(SemEncArgs a, const int32_t* __restrict__ oor, uint8_t* __restrict__ out,
                                         long long out_stride, int32_t* __restrict__ sizes, int32_t* __restrict__ status) {
  const SemGeom& g = a.g;
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y, S = g.S;
  if (s >= S) return;                           // wave-uniform
  const SemEncPlane& pl = a.p[blockIdx.z];
  const int raw = pl.id == 0 ? 1 : 4;
  // the host checked out_stride against the plane's capacity: 4 S + the sum of all slots
  const Compacted r = compact_stream(out + (long long)n * out_stride + pl.out_off, pl.slots + ((long long)n * S + s) * pl.slot_stride,
                                     pl.lens + (long long)n * S, oor + ((long long)n * 2 + pl.id) * S, S, s, lane,
                                     [&](int j) { return g.scap(j, raw); });
  if (s == S - 1 && lane == 0) {
    sizes[2 * n + pl.id] = r.end;
    status[2 * n + pl.id] = r.status;
  }
}

// Decoder of one strip.  `sp`, `slen`: the stream, already clipped to the input; a byte past its end reads as 0 and the
// pixel count is fixed, so whatever the bytes are the lane writes its rows * W pixels and nothing else.  Returns the flags
// of what it decoded: 1 a label >= num_labels, 2 an instance value >= 2^31.
template <typename P>
__device__ __forceinline__ uint32_t sem_decode_strip(typename P::Elem* img, const SemGeom& g, int s, bool vec,
                                                     const uint8_t* __restrict__ sp, long long slen, uint32_t limit,
                                                     uint32_t* lds) {
  typedef typename P::Elem T;
  const int lane = threadIdx.x, W = g.W, rows = g.rows(s);
  uint32_t* prob = lds + lane;
  uint32_t* upc = lds + (kSemProbs + kSemChunk) * 64 + lane;
  for (int k = 0; k < kSemProbs; ++k) prob[k * 64] = kProbInit;
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
  uint32_t range = 0xFFFFFFFFu, code = 0, flags = 0;
  for (int k = 0; k < 4; ++k) code = code << 8 | next_byte();
  auto split = [&](uint32_t bound) -> uint32_t {
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
  };
  auto decode = [&](int ctx) -> uint32_t {
    uint32_t p = prob[ctx * 64];
    const uint32_t bit = split((range >> 11) * p);
    p = bit ? p - (p >> kMoveBits) : p + ((kProbOne - p) >> kMoveBits);
    prob[ctx * 64] = p;
    return bit;
  };

  const int nch = (W + kSemChunk - 1) / kSemChunk;
  T* base = img + (long long)s * g.sr * W;
  for (int sy = 0; sy < rows; ++sy) {
    uint32_t L = 0, UL = 0;
    for (int j = 0; j < nch; ++j) {
      const int cnt = min(kSemChunk, W - j * kSemChunk);
      T* px = base + (long long)sy * W + j * kSemChunk;
      if (sy > 0) {
        // the row above: what this lane stored one row ago
        uint32_t ru[kSemChunk] = {};
        sem_load_chunk(const_cast<const T*>(px - W), cnt, vec, [&](int k, T v) { ru[k] = P::back(v); });
#pragma unroll
        for (int k = 0; k < kSemChunk; ++k) upc[k * 64] = ru[k];
      }
      for (int k = 0; k < cnt; ++k) {
        const bool hasL = (j | k) != 0, hasU = sy > 0, both = hasL && hasU;
        const uint32_t U = hasU ? upc[k * 64] : 0u;
        const bool lu = both && L == U, ull = both && UL == L, ulu = both && UL == U;
        bool done = false;
        uint32_t v = 0;
        if (hasL && decode((int)lu | (int)ull << 1 | (int)ulu << 2)) {
          v = L;
          done = true;
        }
        if (!done && hasU && !lu && decode(hasL ? 8 + (int)ull : 10)) {
          v = U;
          done = true;
        }
        if (!done) {
          for (int b = 0; b < P::kBits; ++b) v = v << 1 | split((range >> 11) << 10);
        }
        flags |= v >= limit ? (P::kId == 0 ? 1u : 2u) : 0u;
        px[k] = P::put(v);
        UL = U;
        L = v;
      }
    }
  }
  return flags;
}

// grid (ceil(S / 64), N, planes), one wave per block.  Nothing in the payload is trusted: the size of a plane's payload is
// clipped to its region of the row, a table entry that does not lie inside it reads as 0, every stream is clipped to the
// region, and the pixel count is fixed.  sizes[n][plane] <= 0: that plane of that image is not coded here, nothing is written.
__global__ void __launch_bounds__(64) semantics_decode_kernel(SemDecArgs a) {
  __shared__ uint32_t lds[kSemLdsWords];
  const SemGeom& g = a.g;
  const int lane = threadIdx.x, s0 = blockIdx.x * 64, s = s0 + lane, n = blockIdx.y, S = g.S;
  const int z = blockIdx.z, id = a.id[z];
  const long long have = min((long long)a.sizes[2 * n + id], a.len[id]);
  if (have <= 0) return;                        // block-uniform
  const uint8_t* image = a.in + (long long)n * a.stride + a.off[id];
  auto table = [&](int j) -> unsigned long long {
    if (j >= S || 4LL * j + 4 > have) return 0;
    const uint8_t* t = image + 4LL * j;
    return (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  };
  // where the stream starts: the lengths of all strips in front of it (whole wave, before any lane leaves)
  unsigned long long before = 0;
  for (int j0 = 0; j0 < s0; j0 += 64) {
    unsigned long long v = table(j0 + lane);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    before += v;
  }
  const unsigned long long mine = table(s);
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (s >= S) return;
  // sums of up to S values below 2^32 cannot wrap 64 bits
  const unsigned long long uhave = (unsigned long long)have;
  const unsigned long long start = min(4ull * S + before + (incl - mine), uhave);
  const unsigned long long end = min(start + mine, uhave);
  uint32_t flags;
  if (id == 0)
    flags = sem_decode_strip<SemLabel>(a.label + (long long)n * g.H * g.W, g, s, a.vec[z] != 0, image + start,
                                       (long long)(end - start), (uint32_t)a.num_labels, lds);
  else
    flags = sem_decode_strip<SemInst>(a.inst + (long long)n * g.H * g.W, g, s, a.vec[z] != 0, image + start,
                                      (long long)(end - start), 0x80000000u, lds);
  if (flags) atomicOr(a.bad + n, (int)flags);
}

static int sem_shape_check(const char* who, int N, int H, int W, int strip_rows, int mask) {
  JPDSE_REQUIRE(N > 0 && H > 0 && W > 0, "%s: non-positive extent (N %d, H %d, W %d)", who, N, H, W);
  JPDSE_REQUIRE(strip_rows > 0, "%s: non-positive strip_rows %d", who, strip_rows);
  JPDSE_REQUIRE(mask >= 1 && mask <= 3, "%s: plane mask %d is empty or unknown (bit 0: label, bit 1: instance)", who, mask);
  JPDSE_REQUIRE(N <= kSemMaxN && sem_image_cap(H, W, strip_rows, mask) > 0,
                "%s: shape beyond the coder's limits (N %d <= %d, %d strips per image <= %d, payload capacity below 2^31 bytes)",
                who, N, kSemMaxN, sem_strips(H, strip_rows), kSemMaxStrips);
  return JPDSE_OK;
}
static inline SemGeom sem_geom(int N, int H, int W, int strip_rows) {
  return SemGeom{N, H, W, min(strip_rows, H), sem_strips(H, strip_rows)};
}
// rows of W elements of `size` bytes from p can be read in 16-byte pieces
static inline int sem_vec_ok(const void* p, int W, int size) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ((long long)W * size) % 16 == 0;
}

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_semantics_capacity(int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask) {
  return (size_t)sem_image_cap(H, W, strip_rows, plane_mask);
}

size_t jpdse_semantics_workspace_size(int32_t N, int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask) {
  if (N <= 0 || N > kSemMaxN || sem_image_cap(H, W, strip_rows, plane_mask) == 0) return 0;
  const size_t S = sem_strips(H, strip_rows);
  // the out-of-range flags int32 [N][2][S]; per present plane the slots [N][S][min(strip_rows, H) * W * raw + 8] and the
  // lengths int32 [N][S]
  size_t bytes = align_up((size_t)N * 2 * S * sizeof(int32_t), 16);
  for (int id = 0; id < 2; ++id)
    if (plane_mask >> id & 1)
      bytes += align_up((size_t)N * S * sem_slot_stride(H, W, strip_rows, id ? 4 : 1), 16) +
               align_up((size_t)N * S * sizeof(int32_t), 16);
  return bytes;
}

int jpdse_semantics_encode(int32_t N, int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask, const float* label,
                           const int64_t* inst, uint8_t* out, int64_t out_stride, int32_t* sizes, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream) {
  if (int rc = sem_shape_check("semantics_encode", N, H, W, strip_rows, plane_mask)) return rc;
  JPDSE_REQUIRE(out && sizes && status, "semantics_encode: null pointer");
  JPDSE_REQUIRE(!(plane_mask & 1) || label, "semantics_encode: the plane mask %d names the label plane, but label is NULL", plane_mask);
  JPDSE_REQUIRE(!(plane_mask & 2) || inst, "semantics_encode: the plane mask %d names the instance plane, but inst is NULL", plane_mask);
  const long long cap = sem_image_cap(H, W, strip_rows, plane_mask);
  JPDSE_REQUIRE(out_stride >= cap, "semantics_encode: row stride %lld below the payload capacity %lld", (long long)out_stride, cap);
  if (ws == nullptr || ws_bytes < jpdse_semantics_workspace_size(N, H, W, strip_rows, plane_mask))
    return set_error(JPDSE_EWORKSPACE, "semantics_encode: workspace too small");
  SemEncArgs a{};
  a.g = sem_geom(N, H, W, strip_rows);
  a.label = label;
  a.inst = reinterpret_cast<const long long*>(inst);
  const size_t S = a.g.S;
  uint8_t* at = mptr<uint8_t>(ws);
  int32_t* oor = reinterpret_cast<int32_t*>(at);
  at += align_up((size_t)N * 2 * S * sizeof(int32_t), 16);
  int np = 0;
  long long out_off = 0;
  for (int id = 0; id < 2; ++id) {
    if (!(plane_mask >> id & 1)) continue;
    SemEncPlane& pl = a.p[np++];
    pl.id = id;
    pl.vec = id ? sem_vec_ok(inst, W, 8) : sem_vec_ok(label, W, 4);
    pl.slot_stride = sem_slot_stride(H, W, strip_rows, id ? 4 : 1);
    pl.slots = at;
    at += align_up((size_t)N * S * pl.slot_stride, 16);
    pl.lens = reinterpret_cast<int32_t*>(at);
    at += align_up((size_t)N * S * sizeof(int32_t), 16);
    pl.out_off = out_off;
    out_off += sem_plane_cap(H, W, (int)S, id ? 4 : 1);
  }
  hipLaunchKernelGGL(semantics_encode_kernel, dim3((a.g.S + 63) / 64, N, np), dim3(64), 0, as_stream(stream), a, oor);
  if (int rc = check_launch("semantics_encode")) return rc;
  return launch256("semantics_encode(compact)", semantics_compact_kernel, dim3((a.g.S + 3) / 4, N, np), stream, a, oor, out,
                   (long long)out_stride, sizes, status);
}

int jpdse_semantics_decode(int32_t N, int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask, int32_t num_labels,
                           const uint8_t* in, int64_t in_stride, int64_t inst_offset, const int32_t* sizes, float* label,
                           int64_t* inst, int32_t* bad, void* stream) {
  if (int rc = sem_shape_check("semantics_decode", N, H, W, strip_rows, plane_mask)) return rc;
  JPDSE_REQUIRE(in && sizes && bad, "semantics_decode: null pointer");
  JPDSE_REQUIRE(!(plane_mask & 1) || label, "semantics_decode: the plane mask %d names the label plane, but label is NULL", plane_mask);
  JPDSE_REQUIRE(!(plane_mask & 2) || inst, "semantics_decode: the plane mask %d names the instance plane, but inst is NULL", plane_mask);
  JPDSE_REQUIRE(num_labels >= 1 && num_labels <= 256, "semantics_decode: num_labels %d outside [1, 256]", num_labels);
  SemDecArgs a{};
  a.g = sem_geom(N, H, W, strip_rows);
  const long long table = 4LL * a.g.S;
  if (plane_mask == 3) {
    JPDSE_REQUIRE(inst_offset >= table && in_stride - inst_offset >= table && inst_offset <= in_stride,
                  "semantics_decode: row stride %lld and instance offset %lld leave a plane less than its %lld-byte length table",
                  (long long)in_stride, (long long)inst_offset, table);
  } else {
    JPDSE_REQUIRE(in_stride >= table, "semantics_decode: row stride %lld below the %lld-byte length table", (long long)in_stride,
                  table);
    inst_offset = 0;
  }
  a.in = in;
  a.stride = in_stride;
  a.sizes = sizes;
  a.off[0] = 0;
  a.len[0] = plane_mask == 3 ? inst_offset : in_stride;
  a.off[1] = inst_offset;
  a.len[1] = in_stride - inst_offset;
  int np = 0;
  for (int id = 0; id < 2; ++id)
    if (plane_mask >> id & 1) {
      a.id[np] = id;
      a.vec[np++] = id ? sem_vec_ok(inst, W, 8) : sem_vec_ok(label, W, 4);
    }
  a.label = label;
  a.inst = reinterpret_cast<long long*>(inst);
  a.bad = bad;
  a.num_labels = num_labels;
  if (hipMemsetAsync(bad, 0, (size_t)N * sizeof(int32_t), as_stream(stream)) != hipSuccess)
    return set_error(JPDSE_ELAUNCH, "semantics_decode: clearing the flags failed");
  hipLaunchKernelGGL(semantics_decode_kernel, dim3((a.g.S + 63) / 64, N, np), dim3(64), 0, as_stream(stream), a);
  return check_launch("semantics_decode");
}

}  // extern "C"
