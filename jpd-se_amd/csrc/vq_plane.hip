// Spatial-context coder of the S2HVQ bottleneck's index planes (no reference counterpart): the code of one image as the
// feature map it is -- h x w pixels, G channel groups per pixel -- coded with the neighbour-match flags of the label-map
// coder in front of the adaptive literal of the order-0 index coder (4.14).  Format: DESIGN.md 4.19.  Entry
// points: include/jpdse.h, "soft-to-hard vector quantizer: coded index planes"; argument checks and the closed forms of the
// sizes: api.cpp.
//
// The plane of a group is cut into strips of strip_rows rows; stream s = k * G + g is strip k of group g, so lane = stream and
// the lanes of a wave that share a strip read (encoder) or write (decoder) consecutive int32 words per step.  A symbol is at
// most two flag decisions (equal to the left cell? equal to the upper cell?) and, when neither matched, the nb decisions of
// 4.14's bit tree; every decision is range_coder.h's RcEncoder::encode / RcDecoder::decode, and the payload layout,
// stream_span and compact_stream are that header's too.  A lane's table -- 11 flag probabilities at the entries 0 .. 10, tree
// node m at entry 10 + m -- is a private LDS column in the layout of vq_col.h (no barrier).  One wave per block,
// (10 + 2^nb) * 128 bytes of LDS: 66,816 bytes at nb = 9, which the launch opts in for (vq_plane_lds_optin).
#include "range_coder.h"
#include "vq_col.h"
#include "vq_model.h"

namespace jpdse {

// The slot of stream s (its geometry: vq_model.h) in the workspace.  Only the last strip is short: the streams of the strips in
// front of stream s have full slots of (nb + 2) * strip_rows * w + 8 bytes, the g streams of its own strip in front of it have
// slots of its own size -- the slots are packed and add up to (nb + 2) M + 8 S
__device__ __forceinline__ int plane_slot_bytes(int rows, int w, int nb) { return (nb + 2) * rows * w + 8; }
__device__ __forceinline__ long long plane_slot_offset(int s, PlaneStream st, int w, int strip_rows, int nb) {
  return (long long)(s - st.g) * plane_slot_bytes(strip_rows, w, nb) + (long long)st.g * plane_slot_bytes(st.rows, w, nb);
}

// one adaptive decision with the lane's table entry e
__device__ __forceinline__ void plane_put(RcEncoder& rc, uint16_t* prob, int e, uint32_t bit) {
  uint32_t p = prob[e * 64];
  rc.encode(p, bit);
  prob[e * 64] = (uint16_t)p;
}
__device__ __forceinline__ uint32_t plane_get(RcDecoder& rc, uint16_t* prob, int e) {
  uint32_t p = prob[e * 64];
  const uint32_t bit = rc.decode(p);
  prob[e * 64] = (uint16_t)p;
  return bit;
}

// Phase 1 of the encoder: stream s into its slot; lens[s] = the bytes it needs (slot size + 1: it did not fit, unreachable by
// the bound of DESIGN.md 4.19), flags[s] = 2 when the stream met an index outside [0, L).  The upper neighbour is read from
// the input (the upper-left one is the upper neighbour of the step before), the left one stays in a register.
// grid ceil(S / 64), one wave per block, (10 + 2^nb) * 128 bytes of dynamic LDS.
__global__ void __launch_bounds__(64) vq_plane_encode_kernel(const int32_t* __restrict__ index, uint8_t* __restrict__ slots,
                                                             int32_t* __restrict__ lens, int32_t* __restrict__ flags, int h,
                                                             int w, int G, int L, int strip_rows, int S, int nb) {
  extern __shared__ uint16_t plane_prob[];
  const int lane = threadIdx.x, s = blockIdx.x * 64 + lane;
  if (s >= S) return;                           // no cross-lane operation below
  uint16_t* prob = plane_prob + vq_col(lane);   // [10 + 2^nb][64]
  plane_table_init(prob, nb);
  const PlaneStream st = plane_stream(s, h, G, strip_rows);
  RcEncoder rc;
  rc.init(slots + plane_slot_offset(s, st, w, strip_rows, nb), plane_slot_bytes(st.rows, w, nb));
  const long long rowstep = (long long)w * G;
  const int32_t* cell = index + ((long long)st.y0 * w) * G + st.g;      // the cell of the step; the next one is cell + G
  int bad = 0, lf = 0, u = 0, ul = 0;
  // the words of the next step are loaded before the current one is coded
  int32_t next = cell[0], next_u = 0;
  for (int row = 0; row < st.rows; ++row) {
    for (int x = 0; x < w; ++x, cell += G) {
      const int v = plane_clean(next, L, bad);
      const bool has_l = x > 0, has_u = row > 0;
      if (has_u) {
        ul = u;                                 // of the cell to the left: used with has_l only
        u = plane_clean(next_u, L, bad);
      }
      if (x + 1 < w || row + 1 < st.rows) {
        next = cell[G];
        if (row > 0 || x + 1 == w) next_u = cell[G - rowstep];
      }
      const bool has_ul = has_l && has_u;
      bool matched = false;
      if (has_l) {
        const int e = (has_u && lf == u ? 1 : 0) | (has_ul && ul == lf ? 2 : 0) | (has_ul && ul == u ? 4 : 0);
        matched = v == lf;
        plane_put(rc, prob, e, matched ? 1u : 0u);
      }
      if (!matched && has_u && !(has_l && u == lf)) {
        const int e = has_l ? kPlaneUp + (ul == lf ? 1 : 0) : kPlaneUpOnly;
        matched = v == u;
        plane_put(rc, prob, e, matched ? 1u : 0u);
      }
      if (!matched) {
        uint32_t m = 1;
        for (int k = nb - 1; k >= 0; --k) {
          const uint32_t bit = ((uint32_t)v >> k) & 1u;
          plane_put(rc, prob, kPlaneTree + (int)m, bit);
          m = m << 1 | bit;
        }
      }
      lf = v;
    }
  }
  lens[s] = rc.finish();
  flags[s] = bad;
}

// Phase 2: the S little-endian uint32 stream lengths, then the streams in order.  One wave per stream (compact_stream); the
// wave of the last stream also writes the payload's size and the status word (bit 0: a cut stream, bit 1: a bad index).
// grid ceil(S / 4), 256 threads.
__global__ void vq_plane_compact_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens,
                                        const int32_t* __restrict__ flags, uint8_t* __restrict__ out, int32_t* __restrict__ size,
                                        int32_t* __restrict__ status, int h, int w, int G, int strip_rows, int S, int nb) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;                           // wave-uniform
  // the host checked the room at `out` against 4 S + the sum of the slots
  const uint8_t* slot = slots + plane_slot_offset(s, plane_stream(s, h, G, strip_rows), w, strip_rows, nb);
  const Compacted c = compact_stream(out, slot, lens, flags, S, s, lane, [=](int j) {
    return plane_slot_bytes(plane_stream(j, h, G, strip_rows).rows, w, nb);
  });
  if (s == S - 1 && lane == 0) {
    *size = c.end;
    *status = c.status;
  }
}

// Decoder: lane s decodes exactly rows * w symbols from its stream, whatever the bytes are, and writes them to the cells of
// its strip.  The length table is device data it does not trust: every stream is clipped to the `have` bytes of the payload
// (stream_span; 4 S <= have: checked by the host) and a byte past a stream's end reads as 0.  A literal is taken as read (it
// need not differ from its neighbours); a value >= L is written as L - 1, which is also what later symbols see as their
// neighbour, and sets bit 1 of *status with a plain store.  The upper neighbour is read back from the output this lane wrote a
// row earlier (same lane, program order; at w = 1 it is the symbol of the step before and never leaves the register).
// grid ceil(S / 64), one wave per block, (10 + 2^nb) * 128 bytes of dynamic LDS.
__global__ void __launch_bounds__(64) vq_plane_decode_kernel(const uint8_t* __restrict__ in, long long have, int32_t* index,
                                                             int32_t* __restrict__ status, int h, int w, int G, int L,
                                                             int strip_rows, int S, int nb) {
  extern __shared__ uint16_t plane_prob[];
  const int lane = threadIdx.x, s0 = blockIdx.x * 64, s = s0 + lane;
  const StreamSpan span = stream_span(in, S, s0, lane, have);
  if (s >= S) return;
  uint16_t* prob = plane_prob + vq_col(lane);
  plane_table_init(prob, nb);
  const PlaneStream st = plane_stream(s, h, G, strip_rows);
  RcDecoder rc;
  rc.init(in + span.start, (long long)(span.end - span.start));
  const long long rowstep = (long long)w * G;
  int32_t* cell = index + ((long long)st.y0 * w) * G + st.g;
  bool bad = false;
  int lf = 0, u = 0, ul = 0, next_u = 0;
  for (int row = 0; row < st.rows; ++row) {
    for (int x = 0; x < w; ++x, cell += G) {
      const bool has_l = x > 0, has_u = row > 0;
      if (has_u) {
        ul = u;
        u = next_u;
      }
      // the next step's upper neighbour was written at least one step ago when w > 1: its load overlaps this step's decisions
      if (w > 1 && (x + 1 < w ? row > 0 : row + 1 < st.rows)) next_u = cell[G - rowstep];
      const bool has_ul = has_l && has_u;
      bool matched = false;
      int v = 0;
      if (has_l) {
        const int e = (has_u && lf == u ? 1 : 0) | (has_ul && ul == lf ? 2 : 0) | (has_ul && ul == u ? 4 : 0);
        matched = plane_get(rc, prob, e) != 0;
        v = lf;
      }
      if (!matched && has_u && !(has_l && u == lf)) {
        const int e = has_l ? kPlaneUp + (ul == lf ? 1 : 0) : kPlaneUpOnly;
        matched = plane_get(rc, prob, e) != 0;
        v = u;
      }
      if (!matched) {
        uint32_t m = 1;
        for (int k = 0; k < nb; ++k) m = m << 1 | plane_get(rc, prob, kPlaneTree + (int)m);
        v = (int)(m - (1u << nb));
        if (v >= L) {
          v = L - 1;
          bad = true;
        }
      }
      cell[0] = v;
      lf = v;
      if (w == 1) next_u = v;
    }
  }
  if (bad) *status = 2;                         // every writer stores the same word
}

static inline size_t vq_plane_lds_bytes(int nb) { return (size_t)(kPlaneTree + (1 << nb)) * 64 * sizeof(uint16_t); }

}  // namespace jpdse

using namespace jpdse;

extern "C" {

size_t jpdse_vq_plane_capacity(int32_t h, int32_t w, int32_t G, int32_t L, int32_t strip_rows) {
  return (size_t)vq_plane_capacity_bytes(h, w, G, L, strip_rows);
}

size_t jpdse_vq_plane_workspace_size(int32_t h, int32_t w, int32_t G, int32_t L, int32_t strip_rows) {
  return vq_plane_workspace_bytes(h, w, G, L, strip_rows);
}

int jpdse_vq_plane_encode(const jpdse_vq_plane_encode_args* a) {
  if (int rc = vq_plane_encode_check(a)) return rc;
  const int h = a->h, w = a->w, G = a->G, L = a->L, rows = a->strip_rows, nb = vq_index_bits(L);
  const int S = vq_plane_streams(h, G, rows);
  // the workspace: the slots ((nb + 2) M + 8 S bytes), then the lengths and the flags, int32 [S] each
  uint8_t* slots = mptr<uint8_t>(a->ws);
  int32_t* lens = reinterpret_cast<int32_t*>(slots + align_up((size_t)(nb + 2) * h * w * G + 8 * (size_t)S, 16));
  int32_t* flags = lens + S;
  const size_t lds = vq_plane_lds_bytes(nb);
  if (int rc = vq_plane_lds_optin("vq_plane_encode", vq_plane_encode_kernel, lds)) return rc;
  hipLaunchKernelGGL(vq_plane_encode_kernel, dim3((S + 63) / 64), dim3(64), lds, as_stream(a->stream), a->index, slots, lens,
                     flags, h, w, G, L, rows, S, nb);
  if (int rc = check_launch("vq_plane_encode")) return rc;
  return launch256("vq_plane_encode(compact)", vq_plane_compact_kernel, dim3((S + 3) / 4), a->stream, slots, lens, flags, a->out,
                   a->size, a->status, h, w, G, rows, S, nb);
}

int jpdse_vq_plane_decode(const jpdse_vq_plane_decode_args* a) {
  if (int rc = vq_plane_decode_check(a)) return rc;
  const int nb = vq_index_bits(a->L), S = vq_plane_streams(a->h, a->G, a->strip_rows);
  const size_t lds = vq_plane_lds_bytes(nb);
  if (int rc = vq_plane_lds_optin("vq_plane_decode", vq_plane_decode_kernel, lds)) return rc;
  hipLaunchKernelGGL(vq_plane_decode_kernel, dim3((S + 63) / 64), dim3(64), lds, as_stream(a->stream), a->in,
                     (long long)a->in_bytes, a->index, a->status, a->h, a->w, a->G, a->L, a->strip_rows, S, nb);
  return check_launch("vq_plane_decode");
}

}  // extern "C"
