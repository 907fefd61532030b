"""Pure-Python restatement of the coded label / instance maps (TEST INFRASTRUCTURE), written from the format text of
DESIGN.md 4.9 and from nothing else.  The binary coder and the payload layout are those of 4.8 (tests/rc_ref.py has both, and
the carry counters); only the modelling is new:

  planes    0: label map, values 0..255, 8-bit literal, 1 raw byte;  1: instance map, values 0..2^31-1, 32-bit literal,
            4 raw bytes (little-endian int32)
  streams   every plane of every image is cut into strips of `strip_rows` rows (the last may be shorter); a strip is one
            independent stream with 11 adaptive probabilities and never looks above its first row
  pixel     L, U, UL = left, up, up-left inside the strip; a comparison with a neighbour that does not exist is false
            1. L exists: bit (v == L) in context (L==U) | (UL==L) << 1 | (UL==U) << 2            [probabilities 0..7]
            2. not equal to L (or no L), U exists and U != L: bit (v == U) in context 8 + (UL==L), or 10 without an L
            3. otherwise the value, most significant bit first, each bit at the fixed probability 1024 (no update)
  payload   of one plane of one image: S little-endian uint32 stream lengths, then the S streams in strip order
"""
import numpy as np

from rc_ref import Counters, Encoder, Decoder, PROB_INIT, join_payload, split_payload  # noqa: F401  (Counters, split_payload: re-exported)

LITERAL_BITS = (8, 32)
RAW_BYTES = (1, 4)
RAW_DTYPE = ('u1', '<i4')
N_PROBS = 11


def strips(H, strip_rows):
  """[(first row, rows)] of the strips of an H-row plane."""
  return [(y, min(strip_rows, H - y)) for y in range(0, H, strip_rows)]


def stream_capacity(plane, rows, W):
  """The slot of a strip: its raw size + 8.  NOT a bound of the format (a pixel can cost two adaptive decisions and a
  literal): a stream that needs more is cut, and the plane is then stored raw."""
  return rows * W * RAW_BYTES[plane] + 8


def plane_capacity(plane, H, W, strip_rows):
  return sum(4 + stream_capacity(plane, r, W) for _, r in strips(H, strip_rows))


def raw_size(plane, H, W):
  return H * W * RAW_BYTES[plane]


def encode_stream(values, rows, W, plane, counters=None):
  """values: rows*W ints in raster order -> the stream's bytes (uncut, whatever their number)."""
  assert len(values) == rows * W
  nlit = LITERAL_BITS[plane]
  probs, rc = [PROB_INIT] * N_PROBS, Encoder(counters)
  for y in range(rows):
    for x in range(W):
      v = values[y * W + x]
      has_l, has_u = x > 0, y > 0
      L = values[y * W + x - 1] if has_l else None
      U = values[(y - 1) * W + x] if has_u else None
      UL = values[(y - 1) * W + x - 1] if has_l and has_u else None
      done = False
      if has_l:
        ctx = int(has_u and L == U) | int(UL is not None and UL == L) << 1 | int(UL is not None and UL == U) << 2
        rc.encode(probs, ctx, int(v == L))
        done = v == L
      if not done and has_u and not (has_l and U == L):
        rc.encode(probs, 8 + int(UL is not None and UL == L) if has_l else 10, int(v == U))
        done = v == U
      if not done:
        for k in range(nlit - 1, -1, -1):
          rc.encode(probs, None, (v >> k) & 1)      # None: the fixed probability 1024, no update
  return rc.finish()


def decode_stream(data, rows, W, plane):
  """The rows*W values of a stream; bytes past the end of `data` read as 0, the pixel count is fixed."""
  nlit = LITERAL_BITS[plane]
  probs, rc = [PROB_INIT] * N_PROBS, Decoder(data)
  values = [0] * (rows * W)
  for y in range(rows):
    for x in range(W):
      has_l, has_u = x > 0, y > 0
      L = values[y * W + x - 1] if has_l else None
      U = values[(y - 1) * W + x] if has_u else None
      UL = values[(y - 1) * W + x - 1] if has_l and has_u else None
      v = None
      if has_l:
        ctx = int(has_u and L == U) | int(UL is not None and UL == L) << 1 | int(UL is not None and UL == U) << 2
        if rc.decode(probs, ctx):
          v = L
      if v is None and has_u and not (has_l and U == L):
        if rc.decode(probs, 8 + int(UL is not None and UL == L) if has_l else 10):
          v = U
      if v is None:
        v = 0
        for _ in range(nlit):
          v = v << 1 | rc.decode(probs, None)
      values[y * W + x] = v
  return values


def encode_plane(a, plane, strip_rows, counters=None):
  """a: integer [H, W] -> (payload, cut): the length table and the streams; cut: a stream outgrew its slot (its bytes are
  then clipped to the slot, as the device leaves them, and the plane is to be stored raw)."""
  H, W = a.shape
  a = np.asarray(a).astype(np.int64)
  assert a.min() >= 0 and a.max() < (256 if plane == 0 else 1 << 31)
  streams, cut = [], False
  for y0, rows in strips(H, strip_rows):
    s = encode_stream(a[y0:y0 + rows].reshape(-1).tolist(), rows, W, plane, counters)
    cap = stream_capacity(plane, rows, W)
    if len(s) > cap:
      s, cut = s[:cap], True
    streams.append(s)
  return join_payload(streams), cut


def decode_plane(payload, plane, H, W, strip_rows):
  """int64 [H, W]."""
  st = strips(H, strip_rows)
  rows = [decode_stream(s, r, W, plane) for s, (_, r) in zip(split_payload(payload, len(st)), st)]
  return np.array([v for r in rows for v in r], dtype=np.int64).reshape(H, W)


def raw_plane(a, plane):
  return np.ascontiguousarray(np.asarray(a).astype(RAW_DTYPE[plane])).tobytes()


def entry(a, plane, strip_rows, counters=None):
  """(mode, payload) as a file stores the plane: coded (1) unless a stream was cut or coding did not make it smaller."""
  payload, cut = encode_plane(a, plane, strip_rows, counters)
  if cut or len(payload) >= raw_size(plane, *a.shape):
    return 0, raw_plane(a, plane)
  return 1, payload
