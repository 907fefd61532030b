"""Pure-Python restatement of the coded label / instance maps (TEST INFRASTRUCTURE), written from the format text of
DESIGN.md 4.9 and from nothing else.  The binary coder is the one of 4.8 (tests/entropy_ref.py has its constants and the
carry counters); only the modelling is new:

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
import struct

import numpy as np

from entropy_ref import Counters, PROB_INIT, PROB_ONE, MOVE_BITS, TOP

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
  probs = [PROB_INIT] * N_PROBS
  low, rng, cache, cache_size = 0, 0xFFFFFFFF, 0, 1
  out = bytearray()
  stats = counters if counters is not None else Counters()

  def shift_low():
    nonlocal low, cache, cache_size
    if (low & 0xFFFFFFFF) < 0xFF000000 or (low >> 32) != 0:
      carry = low >> 32
      run = cache_size - 1
      stats.longest_run = max(stats.longest_run, run)
      stats.carries += carry
      if carry and run >= 2:
        stats.carries_into_run2 += 1
      out.append((cache + carry) & 0xFF)
      for _ in range(run):
        out.append((0xFF + carry) & 0xFF)
      cache_size = 0
      cache = (low >> 24) & 0xFF
    cache_size += 1
    low = (low & 0x00FFFFFF) << 8

  def code(ctx, bit):
    """One binary decision; ctx None: the fixed probability 1024, no update."""
    nonlocal low, rng
    p = PROB_INIT if ctx is None else probs[ctx]
    bound = (rng >> 11) * p
    if bit == 0:
      rng = bound
      if ctx is not None:
        probs[ctx] = p + ((PROB_ONE - p) >> MOVE_BITS)
    else:
      low += bound
      rng -= bound
      if ctx is not None:
        probs[ctx] = p - (p >> MOVE_BITS)
    while rng < TOP:
      rng = (rng << 8) & 0xFFFFFFFF
      shift_low()

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
        code(ctx, int(v == L))
        done = v == L
      if not done and has_u and not (has_l and U == L):
        code(8 + int(UL is not None and UL == L) if has_l else 10, int(v == U))
        done = v == U
      if not done:
        for k in range(nlit - 1, -1, -1):
          code(None, (v >> k) & 1)
  for _ in range(5):
    shift_low()
  assert out[0] == 0
  return bytes(out[1:])


def decode_stream(data, rows, W, plane):
  """The rows*W values of a stream; bytes past the end of `data` read as 0, the pixel count is fixed."""
  nlit = LITERAL_BITS[plane]
  probs = [PROB_INIT] * N_PROBS
  n = len(data)
  code = int.from_bytes((bytes(data[:4]) + b'\0\0\0\0')[:4], 'big')
  pos, rng = 4, 0xFFFFFFFF
  values = [0] * (rows * W)

  def bit_of(ctx):
    nonlocal code, rng, pos
    p = PROB_INIT if ctx is None else probs[ctx]
    bound = (rng >> 11) * p
    if code < bound:
      rng = bound
      if ctx is not None:
        probs[ctx] = p + ((PROB_ONE - p) >> MOVE_BITS)
      bit = 0
    else:
      rng -= bound
      code -= bound
      if ctx is not None:
        probs[ctx] = p - (p >> MOVE_BITS)
      bit = 1
    while rng < TOP:
      rng = (rng << 8) & 0xFFFFFFFF
      code = ((code << 8) & 0xFFFFFFFF) | (data[pos] if pos < n else 0)
      pos += 1
    return bit

  for y in range(rows):
    for x in range(W):
      has_l, has_u = x > 0, y > 0
      L = values[y * W + x - 1] if has_l else None
      U = values[(y - 1) * W + x] if has_u else None
      UL = values[(y - 1) * W + x - 1] if has_l and has_u else None
      v = None
      if has_l:
        ctx = int(has_u and L == U) | int(UL is not None and UL == L) << 1 | int(UL is not None and UL == U) << 2
        if bit_of(ctx):
          v = L
      if v is None and has_u and not (has_l and U == L):
        if bit_of(8 + int(UL is not None and UL == L) if has_l else 10):
          v = U
      if v is None:
        v = 0
        for _ in range(nlit):
          v = v << 1 | bit_of(None)
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
  return b''.join([struct.pack('<I', len(s)) for s in streams] + streams), cut


def split_payload(payload, S):
  if len(payload) < 4 * S:
    raise ValueError('payload of %d bytes is shorter than its table of %d lengths' % (len(payload), S))
  lens = struct.unpack('<%dI' % S, payload[:4 * S])
  if sum(lens) != len(payload) - 4 * S:
    raise ValueError('length table sums to %d, %d bytes follow it' % (sum(lens), len(payload) - 4 * S))
  out, at = [], 4 * S
  for n in lens:
    out.append(payload[at:at + n])
    at += n
  return out


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
