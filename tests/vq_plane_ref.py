"""Pure-Python restatement of the spatial-context coder of the S2HVQ index planes (TEST INFRASTRUCTURE), written from the
format text of DESIGN.md 4.19 and from nothing else.  The binary coder, its carry counters and the payload layout are
tests/rc_ref.py's (imported, not edited); this is the modelling:

  input     flat[(y * w + x) * G + g], each in [0, L): h x w pixels in raster order, G groups ascending inside a pixel
  streams   the plane of a group is cut into K = ceil(h / strip_rows) strips; stream s = k * G + g is strip k of group g,
            rows * w symbols in raster order, its own table, no look above the strip's first row
  symbol    1. with a left cell Lf: the bit v == Lf, table entry (Lf == U) | (UL == Lf) << 1 | (UL == U) << 2
            2. no bit 1 yet, an upper cell U, and U != Lf (true without Lf): the bit v == U, entry 8 + (UL == Lf), 10 without Lf
            3. no bit 1 yet: v through the bit tree, nb decisions, most significant bit first, node m at entry 10 + m
            a comparison with a cell that does not exist is false; a table is 10 + 2^nb adaptive probabilities
  payload   S = K * G little-endian uint32 stream lengths, then the S streams in order
  decoder   exactly rows * w symbols per stream whatever the bytes are; a literal is taken as read; a value >= L is written
            -- and seen by later symbols -- as L - 1 and reported
"""
from rc_ref import Counters, Encoder, Decoder, PROB_INIT, join_payload, split_payload  # noqa: F401  (Counters: re-exported)


def index_bits(L):
  return max(1, (L - 1).bit_length())


def strips(h, strip_rows):
  return (h + strip_rows - 1) // strip_rows


def stream_count(h, w, strip_rows, k):
  return min(strip_rows, h - k * strip_rows) * w


def stream_capacity(h, w, L, strip_rows, k):
  """Bytes a stream of strip k can never exceed: every decision is adaptive, so at most one byte follows each; a symbol has at
  most nb + 2 decisions; the flush fits in the 8."""
  return (index_bits(L) + 2) * stream_count(h, w, strip_rows, k) + 8


def capacity(h, w, G, L, strip_rows):
  K = strips(h, strip_rows)
  return 4 * K * G + G * sum(stream_capacity(h, w, L, strip_rows, k) for k in range(K))


def _flag_entries(lf, u, ul):
  """(entry of the left flag, entry of the upper flag) from the neighbours, None for a cell that does not exist."""
  eq = lambda a, b: a is not None and b is not None and a == b
  left = (1 if eq(lf, u) else 0) | (2 if eq(ul, lf) else 0) | (4 if eq(ul, u) else 0)
  up = 8 + (1 if eq(ul, lf) else 0) if lf is not None else 10
  return left, up


def encode_stream(rows, L, counters=None):
  """rows: the strip of one group as a list of rows of values in [0, L)."""
  nb = index_bits(L)
  probs, rc = [PROB_INIT] * (10 + (1 << nb)), Encoder(counters)
  for y, row in enumerate(rows):
    for x, v in enumerate(row):
      assert 0 <= v < L
      lf = row[x - 1] if x > 0 else None
      u = rows[y - 1][x] if y > 0 else None
      ul = rows[y - 1][x - 1] if x > 0 and y > 0 else None
      left, up = _flag_entries(lf, u, ul)
      hit = False
      if lf is not None:
        hit = v == lf
        rc.encode(probs, left, int(hit))
      if not hit and u is not None and u != lf:
        hit = v == u
        rc.encode(probs, up, int(hit))
      if not hit:
        m = 1
        for k in range(nb - 1, -1, -1):
          bit = (v >> k) & 1
          rc.encode(probs, 10 + m, bit)
          m = m << 1 | bit
  return rc.finish()


def decode_stream(data, n_rows, w, L):
  """(the strip as a list of rows of values in [0, L), clipped): bytes past the end of `data` read as 0."""
  nb = index_bits(L)
  probs, rc = [PROB_INIT] * (10 + (1 << nb)), Decoder(data)
  rows, clipped = [], False
  for y in range(n_rows):
    row = []
    for x in range(w):
      lf = row[x - 1] if x > 0 else None
      u = rows[y - 1][x] if y > 0 else None
      ul = rows[y - 1][x - 1] if x > 0 and y > 0 else None
      left, up = _flag_entries(lf, u, ul)
      v = None
      if lf is not None and rc.decode(probs, left):
        v = lf
      if v is None and u is not None and u != lf and rc.decode(probs, up):
        v = u
      if v is None:
        m = 1
        for _k in range(nb):
          m = m << 1 | rc.decode(probs, 10 + m)
        v = m - (1 << nb)
        if v >= L:
          v, clipped = L - 1, True
      row.append(v)
    rows.append(row)
  return rows, clipped


def _strip_rows_of(flat, h, w, G, strip_rows, k, g):
  y0 = k * strip_rows
  return [[flat[(y * w + x) * G + g] for x in range(w)] for y in range(y0, min(y0 + strip_rows, h))]


def encode(indices, h, w, G, L, strip_rows, counters=None):
  """indices: h * w * G integers in [0, L) -> the payload."""
  flat = [int(v) for v in indices]
  K = strips(h, strip_rows)
  assert len(flat) == h * w * G and strip_rows >= 1 and 2 <= L <= 512 and K * G <= 65535
  return join_payload([encode_stream(_strip_rows_of(flat, h, w, G, strip_rows, k, g), L, counters)
                       for k in range(K) for g in range(G)])


def decode_streams(streams, h, w, G, L, strip_rows):
  """(the h * w * G indices, clipped) of S streams given as bytes."""
  out, clipped = [0] * (h * w * G), False
  for k in range(strips(h, strip_rows)):
    y0 = k * strip_rows
    for g in range(G):
      rows, c = decode_stream(streams[k * G + g], min(strip_rows, h - y0), w, L)
      clipped = clipped or c
      for dy, row in enumerate(rows):
        for x, v in enumerate(row):
          out[((y0 + dy) * w + x) * G + g] = v
  return out, clipped


def decode(payload, h, w, G, L, strip_rows):
  """The indices of a payload; ValueError when the length table does not add up or a decoded value was >= L."""
  out, clipped = decode_streams(split_payload(payload, strips(h, strip_rows) * G), h, w, G, L, strip_rows)
  if clipped:
    raise ValueError('a decoded value outside [0, %d)' % L)
  return out
