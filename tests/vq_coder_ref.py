"""Pure-Python restatement of the coded index stream of the vector quantizer (TEST INFRASTRUCTURE), written from the format
text of DESIGN.md 4.14 and from nothing else.  The binary coder, its carry counters and the payload layout are
tests/rc_ref.py's (imported, not edited); this is the modelling:

  streams   the M indices, each in [0, L), are dealt to S streams by interleaving: stream s holds the symbols s, s + S, ...
  symbol    nb = max(1, bit_length(L - 1)) binary decisions, most significant bit first, through a bit tree: m = 1; the bit is
            coded with probs[m]; m = m << 1 | bit.  2^nb adaptive probabilities per stream, entry 0 unused
  payload   S little-endian uint32 stream lengths, then the S streams in order
  decoder   exactly ceil((M - s) / S) symbols per stream whatever the bytes are; a value >= L is written as L - 1 and reported
"""
from rc_ref import Counters, Encoder, Decoder, PROB_INIT, join_payload, split_payload  # noqa: F401  (Counters: re-exported)


def index_bits(L):
  return max(1, (L - 1).bit_length())


def stream_count(M, S, s):
  return (M - s + S - 1) // S


def stream_capacity(M, L, S, s):
  """Bytes stream s can never exceed: a probability stays within [31, 2017], so at most one normalisation (one byte)
  follows a decision; nb decisions per symbol and the flush fit in nb * count + 8."""
  return index_bits(L) * stream_count(M, S, s) + 8


def capacity(M, L, S):
  """4 S + the sum of the slots; the counts add up to M."""
  return 4 * S + sum(stream_capacity(M, L, S, s) for s in range(S))


def encode_stream(symbols, L, counters=None):
  nb = index_bits(L)
  probs, rc = [PROB_INIT] * (1 << nb), Encoder(counters)
  for v in symbols:
    assert 0 <= v < L
    m = 1
    for k in range(nb - 1, -1, -1):
      bit = (v >> k) & 1
      rc.encode(probs, m, bit)
      m = m << 1 | bit
  return rc.finish()


def decode_stream(data, count, L):
  """(`count` values in [0, L), clipped): bytes past the end of `data` read as 0; clipped: a decoded value was >= L."""
  nb = index_bits(L)
  probs, rc = [PROB_INIT] * (1 << nb), Decoder(data)
  out, clipped = [], False
  for _ in range(count):
    m = 1
    for _k in range(nb):
      m = m << 1 | rc.decode(probs, m)
    v = m - (1 << nb)
    if v >= L:
      v, clipped = L - 1, True
    out.append(v)
  return out, clipped


def encode(indices, L, S, counters=None):
  """indices: M integers in [0, L) -> the payload."""
  flat = [int(v) for v in indices]
  assert 1 <= S <= min(len(flat), 65535) and 2 <= L <= 512
  return join_payload([encode_stream(flat[s::S], L, counters) for s in range(S)])


def decode_streams(streams, M, L, S):
  """(the M indices, clipped) of S streams given as bytes."""
  out, clipped = [0] * M, False
  for s in range(S):
    out[s::S], c = decode_stream(streams[s], stream_count(M, S, s), L)
    clipped = clipped or c
  return out, clipped


def decode(payload, M, L, S):
  """The M indices of a payload; ValueError when the length table does not add up or a decoded value was >= L."""
  out, clipped = decode_streams(split_payload(payload, S), M, L, S)
  if clipped:
    raise ValueError('a decoded value outside [0, %d)' % L)
  return out
