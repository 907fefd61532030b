"""Pure-Python restatement of the learned codec's entropy-coded bitstream (TEST INFRASTRUCTURE), written from the format text
of DESIGN.md 4.8 and from nothing else.  The binary coder, its carry counters and the payload layout are tests/rc_ref.py's;
this is the modelling:

  symbols   bit of element (c, y, x) = b > 0; every (image, channel) is one stream of H*W symbols, y then x
  context   left | up << 1 | upleft << 2 | upright << 3 from the coded bits of the same channel, 0 outside the frame;
            16 adaptive probabilities per stream
  payload   C little-endian uint32 stream lengths, then the C streams in channel order
"""
import numpy as np

from rc_ref import Counters, Encoder, Decoder, PROB_INIT, join_payload, split_payload  # noqa: F401  (Counters, split_payload: re-exported)


def stream_capacity(H, W):
  """Bytes one stream can never exceed: a probability stays within [31, 2017], so a symbol costs less than
  log2(2048 / 31) < 6.05 bits; H*W symbols and the 4 stored bytes of the flush fit in H*W + 8."""
  return H * W + 8


def encode_stream(bits, H, W, counters=None):
  """bits: H*W values of 0 / 1 in raster order -> the stream's bytes."""
  assert len(bits) == H * W
  probs, rc = [PROB_INIT] * 16, Encoder(counters)
  prev = [0] * (W + 2)                 # the row above, shifted by one: prev[x + 1] is the bit at x; zeros outside the frame
  for y in range(H):
    cur = [0] * (W + 2)
    for x in range(W):
      bit = bits[y * W + x]
      ctx = cur[x] | prev[x + 1] << 1 | prev[x] << 2 | prev[x + 2] << 3
      rc.encode(probs, ctx, bit)
      cur[x + 1] = bit
    prev = cur
  return rc.finish()


def decode_stream(data, H, W):
  """The H*W bits of a stream; bytes past the end of `data` read as 0, the symbol count is fixed."""
  probs, rc = [PROB_INIT] * 16, Decoder(data)
  bits = [0] * (H * W)
  prev = [0] * (W + 2)
  for y in range(H):
    cur = [0] * (W + 2)
    for x in range(W):
      ctx = cur[x] | prev[x + 1] << 1 | prev[x] << 2 | prev[x + 2] << 3
      bit = rc.decode(probs, ctx)
      cur[x + 1] = bit
      bits[y * W + x] = bit
    prev = cur
  return bits


def encode_image(b, counters=None):
  """b: [C, H, W] of any sign -> the image payload."""
  C, H, W = b.shape
  on = (np.asarray(b) > 0).astype(np.uint8).reshape(C, H * W)
  streams = [encode_stream(on[c].tolist(), H, W, counters) for c in range(C)]
  return join_payload(streams)


def decode_image(payload, C, H, W):
  """float32 [C, H, W] of +1 / -1."""
  rows = [decode_stream(s, H, W) for s in split_payload(payload, C)]
  return np.where(np.array(rows, dtype=np.uint8).reshape(C, H, W) > 0, np.float32(1), np.float32(-1)).astype(np.float32)


def encode(b, counters=None):
  """b: [N, C, H, W] -> list of N payloads."""
  return [encode_image(b[n], counters) for n in range(b.shape[0])]


def decode(payloads, C, H, W):
  return np.stack([decode_image(p, C, H, W) for p in payloads])
