"""Pure-Python restatement of the learned codec's entropy-coded bitstream (TEST INFRASTRUCTURE), written from the format text
of DESIGN.md 4.8 and from nothing else: a context-adaptive binary range coder with carry propagation (the "rc" scheme of
LZMA: I. Pavlov's LZMA SDK, public domain; 11-bit probabilities, shift 5, 32-bit range, 64-bit low, cache / cacheSize).

  symbols   bit of element (c, y, x) = b > 0; every (image, channel) is one stream of H*W symbols, y then x
  context   left | up << 1 | upleft << 2 | upright << 3 from the coded bits of the same channel, 0 outside the frame;
            16 adaptive probabilities per stream
  stream    the bytes the coder emits without the first one (always 0)
  payload   C little-endian uint32 stream lengths, then the C streams in channel order

The encoder counts what the GPU tests need to know about their inputs: how often a carry was propagated, the longest run of
pending 0xFF bytes, and how often a carry went into a run of two or more (Counters)."""
import struct

import numpy as np

PROB_INIT, PROB_ONE, MOVE_BITS, TOP = 1024, 2048, 5, 1 << 24


class Counters(object):
  """carries: shiftLow calls that emitted with carry 1; longest_run: the most 0xFF bytes ever pending behind `cache`;
  carries_into_run2: carries that went through a pending run of length >= 2 (which they turn into 0x00 bytes)."""

  def __init__(self):
    self.carries, self.longest_run, self.carries_into_run2 = 0, 0, 0

  def add(self, other):
    self.carries += other.carries
    self.carries_into_run2 += other.carries_into_run2
    self.longest_run = max(self.longest_run, other.longest_run)


def stream_capacity(H, W):
  """Bytes one stream can never exceed: a probability stays within [31, 2017], so a symbol costs less than
  log2(2048 / 31) < 6.05 bits; H*W symbols and the 4 stored bytes of the flush fit in H*W + 8."""
  return H * W + 8


def encode_stream(bits, H, W, counters=None):
  """bits: H*W values of 0 / 1 in raster order -> the stream's bytes."""
  assert len(bits) == H * W
  probs = [PROB_INIT] * 16
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

  prev = [0] * (W + 2)                 # the row above, shifted by one: prev[x + 1] is the bit at x; zeros outside the frame
  for y in range(H):
    cur = [0] * (W + 2)
    for x in range(W):
      bit = bits[y * W + x]
      ctx = cur[x] | prev[x + 1] << 1 | prev[x] << 2 | prev[x + 2] << 3
      p = probs[ctx]
      bound = (rng >> 11) * p
      if bit == 0:
        rng = bound
        probs[ctx] = p + ((PROB_ONE - p) >> MOVE_BITS)
      else:
        low += bound
        rng -= bound
        probs[ctx] = p - (p >> MOVE_BITS)
      while rng < TOP:
        rng = (rng << 8) & 0xFFFFFFFF
        shift_low()
      cur[x + 1] = bit
    prev = cur
  for _ in range(5):
    shift_low()
  assert out[0] == 0
  return bytes(out[1:])


def decode_stream(data, H, W):
  """The H*W bits of a stream; bytes past the end of `data` read as 0, the symbol count is fixed."""
  probs = [PROB_INIT] * 16
  pos = 4
  code = int.from_bytes((bytes(data[:4]) + b'\0\0\0\0')[:4], 'big')
  rng = 0xFFFFFFFF
  n = len(data)
  bits = [0] * (H * W)
  prev = [0] * (W + 2)
  for y in range(H):
    cur = [0] * (W + 2)
    for x in range(W):
      ctx = cur[x] | prev[x + 1] << 1 | prev[x] << 2 | prev[x + 2] << 3
      p = probs[ctx]
      bound = (rng >> 11) * p
      if code < bound:
        rng = bound
        probs[ctx] = p + ((PROB_ONE - p) >> MOVE_BITS)
        bit = 0
      else:
        rng -= bound
        code -= bound
        probs[ctx] = p - (p >> MOVE_BITS)
        bit = 1
      while rng < TOP:
        rng = (rng << 8) & 0xFFFFFFFF
        code = ((code << 8) & 0xFFFFFFFF) | (data[pos] if pos < n else 0)
        pos += 1
      cur[x + 1] = bit
      bits[y * W + x] = bit
    prev = cur
  return bits


def encode_image(b, counters=None):
  """b: [C, H, W] of any sign -> the image payload."""
  C, H, W = b.shape
  on = (np.asarray(b) > 0).astype(np.uint8).reshape(C, H * W)
  streams = [encode_stream(on[c].tolist(), H, W, counters) for c in range(C)]
  return b''.join([struct.pack('<I', len(s)) for s in streams] + streams)


def split_payload(payload, C):
  """The C streams of a payload; ValueError when the length table does not add up to the bytes that follow it."""
  if len(payload) < 4 * C:
    raise ValueError('payload of %d bytes is shorter than its table of %d lengths' % (len(payload), C))
  lens = struct.unpack('<%dI' % C, payload[:4 * C])
  if sum(lens) != len(payload) - 4 * C:
    raise ValueError('length table sums to %d, %d bytes follow it' % (sum(lens), len(payload) - 4 * C))
  out, at = [], 4 * C
  for n in lens:
    out.append(payload[at:at + n])
    at += n
  return out


def decode_image(payload, C, H, W):
  """float32 [C, H, W] of +1 / -1."""
  rows = [decode_stream(s, H, W) for s in split_payload(payload, C)]
  return np.where(np.array(rows, dtype=np.uint8).reshape(C, H, W) > 0, np.float32(1), np.float32(-1)).astype(np.float32)


def encode(b, counters=None):
  """b: [N, C, H, W] -> list of N payloads."""
  return [encode_image(b[n], counters) for n in range(b.shape[0])]


def decode(payloads, C, H, W):
  return np.stack([decode_image(p, C, H, W) for p in payloads])
