"""Pure-Python restatement of the binary range coder and the payload layout that the coded bitstream (tests/entropy_ref.py)
and the coded label / instance maps (tests/semantics_ref.py) share (TEST INFRASTRUCTURE), written from the format text of
DESIGN.md 4.8 and from nothing else: the carry-propagating "rc" scheme of LZMA (I. Pavlov's LZMA SDK, public domain; 11-bit
probabilities of bit 0, shift 5, 32-bit range, 64-bit low, cache / cacheSize).

  stream    the bytes the coder emits without the first one (always 0)
  payload   `count` little-endian uint32 stream lengths, then the streams in order

The encoder counts what the GPU tests need to know about their inputs: how often a carry was propagated, the longest run of
pending 0xFF bytes, and how often a carry went into a run of two or more (Counters)."""
import struct

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


class Encoder(object):
  def __init__(self, counters=None):
    self.low, self.rng, self.cache, self.cache_size = 0, 0xFFFFFFFF, 0, 1
    self.out = bytearray()
    self.stats = counters if counters is not None else Counters()

  def shift_low(self):
    if (self.low & 0xFFFFFFFF) < 0xFF000000 or (self.low >> 32) != 0:
      carry = self.low >> 32
      run = self.cache_size - 1
      self.stats.longest_run = max(self.stats.longest_run, run)
      self.stats.carries += carry
      if carry and run >= 2:
        self.stats.carries_into_run2 += 1
      self.out.append((self.cache + carry) & 0xFF)
      for _ in range(run):
        self.out.append((0xFF + carry) & 0xFF)
      self.cache_size = 0
      self.cache = (self.low >> 24) & 0xFF
    self.cache_size += 1
    self.low = (self.low & 0x00FFFFFF) << 8

  def encode(self, probs, ctx, bit):
    """One binary decision with the adaptive probability probs[ctx]; ctx None: the fixed probability 1024, no update."""
    p = PROB_INIT if ctx is None else probs[ctx]
    bound = (self.rng >> 11) * p
    if bit == 0:
      self.rng = bound
      if ctx is not None:
        probs[ctx] = p + ((PROB_ONE - p) >> MOVE_BITS)
    else:
      self.low += bound
      self.rng -= bound
      if ctx is not None:
        probs[ctx] = p - (p >> MOVE_BITS)
    while self.rng < TOP:
      self.rng = (self.rng << 8) & 0xFFFFFFFF
      self.shift_low()

  def finish(self):
    """The flush -> the stream's bytes (uncut, whatever their number)."""
    for _ in range(5):
      self.shift_low()
    assert self.out[0] == 0
    return bytes(self.out[1:])


class Decoder(object):
  """Bytes past the end of `data` read as 0: the caller decodes a fixed number of decisions whatever the bytes are."""

  def __init__(self, data):
    self.data, self.pos, self.rng = data, 4, 0xFFFFFFFF
    self.code = int.from_bytes((bytes(data[:4]) + b'\0\0\0\0')[:4], 'big')

  def decode(self, probs, ctx):
    p = PROB_INIT if ctx is None else probs[ctx]
    bound = (self.rng >> 11) * p
    if self.code < bound:
      self.rng = bound
      if ctx is not None:
        probs[ctx] = p + ((PROB_ONE - p) >> MOVE_BITS)
      bit = 0
    else:
      self.rng -= bound
      self.code -= bound
      if ctx is not None:
        probs[ctx] = p - (p >> MOVE_BITS)
      bit = 1
    while self.rng < TOP:
      self.rng = (self.rng << 8) & 0xFFFFFFFF
      self.code = ((self.code << 8) & 0xFFFFFFFF) | (self.data[self.pos] if self.pos < len(self.data) else 0)
      self.pos += 1
    return bit


def join_payload(streams):
  return b''.join([struct.pack('<I', len(s)) for s in streams] + list(streams))


def split_payload(payload, count):
  """The `count` streams of a payload; ValueError when the length table does not add up to the bytes that follow it."""
  if len(payload) < 4 * count:
    raise ValueError('payload of %d bytes is shorter than its table of %d lengths' % (len(payload), count))
  lens = struct.unpack('<%dI' % count, payload[:4 * count])
  if sum(lens) != len(payload) - 4 * count:
    raise ValueError('length table sums to %d, %d bytes follow it' % (sum(lens), len(payload) - 4 * count))
  out, at = [], 4 * count
  for n in lens:
    out.append(payload[at:at + n])
    at += n
  return out
