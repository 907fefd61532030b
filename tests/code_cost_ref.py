"""Pure-Python restatement of the code-length map jpdse_code_cost writes (TEST INFRASTRUCTURE), written from the definitions
of DESIGN.md 4.12 and from nothing else.  The model half of the coder -- the 16 adaptive probabilities, their start value and
their update -- is tests/rc_ref.py's (Encoder.encode's two update lines, restated as `adapted`), the context rule and the walk
are tests/entropy_ref.py's.  Integer arithmetic throughout: the only floating-point step is the cost table, math.log2 in
float64, rounded to an integer once.

  unit      2^-16 bit
  T[v]      round(-log2(v / 2048) * 65536), v = 1 .. 2047; T[0] = T[2048] = 0
  cost      of a symbol coded with probability q of bit 0 (before the update): T[q] for bit 0, T[2048 - q] for bit 1
"""
import functools
import math

import numpy as np

from rc_ref import PROB_INIT, PROB_ONE, MOVE_BITS
from class_metrics_ref import class_index

UNIT = 1 << 16


@functools.lru_cache(maxsize=None)
def table():
  return tuple([0] + [int(round(-math.log2(v / PROB_ONE) * UNIT)) for v in range(1, PROB_ONE)] + [0])


def adapted(q, bit):
  """rc_ref.Encoder.encode's update of probs[ctx]."""
  return q - (q >> MOVE_BITS) if bit else q + ((PROB_ONE - q) >> MOVE_BITS)


def stream_costs(bits, H, W):
  """bits: H*W values of 0 / 1 in raster order -> the H*W symbol costs (Python ints), the walk of entropy_ref.encode_stream."""
  assert len(bits) == H * W
  T = table()
  probs = [PROB_INIT] * 16
  out = [0] * (H * W)
  prev = [0] * (W + 2)
  for y in range(H):
    cur = [0] * (W + 2)
    for x in range(W):
      bit = bits[y * W + x]
      ctx = cur[x] | prev[x + 1] << 1 | prev[x] << 2 | prev[x + 2] << 3
      q = probs[ctx]
      out[y * W + x] = T[PROB_ONE - q] if bit else T[q]
      probs[ctx] = adapted(q, bit)
      cur[x + 1] = bit
    prev = cur
  return out


def code_cost(b):
  """b: [N, C, H, W] of any sign (bit = b > 0) -> dict(symbol int64 [N, H, W, C], cell int64 [N, H, W], channel int64 [N, C])."""
  b = np.asarray(b)
  N, C, H, W = b.shape
  on = (b > 0).astype(np.uint8).reshape(N, C, H * W)
  symbol = np.zeros((N, H, W, C), dtype=np.int64)
  for n in range(N):
    for c in range(C):
      symbol[n, :, :, c] = np.array(stream_costs(on[n, c].tolist(), H, W), dtype=np.int64).reshape(H, W)
  return dict(symbol=symbol, cell=symbol.sum(axis=3), channel=symbol.sum(axis=(1, 2)))


def class_tables(cell, label, n_classes):
  """cell: int64 [N, h, w]; label: float [N, 1, H, W] or [N, H, W] with H = s h, W = s w.  -> (units, pixels), int64
  [N, n_classes + 1]: units[n, k] = the sum over the pixels of image n with class k of the (undivided) units of the cell that
  covers the pixel, cell[n, y // s, x // s]; the class of a pixel is class_metrics_ref.class_index's, row n_classes for a pixel
  without one.  Integer adds (np.add.at), no float weights."""
  cell = np.asarray(cell, dtype=np.int64)
  N, h, w = cell.shape
  label = np.asarray(label)
  H, W = label.shape[-2:]
  s = H // h
  assert label.size == N * H * W and s * h == H and s * w == W, (label.shape, cell.shape)
  idx = class_index(label, n_classes).reshape(N, H * W)
  spread = np.repeat(np.repeat(cell, s, axis=1), s, axis=2).reshape(N, H * W)
  units = np.zeros((N, n_classes + 1), dtype=np.int64)
  pixels = np.zeros((N, n_classes + 1), dtype=np.int64)
  for n in range(N):
    np.add.at(units[n], idx[n], spread[n])
    np.add.at(pixels[n], idx[n], 1)
  return units, pixels


def bound_bits(h, w):
  """|8 * stream bytes - stream units / 65536| <= 48 + h * w / 64."""
  return 48.0 + h * w / 64.0
