"""The cases of the context-coded index planes that the host and the GPU tests share (TEST INFRASTRUCTURE):
the (h, w, G, L, strip_rows) shapes, the sources, and the reference coder's payload of each, computed once.

  (1, 1, 1, 2, 1)       one symbol, no neighbour
  (1, 65, 1, 2, 1)      one row, never an upper cell
  (3, 1, 2, 64, 2)      one column, never a left cell; short last strip
  (8, 16, 16, 64, 4)    32 streams, half a wave
  (16, 8, 5, 100, 3)    L not a power of two, uneven last strip, 30 streams
  (12, 4, 16, 257, 2)   nb = 9, 96 streams
  (4, 8, 8, 512, 4)     full tables
  (64, 32, 1, 64, 64)   one long stream of 2048 symbols
"""
import functools

import numpy as np

import vq_plane_ref as pref

SHAPES = [(1, 1, 1, 2, 1), (1, 65, 1, 2, 1), (3, 1, 2, 64, 2), (8, 16, 16, 64, 4), (16, 8, 5, 100, 3), (12, 4, 16, 257, 2),
          (4, 8, 8, 512, 4), (64, 32, 1, 64, 64)]
KINDS = ['uniform', 'zeros', 'top', 'ramp', 'stripes', 'correlated']
# Picked on the CPU: the first of the seeds 0, 1, ... whose uniform and correlated inputs, over the eight shapes, make the
# reference coder propagate a carry through a pending run of two 0xFF bytes (seed 27 of 28 tried: 2400 carries, longest pending
# run 2, one carry into it); test_the_inputs_exercise_carry_propagation asserts the counters
SEED = 27
CARRY_KINDS = ('uniform', 'correlated')
# the shape of the size conditions and of the bench: the workload's code, and the order-0 coder's stream count next to it
WORKLOAD = (32, 64, 16, 64, 8)
ORDER0_STREAMS = 64


def shape_id(shape):
  return 'h%d-w%d-G%d-L%d-r%d' % tuple(shape)


def correlated(rng, h, w, G, L):
  """In raster order per group: a cell equals its left neighbour with probability 0.6, else its upper neighbour with
  probability 0.5 where one exists, else it is a fresh uniform draw.  int64 [h, w, G]."""
  v = np.zeros((h, w, G), dtype=np.int64)
  left, up, fresh = rng.random((h, w, G)) < 0.6, rng.random((h, w, G)) < 0.5, rng.integers(0, L, size=(h, w, G))
  for y in range(h):
    for x in range(w):
      cell = fresh[y, x].copy()
      if y > 0:
        cell = np.where(up[y, x], v[y - 1, x], cell)
      if x > 0:
        cell = np.where(left[y, x], v[y, x - 1], cell)
      v[y, x] = cell
  return v


def indices(shape, kind, seed=None):
  """int32 numpy [h * w * G] in [0, L), cell (y, x, g) at (y * w + x) * G + g."""
  h, w, G, L, strip_rows = shape
  rng = np.random.default_rng([SEED if seed is None else seed, h, w, G, L, strip_rows, KINDS.index(kind)])
  y, x, g = np.meshgrid(np.arange(h), np.arange(w), np.arange(G), indexing='ij')
  if kind == 'uniform':
    v = rng.integers(0, L, size=(h, w, G))
  elif kind == 'zeros':
    v = np.zeros((h, w, G))
  elif kind == 'top':
    v = np.full((h, w, G), L - 1)
  elif kind == 'ramp':
    v = (y * w + x + g) % L
  elif kind == 'stripes':                      # always equal to the upper cell, never to the left one
    v = x % L
  else:
    v = correlated(rng, h, w, G, L)
  return np.ascontiguousarray(v).reshape(-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
  """(indices, the reference coder's payload, its carry counters); shared, never modified."""
  v = indices(shape, kind)
  v.setflags(write=False)
  counters = pref.Counters()
  return v, pref.encode(v.tolist(), *shape, counters=counters), counters


def carry_counters(seed=None):
  """The reference's counters over the uniform and the correlated inputs of all shapes."""
  total = pref.Counters()
  for shape in SHAPES:
    for kind in CARRY_KINDS:
      if seed is None:
        total.add(reference(shape, kind)[2])
      else:
        c = pref.Counters()
        pref.encode(indices(shape, kind, seed).tolist(), *shape, counters=c)
        total.add(c)
  return total
