"""The cases of the coded index stream that the host and the GPU tests share (TEST INFRASTRUCTURE): the
(M, L, S) shapes, the input kinds, and the reference coder's payload of each, computed once.

  (1, 2, 1)          one symbol
  (65, 2, 64)        lane 0 has two symbols, the others one
  (4096, 64, 64)     the bench's alphabet, one full wave
  (3000, 100, 7)     L not a power of two, a partly filled wave, uneven counts
  (4096, 257, 130)   nb = 9 with one value above 256, three waves, the last with 2 lanes
  (8192, 512, 64)    full-size tables
  (16384, 64, 4)     long streams
"""
import functools

import numpy as np

import vq_coder_ref as vref

SHAPES = [(1, 2, 1), (65, 2, 64), (4096, 64, 64), (3000, 100, 7), (4096, 257, 130), (8192, 512, 64), (16384, 64, 4)]
KINDS = ['uniform', 'geometric', 'zeros', 'top', 'ramp']
# Picked on the CPU: the first of the seeds 0, 1, ... whose uniform inputs, over the seven shapes, make the reference coder
# propagate a carry through a pending run of two 0xFF bytes (seed 9 of 10 tried: 11019 carries, longest pending run 2, one
# carry into it); test_the_inputs_exercise_carry_propagation asserts the counters
SEED = 9


def shape_id(shape):
  return 'M%d-L%d-S%d' % tuple(shape)


def indices(shape, kind, seed=None):
  """int32 numpy [M] in [0, L)."""
  M, L, S = shape
  rng = np.random.default_rng([SEED if seed is None else seed, M, L, S, KINDS.index(kind)])
  if kind == 'uniform':
    v = rng.integers(0, L, size=M)
  elif kind == 'geometric':                    # p_k proportional to 0.7^k
    p = 0.7 ** np.arange(L)
    v = rng.choice(L, size=M, p=p / p.sum())
  elif kind == 'zeros':
    v = np.zeros(M)
  elif kind == 'top':
    v = np.full(M, L - 1)
  else:
    v = np.arange(M) % L
  return v.astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
  """(indices, the reference coder's payload, its carry counters); shared, never modified."""
  v = indices(shape, kind)
  v.setflags(write=False)
  counters = vref.Counters()
  return v, vref.encode(v.tolist(), shape[1], shape[2], counters), counters


def entropy_bits(v, L):
  """Zero-order empirical entropy of the indices, in bits for the whole sequence."""
  n = np.bincount(np.asarray(v), minlength=L).astype(np.float64)
  p = n[n > 0] / n.sum()
  return float(-(n[n > 0] * np.log2(p)).sum())
