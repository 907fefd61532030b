"""Inputs of the entropy-coder tests (TEST INFRASTRUCTURE), shared by tests/test_entropy_host.py and
tests/test_hip_entropy.py: the code shapes, the input kinds, and one cached reference encoding per (shape, kind)."""
import functools

import numpy as np

import entropy_ref as eref

# (N, C, H, W): one symbol; a single row (no row above); a single column (no left / upright neighbour); the golden fixture's
# code; more than 128 channels with a ragged last wave of lanes and CPAD(C) > C; three images, W no multiple of 32 and longer
# than one 32-bit word of row bits
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 9), (1, 5, 7, 1), (2, 32, 4, 8), (1, 130, 3, 5), (3, 64, 16, 33)]
KINDS = ['half', 'sparse', 'ones', 'minus', 'blob', 'zeros']
# Seeds of the i.i.d. p = 0.5 input per shape, picked on the CPU with the reference coder's counters: the one of the largest
# shape makes the coder propagate a carry into a run of two or more pending 0xFF bytes (test_the_inputs_exercise_carry_...)
HALF_SEED = {(3, 64, 16, 33): 40}


def shape_id(s):
  return 'x'.join(str(v) for v in s)


def make_input(shape, kind):
  """float32 [N, C, H, W]: +1 / -1 (and exact zeros for 'zeros')."""
  N, C, H, W = shape
  g = np.random.default_rng([HALF_SEED.get(shape, 0), KINDS.index(kind), N, C, H, W])
  if kind == 'half':
    b = np.where(g.random(shape) < 0.5, 1.0, -1.0)
  elif kind == 'sparse':
    b = np.where(g.random(shape) < 0.02, 1.0, -1.0)
  elif kind == 'ones':
    b = np.ones(shape)
  elif kind == 'minus':
    b = -np.ones(shape)
  elif kind == 'blob':
    # 4 x 4 blocks of one sign each, with 5% of the elements flipped: spatially correlated
    coarse = g.standard_normal((N, C, (H + 3) // 4, (W + 3) // 4))
    b = np.where(np.kron(coarse, np.ones((4, 4)))[:, :, :H, :W] > 0, 1.0, -1.0)
    b = np.where(g.random(shape) < 0.05, -b, b)
  elif kind == 'zeros':
    b = np.where(g.random(shape) < 0.5, 1.0, -1.0)
    b[g.random(shape) < 0.25] = 0.0
    b.reshape(-1)[0] = 0.0
  else:
    raise ValueError(kind)
  return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
  """(b, payloads, counters): the input, the reference encoder's payload of every image, and its counters.  Computed once
  per process and never modified by a test."""
  b = make_input(shape, kind)
  b.setflags(write=False)
  counters = eref.Counters()
  return b, tuple(eref.encode(b, counters)), counters
