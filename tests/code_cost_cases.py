"""Inputs of the code-length-map tests (TEST INFRASTRUCTURE), shared by tests/test_code_cost_host.py and
tests/test_hip_code_cost.py: the code shapes, the input kinds, and one cached reference per (shape, kind)."""
import functools

import numpy as np

import code_cost_ref as ccref
import entropy_ref as eref

# (N, C, h, w): one symbol; a partial channel group and a row that crosses a 32-bit word of row bits without filling the
# second; two channel groups, the second partial, and rows of exact words; one full group, one bit into the second word
SHAPES = [(1, 1, 1, 1), (2, 5, 3, 37), (2, 70, 9, 64), (1, 64, 2, 33)]
KINDS = ['half', 'minus', 'ones', 'blob', 'zeros']


def shape_id(s):
  return 'x'.join(str(v) for v in s)


def make_input(shape, kind):
  """float32 [N, C, h, w]: +1 / -1 (and exact zeros for 'zeros')."""
  N, C, h, w = shape
  g = np.random.default_rng([KINDS.index(kind), N, C, h, w])
  if kind == 'half':
    b = np.where(g.random(shape) < 0.5, 1.0, -1.0)
  elif kind == 'minus':
    b = -np.ones(shape)
  elif kind == 'ones':
    b = np.ones(shape)
  elif kind == 'blob':
    # flat with one rectangle per (image, channel), at a place and of a size that change with the channel
    b = -np.ones(shape)
    for n in range(N):
      for c in range(C):
        y0, x0 = (n + c) % h, (3 * c + n) % w
        b[n, c, y0:y0 + 1 + (c % 4), x0:x0 + 2 + (c % 7)] = 1.0
  elif kind == 'zeros':
    b = np.where(g.random(shape) < 0.5, 1.0, -1.0)
    b[g.random(shape) < 0.25] = 0.0
    b.reshape(-1)[0] = 0.0
  else:
    raise ValueError(kind)
  return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
  """(b, costs): the input and code_cost_ref.code_cost of it.  Computed once per process and never modified by a test."""
  b = make_input(shape, kind)
  b.setflags(write=False)
  r = ccref.code_cost(b)
  for v in r.values():
    v.setflags(write=False)
  return b, r


@functools.lru_cache(maxsize=None)
def stream_bytes(shape, kind):
  """int64 [N, C]: the bytes of every stream the Python CODER (tests/entropy_ref.py) writes for the input."""
  b, _ = reference(shape, kind)
  N, C, h, w = shape
  out = np.zeros((N, C), dtype=np.int64)
  for n in range(N):
    out[n] = [len(s) for s in eref.split_payload(eref.encode_image(b[n]), C)]
  out.setflags(write=False)
  return out


def make_label(N, H, W, n_classes, seed):
  """float32 [N, 1, H, W]: patches of valid classes (the highest class included) with strays in it -- fractional, negative,
  out-of-range (n_classes itself and far beyond) and NaN labels, all of which belong to the extra row."""
  g = np.random.default_rng([seed, N, H, W, n_classes])
  coarse = g.integers(0, n_classes, size=(N, 1, (H + 3) // 4, (W + 3) // 4))
  lab = np.kron(coarse, np.ones((4, 4), dtype=np.int64))[:, :, :H, :W].astype(np.float32)
  lab.reshape(-1)[0] = n_classes - 1
  flat = lab.reshape(N, -1)
  strays = [np.float32(0.5), np.float32(-1.0), np.float32(n_classes), np.float32(1e9), np.float32(np.nan), np.float32(-0.25)]
  for n in range(N):
    at = g.choice(flat.shape[1], size=min(len(strays), flat.shape[1] - 1 if n == 0 else flat.shape[1]), replace=False)
    for i, v in zip(at, strays):
      if not (n == 0 and i == 0):
        flat[n, i] = v
  return lab
