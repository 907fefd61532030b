"""Inputs of the coded-semantics tests (TEST INFRASTRUCTURE), shared by tests/test_semantics_host.py and
tests/test_hip_semantics.py: the shapes, the input kinds, and one cached reference encoding per (shape, kind)."""
import functools
import os

import numpy as np

import semantics_ref as sref

# (N, H, W, strip_rows): one pixel; one row (no row above); one column (no left neighbour); two full strips; a short last
# strip; 70 strips of one row (a second wave whose lanes 6..63 are past the end); W beyond eight 16-pixel chunks with a ragged
# last one and H no multiple of strip_rows; one strip as tall as the image
SHAPES = [(1, 1, 1, 8), (1, 1, 37, 8), (1, 37, 1, 8), (2, 16, 33, 8), (3, 19, 33, 8), (1, 70, 20, 1), (1, 9, 130, 4),
          (1, 24, 40, 24)]
KINDS = ['const', 'vstripes', 'hstripes', 'checker', 'rects', 'iid19', 'extremes']
INST_VALUES = np.array([0, 33999, (1 << 31) - 1, 26001, 26002, 7], dtype=np.int64)
# The carry input, picked on the CPU with the reference coder's counters: no stream of it is cut, so the device comparison
# covers every byte, the carry through two pending 0xFF bytes included (seed 18 of 19 tried: 1111 carries, longest run 2)
CARRY_SHAPE, CARRY_KIND = (3, 19, 33, 8), 'extremes'
SEED = {(CARRY_SHAPE, CARRY_KIND): 18}
# i.i.d. labels cost a literal per pixel on top of two decisions: more than the raw byte, so streams outgrow their slots
CUT_SHAPE, CUT_KIND = (2, 16, 33, 8), 'iid19'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'semantics_cityscapes.npz')


def shape_id(s):
  return 'x'.join(str(v) for v in s)


def make_input(shape, kind, seed=None):
  """(label uint8 [N, H, W], instance int64 [N, H, W])."""
  N, H, W, _ = shape
  g = np.random.default_rng([SEED.get((shape, kind), 0) if seed is None else seed, KINDS.index(kind), N, H, W])
  y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  if kind == 'const':
    label = np.full((N, H, W), 7)
    inst = np.full((N, H, W), 26001)
  elif kind == 'vstripes':
    label = np.broadcast_to((x // 3) % 5, (N, H, W))
    inst = np.broadcast_to(1000 * ((x // 3) % 5) + x // 3, (N, H, W))
  elif kind == 'hstripes':
    label = np.broadcast_to((y // 2) % 4 + 10, (N, H, W))
    inst = np.broadcast_to(24000 + y // 2, (N, H, W))
  elif kind == 'checker':
    label = np.broadcast_to((x + y) % 2 * 11, (N, H, W))
    inst = np.broadcast_to((x + y) % 2 * 33999, (N, H, W))
  elif kind == 'rects':
    label = np.zeros((N, H, W), dtype=np.int64)
    inst = np.zeros((N, H, W), dtype=np.int64)
    for n in range(N):
      for k in range(6):
        y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
        y1, x1 = y0 + 1 + int(g.integers(0, H)), x0 + 1 + int(g.integers(0, W))
        label[n, y0:y1, x0:x1] = g.integers(0, 19)
        inst[n, y0:y1, x0:x1] = 1000 * int(g.integers(24, 34)) + k
    noise = g.random((N, H, W)) < 0.02
    label = np.where(noise, g.integers(0, 19, (N, H, W)), label)
    inst = np.where(noise, INST_VALUES[g.integers(0, len(INST_VALUES), (N, H, W))], inst)
  elif kind == 'iid19':
    label = g.integers(0, 19, (N, H, W))
    inst = g.integers(0, 1 << 31, (N, H, W))
  elif kind == 'extremes':
    label = np.where(g.random((N, H, W)) < 0.5, 0, 255)
    inst = INST_VALUES[g.integers(0, 3, (N, H, W))]
  else:
    raise ValueError(kind)
  return np.ascontiguousarray(label).astype(np.uint8), np.ascontiguousarray(inst).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, seed=None):
  """(label, inst, coded, counters): the inputs, coded[n][plane] = (payload, cut) of the reference encoder (a cut payload
  is clipped to the slots, as the device leaves it), and the coder's counters.  Computed once per process, never modified."""
  label, inst = make_input(shape, kind, seed)
  label.setflags(write=False)
  inst.setflags(write=False)
  counters = sref.Counters()
  coded = tuple((sref.encode_plane(label[n], 0, shape[3], counters), sref.encode_plane(inst[n], 1, shape[3], counters))
                for n in range(shape[0]))
  return label, inst, coded, counters


@functools.lru_cache(maxsize=None)
def golden():
  """(label uint8 [512, 1024], instance int64) of the recorded Cityscapes pair, and coded[plane] = (payload, cut) at the
  default strip_rows of 8."""
  d = np.load(GOLDEN)
  label, inst = d['label'], d['instance'].astype(np.int64)
  label.setflags(write=False)
  inst.setflags(write=False)
  return label, inst, (sref.encode_plane(label, 0, 8), sref.encode_plane(inst, 1, 8))
