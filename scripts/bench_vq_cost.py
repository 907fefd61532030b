"""Times the two cost walks of the S2HVQ index coders (vq_cost.hip) at the workload's code -- one 512 x 1024
image: h = 32, w = 64, G = 16 groups, L = 64, 32768 indices -- each next to the encoder whose model it prices, in the same run:
ops.vq_index_cost against ops.vq_index_encode at S = 128 (the codec's G * 8), ops.vq_plane_cost against ops.vq_plane_encode at
strip_rows 8 (S = 64).  The encode calls are host-synchronous (they end with their one copy to the host); a cost call is timed
with the copy of its cell map and group sums to the host, which is what trainer.get_vq_rate_map does with it.  One lane walks
one stream serially: latency figures, not throughput ones.  Calls alternate in blocks (walk, encoder, walk, ...); a figure is
the median over the blocks of the block's median call.

Two sources: uniform iid indices and the correlated source of the tests (a cell repeats its left neighbour with probability
0.6, else its upper one with probability 0.5, else a fresh draw).  Prints one JSON line per (source, coder) with both times,
the model's code length and the coded stream bytes.

Run:  python scripts/bench_vq_cost.py [--iters 10] [--blocks 3] [--warmup 3]
"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import jpdse_hip  # noqa: E402
from jpdse_hip import ops  # noqa: E402

H, W, G, L = 32, 64, 16, 64
M = H * W * G
INDEX_STREAMS = G * 8
STRIP_ROWS = 8


def block_median(fn, iters):
  """Median wall-clock time of `iters` host-synchronous calls, in milliseconds."""
  times = []
  for _ in range(iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  times.sort()
  return times[len(times) // 2]


def alternating(fns, iters, blocks, warmup):
  """The median over `blocks` alternating blocks of each function's block median."""
  for fn in fns:
    for _ in range(warmup):
      fn()
  per = [[] for _ in fns]
  for _ in range(blocks):
    for i, fn in enumerate(fns):
      per[i].append(block_median(fn, iters))
  return [sorted(t)[len(t) // 2] for t in per], [max(t) / min(t) - 1.0 for t in per]


def correlated(rng):
  """The correlated source of tests/vq_plane_cases.py, restated: int32 [H * W * G]."""
  v = np.zeros((H, W, G), dtype=np.int64)
  left, up, fresh = rng.random((H, W, G)) < 0.6, rng.random((H, W, G)) < 0.5, rng.integers(0, L, size=(H, W, G))
  for y in range(H):
    for x in range(W):
      cell = fresh[y, x].copy()
      if y > 0:
        cell = np.where(up[y, x], v[y - 1, x], cell)
      if x > 0:
        cell = np.where(left[y, x], v[y, x - 1], cell)
      v[y, x] = cell
  return v.reshape(-1).astype(np.int32)


def stream_bytes(payload, S):
  return sum(struct.unpack('<%dI' % S, payload[:4 * S]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--blocks', type=int, default=3)
  ap.add_argument('--warmup', type=int, default=3)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  rng = np.random.default_rng(0)
  sources = {'uniform': torch.from_numpy(rng.integers(0, L, size=M).astype(np.int32)).to(dev),
             'correlated': torch.from_numpy(correlated(rng)).to(dev)}

  def fetched(r):
    return r['cell'].cpu(), r['group'].cpu()

  for name, index in sources.items():
    common = {'bench': 'vq_cost', 'source': name, 'h': H, 'w': W, 'G': G, 'L': L, 'iters': a.iters, 'blocks': a.blocks}
    pairs = (('index', INDEX_STREAMS, lambda: fetched(ops.vq_index_cost(index, L, INDEX_STREAMS, G)),
              lambda: ops.vq_index_encode(index, L, INDEX_STREAMS)),
             ('plane', ops.vq_plane_streams(H, G, STRIP_ROWS), lambda: fetched(ops.vq_plane_cost(index, (H, W, G), L, STRIP_ROWS)),
              lambda: ops.vq_plane_encode(index, H, W, G, L, STRIP_ROWS)))
    for coder, S, walk, encode in pairs:
      cell, group = walk()
      assert int(cell.sum()) == int(group.sum())
      (walk_ms, encode_ms), (walk_spread, encode_spread) = alternating((walk, encode), a.iters, a.blocks, a.warmup)
      print(json.dumps(dict(common, coder=coder, S=S, cost_ms=round(walk_ms, 3), encode_ms=round(encode_ms, 3),
                            cost_block_spread=round(walk_spread, 3), encode_block_spread=round(encode_spread, 3),
                            model_bits=round(int(cell.sum()) / float(ops.CODE_COST_UNIT), 1),
                            stream_bytes=stream_bytes(encode(), S))), flush=True)


if __name__ == '__main__':
  main()
