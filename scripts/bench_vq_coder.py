"""Times the coded index stream of the vector quantizer (vq_coder.hip) at the bench shape of 4.13:
M = 1048576 indices of L = 64, in S = 64, 512 and 4096 streams, for a skewed (p_k ~ 0.7^k) and a uniform source.
ops.vq_index_encode and ops.vq_index_decode are host-synchronous (the encode ends with its one copy to the host, the decode
starts with the copy to the device and ends with the read of its status word), so the figures are wall-clock medians of whole
calls.  One lane codes one stream serially: a latency figure, not a throughput one.  Next to each time: the coded bytes, the
packed size (M * nb / 8) and the zero-order empirical entropy of the same indices.  Prints one JSON line per (source, S).

Run:  python scripts/bench_vq_coder.py [--iters 10] [--warmup 2]
"""
import argparse
import json
import os
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

M, L = 4 * 1024 * 32 * 64 // 8, 64
STREAMS = (64, 512, 4096)


def timed(fn, iters, warmup):
  """Median wall-clock time of `iters` host-synchronous calls, in milliseconds."""
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  times.sort()
  return times[len(times) // 2]


def entropy_bytes(v):
  n = np.bincount(v, minlength=L).astype(np.float64)
  n = n[n > 0]
  return float(-(n * np.log2(n / n.sum())).sum() / 8)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  rng = np.random.default_rng(0)
  p = 0.7 ** np.arange(L)
  sources = {'geometric': rng.choice(L, size=M, p=p / p.sum()).astype(np.int32), 'uniform': rng.integers(0, L, size=M).astype(np.int32)}
  for name, v in sources.items():
    index = torch.from_numpy(v).to(dev)
    for S in STREAMS:
      payload = ops.vq_index_encode(index, L, S)
      assert torch.equal(ops.vq_index_decode(payload, M, L, S, dev), index)
      enc = timed(lambda: ops.vq_index_encode(index, L, S), a.iters, a.warmup)
      dec = timed(lambda: ops.vq_index_decode(payload, M, L, S, dev), a.iters, a.warmup)
      print(json.dumps({'bench': 'vq_coder', 'source': name, 'M': M, 'L': L, 'S': S, 'encode_ms': round(enc, 3),
                        'decode_ms': round(dec, 3), 'coded_bytes': len(payload), 'packed_bytes': M * ops.vq_index_bits(L) // 8,
                        'entropy_bytes': round(entropy_bytes(v), 1),
                        'coded_over_entropy': round(len(payload) / entropy_bytes(v), 4)}), flush=True)


if __name__ == '__main__':
  main()
