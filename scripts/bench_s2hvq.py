"""Times the S2HVQ kernels (vq.hip) at the learned codec's bottleneck of the bench workload regrouped as
vectors: M = 4 * 1024 * 32 * 64 / 8 vectors of D = 8 components, L = 64 centres, x in fp32 and bf16.  Soft forward, soft
backward (dx and dC) and hard forward, each next to ops.copy_ moving the same number of bytes (read + written) as the call.
Prints one JSON line per dtype.

Run:  python scripts/bench_s2hvq.py [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import jpdse_hip  # noqa: E402
from jpdse_hip import ops  # noqa: E402

M, D, L = 4 * 1024 * 32 * 64 // 8, 8, 64
SIGMA = 10.0


def timed(fn, iters, warmup):
  """Median of `iters` event-timed calls, in microseconds."""
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b) * 1e3)
  times.sort()
  return times[len(times) // 2]


def copy_of(nbytes, dev, iters, warmup):
  """ops.copy_ that moves `nbytes` in all: half read, half written."""
  half = (nbytes // 2 + 15) // 16 * 16
  src = torch.empty(half, dtype=torch.uint8, device=dev)
  dst = torch.empty(half, dtype=torch.uint8, device=dev)
  return timed(lambda: ops.copy_(src, dst), iters, warmup)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  g = torch.Generator(device=dev).manual_seed(0)
  scale = (SIGMA * D) ** -0.5
  book = torch.randn(L, D, generator=g, device=dev) * scale
  dp = torch.randn(M, L, generator=g, device=dev)
  for tdtype in (torch.float32, torch.bfloat16):
    es = 2 if tdtype == torch.bfloat16 else 4
    x = (torch.randn(M, D, generator=g, device=dev) * scale).to(tdtype)
    p = ops.vq_soft_fwd(x, book, SIGMA)
    moved = {'soft_fwd': M * D * es + M * L * 4, 'soft_bwd': 2 * M * L * 4 + 2 * M * D * es, 'hard_fwd': M * D * es + M * 4}
    calls = {'soft_fwd': lambda: ops.vq_soft_fwd(x, book, SIGMA), 'soft_bwd': lambda: ops.vq_soft_bwd(dp, p, x, book, SIGMA),
             'hard_fwd': lambda: ops.vq_hard_fwd(x, book)}
    out = {'bench': 's2hvq', 'dtype': 'bf16' if es == 2 else 'fp32', 'M': M, 'D': D, 'L': L}
    for name in ('soft_fwd', 'soft_bwd', 'hard_fwd'):
      us = timed(calls[name], a.iters, a.warmup)
      cp = copy_of(moved[name], dev, a.iters, a.warmup)
      out[name] = {'us': round(us, 1), 'bytes': moved[name], 'copy_us': round(cp, 1), 'ratio_to_copy': round(us / cp, 2)}
    print(json.dumps(out))


if __name__ == '__main__':
  main()
