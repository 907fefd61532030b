"""Times the entropy-constrained assignment (vq_ec.hip) with its histogram and distortion, x in fp32 and bf16, on
three shapes (M, D, L, G): 1048576 x 8 against 64 centres in 16 groups (the bench workload's bottleneck as vectors), 262144 x 32
against 512 centres in one group, and one 32 x 64 x 16 code (M = 32 * 64 * 16 / 8 vectors of 8, 64 centres, 2 groups).  Arms,
interleaved round by round in one process on the same random data:
  fused     ops.vq_ec_assign(bias, groups): index, per-group histogram and distortion in one read of x
  nobias    the same call without a bias
  composed  what gave an index and a per-group histogram before it: ops.vq_hard_fwd, then ops.vq_rate_fwd(hard=True,
            want_hist=True) -- two score loops, no bias, no distortion
  copy      ops.copy_ moving as many bytes in all (half read, half written) as the fused pass must read: x, once
Prints one JSON line per (shape, dtype): the median and the minimum of each arm in microseconds.

Run:  python scripts/bench_vq_ec.py [--rounds 30] [--warmup 5]
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

SHAPES = ((1048576, 8, 64, 16), (262144, 32, 512, 1), (32 * 64 * 16 // 8, 8, 64, 2))
SIGMA = 10.0


def once(fn):
  """One event-timed call, in microseconds."""
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  g = torch.Generator(device=dev).manual_seed(0)
  for M, D, L, G in SHAPES:
    scale = (SIGMA * D) ** -0.5
    book = torch.randn(L, D, generator=g, device=dev) * scale
    for tdtype in (torch.float32, torch.bfloat16):
      es = 2 if tdtype == torch.bfloat16 else 4
      x = (torch.randn(M, D, generator=g, device=dev) * scale).to(tdtype)
      half = (M * D * es // 2 + 15) // 16 * 16      # half read, half written: the bytes of x in all
      src = torch.empty(half, dtype=torch.uint8, device=dev)
      dst = torch.empty(half, dtype=torch.uint8, device=dev)
      # the bias of a real second round: the lengths of the plain code's histogram at lambda = 0.05
      index, hist, _ = ops.vq_ec_assign(x, book, None, G)
      bias, _ = ops.vq_ec_lengths(hist, 0.05)

      def composed():
        idx, _ = ops.vq_hard_fwd(x, book)
        _, h, _ = ops.vq_rate_fwd(x, book, SIGMA, G, 1.0, hard=True, want_hist=True, want_grad=False)
        return idx, h

      idx, h = composed()                            # the two ways agree before they are timed
      assert torch.equal(idx, index) and torch.equal(h.to(torch.int32), hist)
      arms = {'fused': lambda: ops.vq_ec_assign(x, book, bias, G), 'nobias': lambda: ops.vq_ec_assign(x, book, None, G),
              'composed': composed, 'copy': lambda: ops.copy_(src, dst)}
      times = {k: [] for k in arms}
      for r in range(a.warmup + a.rounds):
        for k, fn in arms.items():
          t = once(fn)
          if r >= a.warmup:
            times[k].append(t)
      out = {'bench': 'vq_ec', 'dtype': 'bf16' if es == 2 else 'fp32', 'M': M, 'D': D, 'L': L, 'G': G, 'rounds': a.rounds,
             'x_bytes': M * D * es}
      for k, v in times.items():
        v = sorted(v)
        out[k + '_us_median'] = round(v[len(v) // 2], 1)
        out[k + '_us_min'] = round(v[0], 1)
      print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
