"""Times one Lloyd accumulate pass of the code-book fit (vq_fit.hip) at the two ends of the quantizer's range:
M = 1048576 vectors of D = 8 against L = 64 centres (the bench workload's bottleneck regrouped as vectors) and M = 262144 of
D = 32 against L = 512, x in fp32 and bf16.  Three arms, interleaved round by round in one process on the same random data:
  fused     ops.vq_lloyd_accum: counts, sums, distortion and reseed candidates in one pass, the index never stored
  composed  the same sums and counts from the calls that existed before it: ops.vq_hard_fwd, then ops.vq_decode_bwd(index, x, L),
            then torch.bincount(index) -- no distortion, no reseed candidate
  copy      ops.copy_ moving as many bytes in all (half read, half written) as the fused pass must read: x, once
Prints one JSON line per (shape, dtype): the median and the minimum of each arm in microseconds.

Run:  python scripts/bench_vq_fit.py [--rounds 30] [--warmup 5]
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

SHAPES = ((1048576, 8, 64), (262144, 32, 512))
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
  for M, D, L in SHAPES:
    scale = (SIGMA * D) ** -0.5
    book = torch.randn(L, D, generator=g, device=dev) * scale
    for tdtype in (torch.float32, torch.bfloat16):
      es = 2 if tdtype == torch.bfloat16 else 4
      x = (torch.randn(M, D, generator=g, device=dev) * scale).to(tdtype)
      state = ops.vq_lloyd_state(L, D, dev)
      half = (M * D * es // 2 + 15) // 16 * 16      # half read, half written: the bytes of x in all
      src = torch.empty(half, dtype=torch.uint8, device=dev)
      dst = torch.empty(half, dtype=torch.uint8, device=dev)

      def composed():
        index, _ = ops.vq_hard_fwd(x, book)
        sums, _ = ops.vq_decode_bwd(index, x, L)
        return sums, torch.bincount(index, minlength=L)

      arms = {'fused': lambda: ops.vq_lloyd_accum(x, book, state, True), 'composed': composed,
              'copy': lambda: ops.copy_(src, dst)}
      # the two ways agree before they are timed
      sums, counts = composed()
      ops.vq_lloyd_accum(x, book, state, True)
      assert torch.equal(counts, state['counts'])
      assert float((sums.double() - state['sums']).abs().max()) <= 1e-3 * float(state['sums'].abs().max())
      times = {k: [] for k in arms}
      for r in range(a.warmup + a.rounds):
        for k, fn in arms.items():
          t = once(fn)
          if r >= a.warmup:
            times[k].append(t)
      out = {'bench': 'vq_fit', 'dtype': 'bf16' if es == 2 else 'fp32', 'M': M, 'D': D, 'L': L, 'rounds': a.rounds,
             'x_bytes': M * D * es}
      for k, v in times.items():
        v.sort()
        out[k] = {'median_us': round(v[len(v) // 2], 1), 'min_us': round(v[0], 1)}
      out['fused_over_composed'] = round(out['fused']['median_us'] / out['composed']['median_us'], 3)
      print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
