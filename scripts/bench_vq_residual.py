"""Times the residual quantizer's fused kernels (vq_residual.hip) for S = 2 and S = 4 stages, x in fp32 and bf16,
on the two shapes of the other VQ benches (M, D, L): 1048576 x 8 against 64 centres and 262144 x 32 against 512.  Arms, interleaved
round by round in one process on the same random data:
  fwd            ops.vq_res_fwd: index [S, M] and y in one read of x (the group layout, the residual in LDS)
  fwd_rows       ops.vq_res_rows_fwd: the same bits from one thread per vector, the residual in registers
  fwd_composed   the yardstick: S rounds of ops.vq_quantize_fwd(hard) on a torch-subtracted residual (x widened to fp32 once), the
                 centres summed by torch -- the same indices, S score loops, S - 1 more reads and writes of [M, D] and the launches
  bwd            ops.vq_res_bwd: dx and dbooks
  bwd_composed   S rounds of ops.vq_quantize_bwd at the residuals, stages descending, with the torch additions and subtractions
                 of the recursion (the residuals rebuilt by torch from the indices first: the composed form saves what the fused
                 one saves, x and the indices)
  copy           ops.copy_ moving as many bytes in all (half read, half written) as x holds
Prints one JSON line per (shape, S, dtype): the median and the minimum of each arm in microseconds.

Run:  python scripts/bench_vq_residual.py [--rounds 20] [--warmup 3]
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
STAGES = (2, 4)


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
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  g = torch.Generator(device=dev).manual_seed(0)
  for M, D, L in SHAPES:
    sigma = 1.0 / D
    for S in STAGES:
      books = torch.rand(S, L, D, generator=g, device=dev) * 2 - 1
      for tdtype in (torch.float32, torch.bfloat16):
        es = 2 if tdtype == torch.bfloat16 else 4
        x = torch.randn(M, D, generator=g, device=dev).to(tdtype)
        dy = torch.randn(M, D, generator=g, device=dev).to(tdtype)
        half = (M * D * es // 2 + 15) // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        y, index, _, _ = ops.vq_res_fwd(x, books)

        def fwd_composed():
          r, ysum, ks = x.float(), None, []
          for s in range(S):
            c, k, _ = ops.vq_quantize_fwd(r, books[s], sigma, hard_forward=True)
            ks.append(k)
            ysum = c if ysum is None else ysum + c
            r = r - c
          return ysum.to(tdtype), torch.stack(ks)

        def bwd_composed():
          rs = [x.float()]
          for s in range(S - 1):
            rs.append(rs[-1] - books[s][index[s].long()])
          h, dc = torch.zeros_like(rs[0]), torch.empty_like(books)
          dyf = dy.float()
          for s in range(S - 1, -1, -1):
            u, _ = ops.vq_quantize_bwd((dyf - h).contiguous(), rs[s], books[s], sigma, dc_out=dc[s])
            h = h + u
          return h.to(tdtype), dc

        yc, kc = fwd_composed()                      # the two ways agree before they are timed
        assert torch.equal(kc, index) and torch.equal(yc, y)
        yr, kr = ops.vq_res_rows_fwd(x, books)
        assert torch.equal(kr, index) and torch.equal(yr, y)
        dx, dc = ops.vq_res_bwd(dy, x, books, index, sigma)
        dxc, dcc = bwd_composed()
        assert float((dx.float() - dxc.float()).abs().max()) <= 2e-2 * float(dxc.float().abs().max())
        assert float((dc - dcc).abs().max()) <= 1e-3 * float(dcc.abs().max())
        arms = {'fwd': lambda: ops.vq_res_fwd(x, books), 'fwd_rows': lambda: ops.vq_res_rows_fwd(x, books),
                'fwd_composed': fwd_composed,
                'bwd': lambda: ops.vq_res_bwd(dy, x, books, index, sigma), 'bwd_composed': bwd_composed,
                'copy': lambda: ops.copy_(src, dst)}
        times = {k: [] for k in arms}
        for r in range(a.warmup + a.rounds):
          for k, fn in arms.items():
            t = once(fn)
            if r >= a.warmup:
              times[k].append(t)
        out = {'bench': 'vq_residual', 'dtype': 'bf16' if es == 2 else 'fp32', 'M': M, 'D': D, 'L': L, 'S': S, 'rounds': a.rounds,
               'x_bytes': M * D * es}
        for k, v in times.items():
          v = sorted(v)
          out[k + '_us_median'] = round(v[len(v) // 2], 1)
          out[k + '_us_min'] = round(v[0], 1)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
