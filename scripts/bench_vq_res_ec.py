"""Times one assign round of the entropy-constrained residual code (vq_res_ec.hip) with its statistics, for S = 2
and S = 4 stages, x in fp32 and bf16, G = 16 groups, on the two shapes of the other VQ benches (M, D, L): 1048576 x 8 against 64
centres and 262144 x 32 against 512.  The bias is the code lengths of the plain code's histograms at lambda 0.5.  Arms,
interleaved round by round in one process on the same random data:
  ec             ops.vq_res_ec_assign with the bias: index [S, M], hist and sse, no y (a round before the last)
  ec_y           the same with y (the last round)
  ec_plain       the same without a bias (round 0)
  composed       the yardstick: S rounds of ops.vq_ec_assign on a torch-subtracted residual (x widened to fp32 once) with the
                 torch gather of the chosen centres -- the same indices and counts, S - 1 more reads and writes of [M, D]
  rows           ops.vq_res_rows_fwd alone: index and y, no bias, no statistics -- the price of both is ec_y - rows
  copy           ops.copy_ moving as many bytes in all (half read, half written) as x holds
Prints one JSON line per (shape, S, dtype): the median and the minimum of each arm in microseconds.

Run:  python scripts/bench_vq_res_ec.py [--rounds 20] [--warmup 3]
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
GROUPS = 16


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
  G = GROUPS
  for M, D, L in SHAPES:
    for S in STAGES:
      books = torch.stack([(torch.rand(L, D, generator=g, device=dev) * 2 - 1) * 0.5 ** s for s in range(S)]).contiguous()
      for tdtype in (torch.float32, torch.bfloat16):
        es = 2 if tdtype == torch.bfloat16 else 4
        x = torch.randn(M, D, generator=g, device=dev).to(tdtype)
        half = (M * D * es // 2 + 15) // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        _, _, hist0, _ = ops.vq_res_ec_assign(x, books, None, G, want_y=False)
        bias = ops.vq_ec_lengths(hist0.view(S * G, L), 0.5)[0].view(S, G, L).contiguous()
        stage_bias = [bias[s].contiguous() for s in range(S)]
        stage_book = [books[s].contiguous() for s in range(S)]

        def composed():
          r, ks, hs, es_ = x.float(), [], [], []
          for s in range(S):
            k, h, e = ops.vq_ec_assign(r, stage_book[s], stage_bias[s], G)
            ks.append(k), hs.append(h), es_.append(e)
            if s + 1 < S:
              r = r - stage_book[s][k.long()]
          return torch.stack(ks), torch.stack(hs), torch.stack(es_)

        kc, hc, ec = composed()                      # the two ways agree before they are timed
        _, index, hist, sse = ops.vq_res_ec_assign(x, books, bias, G, want_y=False)
        assert torch.equal(kc, index) and torch.equal(hc, hist)
        assert float(((sse - ec).abs() / ec).max()) <= M * 2.0 ** -52
        arms = {'ec': lambda: ops.vq_res_ec_assign(x, books, bias, G, want_y=False),
                'ec_y': lambda: ops.vq_res_ec_assign(x, books, bias, G),
                'ec_plain': lambda: ops.vq_res_ec_assign(x, books, None, G, want_y=False),
                'composed': composed, 'rows': lambda: ops.vq_res_rows_fwd(x, books), 'copy': lambda: ops.copy_(src, dst)}
        times = {k: [] for k in arms}
        for r in range(a.warmup + a.rounds):
          for k, fn in arms.items():
            t = once(fn)
            if r >= a.warmup:
              times[k].append(t)
        out = {'bench': 'vq_res_ec', 'dtype': 'bf16' if es == 2 else 'fp32', 'M': M, 'D': D, 'L': L, 'G': G, 'S': S,
               'rounds': a.rounds, 'x_bytes': M * D * es}
        for k, v in times.items():
          v = sorted(v)
          out[k + '_us_median'] = round(v[len(v) // 2], 1)
          out[k + '_us_min'] = round(v[0], 1)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
