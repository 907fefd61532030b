"""Times the residual quantizer with a stage depth per cell (vq_residual.hip, the DEP instantiations) for S = 2 and
S = 4 stages, x in fp32 and bf16, G = 16 vectors per cell, on the two shapes of the other VQ benches (M, D, L): 1048576 x 8 against
64 centres and 262144 x 32 against 512.  sigma = 1 / D.  Depth maps: `uniform` (S everywhere), `halves` (whole 256-vector tiles
alternately at 1 and at S, in blocks of 64 tiles), `random` (per cell, uniform over 1 .. S).  Arms, interleaved round by round in
one process on the same random data:
  fwd_depth      ops.vq_res_rows_fwd(depth=, groups=G): y and index
  fwd_plain      ops.vq_res_rows_fwd at uniform S: what the `uniform` map is read against -- the difference is the predicate's price
  fwd_composed   what a user would write without the kernel: per depth value gather the rows, ops.vq_res_rows_fwd with that
                 n_stages, scatter y and index back
  bwd_depth, bwd_plain, bwd_composed   the same three for ops.vq_res_bwd (dx and dbooks; composed: dbooks summed over the calls)
Prints one JSON line per (shape, S, dtype, map): the median and the minimum of each arm in microseconds.  Then the coded sizes of
one 32 x 64 x 16 code (S = 4, 64 centres) under the three maps, as ctu.utils.vqdepth writes it, next to the .jpdr file of the
uniform code: one JSON line.

Run:  python scripts/bench_vq_depth.py [--rounds 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
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
MAPS = ('uniform', 'halves', 'random')


def once(fn):
  """One event-timed call, in microseconds."""
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e3


def depth_map(kind, cells, S, G, seed=0):
  if kind == 'uniform':
    return np.full(cells, S, dtype=np.int32)
  if kind == 'halves':
    tile = np.arange(cells) * G // 256
    return np.where((tile // 64) % 2 == 0, 1, S).astype(np.int32)
  return np.random.RandomState(seed).randint(1, S + 1, size=cells).astype(np.int32)


def composed_fwd(x, books, nm_rows, S):
  y = torch.empty_like(x)
  index = torch.full((S, x.shape[0]), -1, dtype=torch.int32, device=x.device)
  for v, rows in nm_rows:
    yv, iv = ops.vq_res_rows_fwd(x.index_select(0, rows), books, v)
    y.index_copy_(0, rows, yv)
    index[:v].index_copy_(1, rows, iv)
  return y, index


def composed_bwd(dy, x, books, index, sigma, nm_rows):
  dx = torch.empty_like(x)
  dc = torch.zeros_like(books)
  for v, rows in nm_rows:
    dxv, dcv = ops.vq_res_bwd(dy.index_select(0, rows), x.index_select(0, rows), books, index[:v].index_select(1, rows).contiguous(), sigma)
    dx.index_copy_(0, rows, dxv)
    dc += dcv
  return dx, dc


def coded_sizes():
  from ctu.quantizers import ResidualS2HVQ
  from ctu.utils import vqdepth, vqstages
  S, L, D, G, h, w = 4, 64, 8, 16, 32, 64
  g = torch.Generator().manual_seed(5)
  books = torch.stack([(torch.rand(L, D, generator=g) * 2 - 1) * 0.5 ** s for s in range(S)]).cuda()
  x = torch.randn(h * w, G * D, generator=g).cuda()
  rvq = ResidualS2HVQ(books).cuda().eval()
  out = {'jpdr_uniform_bytes': len(vqstages.write_stages(None, rvq.encode(x, G), L))}
  for kind in MAPS:
    d = depth_map(kind, h * w, S, G, seed=7)
    if kind == 'halves':
      d = np.where(np.arange(h * w) < h * w // 2, 1, S).astype(np.int32)          # the upper half of the image at 1, the lower at S
    code = rvq.encode(x, G, depth=torch.from_numpy(d).cuda(), groups=G)
    blob = vqdepth.write_depth_stages(None, code, d, L, groups=G)
    out['jpdm_%s_bytes' % kind] = len(blob)
    out['jpdm_%s_indices' % kind] = int(d.sum()) * G
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  args = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  for M, D, L in SHAPES:
    for S in STAGES:
      for tdtype in (torch.float32, torch.bfloat16):
        g = torch.Generator().manual_seed(M + S)
        x = torch.randn(M, D, generator=g).to(tdtype).to(dev)
        dy = torch.randn(M, D, generator=g).to(tdtype).to(dev)
        books = torch.stack([(torch.rand(L, D, generator=g) * 2 - 1) * 0.5 ** s for s in range(S)]).to(dev)
        sigma = 1.0 / D
        _, plain_index = ops.vq_res_rows_fwd(x, books, S)
        for kind in MAPS:
          d = depth_map(kind, M // GROUPS, S, GROUPS, seed=S)
          dd = torch.from_numpy(d).to(dev)
          nm = dd.long().repeat_interleave(GROUPS)
          nm_rows = [(v, torch.nonzero(nm == v).view(-1)) for v in sorted(set(d.tolist()))]
          _, index = ops.vq_res_rows_fwd(x, books, S, depth=dd, groups=GROUPS)
          arms = {
              'fwd_depth': lambda: ops.vq_res_rows_fwd(x, books, S, depth=dd, groups=GROUPS),
              'fwd_plain': lambda: ops.vq_res_rows_fwd(x, books, S),
              'fwd_composed': lambda: composed_fwd(x, books, nm_rows, S),
              'bwd_depth': lambda: ops.vq_res_bwd(dy, x, books, index, sigma, groups=GROUPS, depth=dd),
              'bwd_plain': lambda: ops.vq_res_bwd(dy, x, books, plain_index, sigma),
              'bwd_composed': lambda: composed_bwd(dy, x, books, index, sigma, nm_rows),
          }
          times = {k: [] for k in arms}
          for r in range(args.warmup + args.rounds):
            for k, fn in arms.items():
              t = once(fn)
              if r >= args.warmup:
                times[k].append(t)
          row = dict(M=M, D=D, L=L, S=S, dtype=str(tdtype).split('.')[-1], map=kind, mean_depth=round(float(d.mean()), 3))
          for k, v in times.items():
            v.sort()
            row[k + '_us'] = round(v[len(v) // 2], 1)
            row[k + '_min_us'] = round(v[0], 1)
          print(json.dumps(row), flush=True)
  print(json.dumps(dict(coded_sizes=coded_sizes())), flush=True)


if __name__ == '__main__':
  main()
