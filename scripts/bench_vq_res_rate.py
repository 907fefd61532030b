"""Times the rate term of the residual quantizer (vq_res_rate.hip, vq_residual.hip) for S = 2 and S = 4 stages, x in
fp32 and bf16, G = 16 groups, on the two shapes of the other VQ benches (M, D, L): 1048576 x 8 against 64 centres and 262144 x 32
against 512.  sigma = 1 / D.  Arms, interleaved round by round in one process on the same random data:
  rate           ops.vq_res_rate_fwd: rate, rates and dhist, no code
  rate_code      the same with want_code: y and index from the same kernel (the training forward)
  rows           ops.vq_res_rows_fwd alone: y and index -- the price of the rate term in a training forward is rate_code - rows
  bwd_grouped    ops.vq_res_bwd(groups=G, dhist=...): dx and dbooks with the rate term's share of dp
  bwd            ops.vq_res_bwd: the same call without it
  copy           ops.copy_ moving as many bytes in all (half read, half written) as x holds
Prints one JSON line per (shape, S, dtype): the median and the minimum of each arm in microseconds.  Then one train step of the
small s2hvq trainer of tests/test_hip_vq_res_rate_step.py (nef 8, 64 x 32 images, batch 2, vq_stages 3, bf16) with and without
opt.lambda_vq_stage_rate, timed as scripts/bench_vq_rate.py times its step: one JSON line.

Run:  python scripts/bench_vq_res_rate.py [--rounds 20] [--warmup 3] [--step_iters 30]
"""
import argparse
import contextlib
import json
import os
import sys
import time

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


def step_times(iters, warmup):
  """Median wall time of one train step (synchronised) of the small residual s2hvq trainer, with and without the rate term, in us."""
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt, synthetic_batch
  out = {}
  xd = synthetic_batch(2, 64, 32, seed=3)
  for name, lam in (('step_us', 0.0), ('step_rate_us', 0.5)):
    opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype='bf16', ngf=8, ndf=8, n_blocks_global=1,
                      n_downsample_global=2, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8,
                      n_downsample_E=2, encoder_binarizer_out_channels=16, encoder_quantizer='s2hvq', vq_n_center=8,
                      vq_center_size=4, vq_sigma=10.0, no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True,
                      no_d_gan_loss=True, skip_unused_losses=True, vq_stages=3, lambda_vq_stage_rate=lam)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
      tr = get_trainer(opt)(opt, 'train')
    for _ in range(warmup):
      tr.step(xd)
    times = []
    for _ in range(iters):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      tr.step(xd)
      torch.cuda.synchronize()
      times.append((time.perf_counter() - t0) * 1e6)
    times.sort()
    out[name] = round(times[len(times) // 2], 1)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--step_iters', type=int, default=30)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  g = torch.Generator(device=dev).manual_seed(0)
  G = GROUPS
  for M, D, L in SHAPES:
    sigma = 1.0 / D
    for S in STAGES:
      books = torch.stack([(torch.rand(L, D, generator=g, device=dev) * 2 - 1) * 0.5 ** s for s in range(S)]).contiguous()
      for tdtype in (torch.float32, torch.bfloat16):
        es = 2 if tdtype == torch.bfloat16 else 4
        x = torch.randn(M, D, generator=g, device=dev).to(tdtype)
        dy = torch.randn(M, D, generator=g, device=dev).to(tdtype)
        half = (M * D * es // 2 + 15) // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        _, _, _, dhist, y, index = ops.vq_res_rate_fwd(x, books, sigma, G, float(M), 0.5, want_code=True)
        y0, index0 = ops.vq_res_rows_fwd(x, books)
        assert torch.equal(y, y0) and torch.equal(index, index0)          # the two forwards agree before they are timed
        arms = {'rate': lambda: ops.vq_res_rate_fwd(x, books, sigma, G, float(M), 0.5),
                'rate_code': lambda: ops.vq_res_rate_fwd(x, books, sigma, G, float(M), 0.5, want_code=True),
                'rows': lambda: ops.vq_res_rows_fwd(x, books),
                'bwd_grouped': lambda: ops.vq_res_bwd(dy, x, books, index, sigma, groups=G, dhist=dhist),
                'bwd': lambda: ops.vq_res_bwd(dy, x, books, index, sigma),
                'copy': lambda: ops.copy_(src, dst)}
        times = {k: [] for k in arms}
        for r in range(a.warmup + a.rounds):
          for k, fn in arms.items():
            t = once(fn)
            if r >= a.warmup:
              times[k].append(t)
        out = {'bench': 'vq_res_rate', 'dtype': 'bf16' if es == 2 else 'fp32', 'M': M, 'D': D, 'L': L, 'G': G, 'S': S,
               'rounds': a.rounds, 'x_bytes': M * D * es}
        for k, v in times.items():
          v = sorted(v)
          out[k + '_us_median'] = round(v[len(v) // 2], 1)
          out[k + '_us_min'] = round(v[0], 1)
        print(json.dumps(out), flush=True)
  out = dict(bench='vq_res_rate_step', model='nef 8, 64 x 32, batch 2, vq_stages 3, bf16')
  out.update(step_times(a.step_iters, a.warmup))
  print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
