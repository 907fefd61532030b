"""Times the rate term of the vector-quantizer bottleneck (vq_bottleneck.hip) at the bench shape of 4.13 / 4.15:
M = 1048576 vectors of D = 8 against L = 64 centres, G = 16 groups (the workload's 128 channels in vectors of 8) and G = 1, fp32
and bf16; medians of event-timed calls.  Next to each figure, from the same run:
  pmf increment   the parent's only histogram: ops.vq_quantize_fwd(hard, want_pmf=True) minus the plain hard forward;
  copy            ops.copy_ of a buffer whose read + write traffic equals the bytes ops.vq_rate_fwd must read, M D e (x; e the
                  element size), and for the backward 3 M D e as in scripts/bench_vq_bottleneck.py.
Then one train step of the small s2hvq trainer of tests/test_hip_vq_encoder.py (nef 8, 64 x 32 images, batch 2) with and
without --lambda_vq_rate.  Prints one JSON line per dtype and one for the step.

Run:  python scripts/bench_vq_rate.py [--iters 30] [--warmup 5]
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

M, D, L, SIGMA = 4 * 1024 * 32 * 64 // 8, 8, 64, 10.0
GROUPS = (16, 1)


def timed(fn, iters, warmup):
  """Median device time of `iters` calls between two events on the current stream, in microseconds."""
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


def step_times(iters, warmup):
  """Median wall time of one train step (synchronised) of the small s2hvq trainer, with and without the rate term, in us."""
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt, synthetic_batch
  out = {}
  xd = synthetic_batch(2, 64, 32, seed=3)
  for name, lam in (('step_us', 0.0), ('step_rate_us', 0.5)):
    opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype='bf16', ngf=8, ndf=8, n_blocks_global=1,
                      n_downsample_global=2, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8,
                      n_downsample_E=2, encoder_binarizer_out_channels=16, encoder_quantizer='s2hvq', vq_n_center=8,
                      vq_center_size=4, vq_sigma=10.0, lambda_vq_rate=lam, no_vgg_loss=True, no_gan_feat_loss=True,
                      no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True)
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
  ap.add_argument('--iters', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  g = torch.Generator().manual_seed(0)
  scale = (SIGMA * D) ** -0.5
  x32 = ((torch.rand(M, D, generator=g) * 2 - 1) * scale).to(dev)
  c = ((torch.rand(L, D, generator=g) * 2 - 1) * scale).to(dev)
  dy32 = torch.randn(M, D, generator=g).to(dev)
  for name, td in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
    x, dy = x32.to(td).contiguous(), dy32.to(td).contiguous()
    e = x.element_size()
    read_bytes, bwd_bytes = M * D * e, 3 * M * D * e
    t = lambda fn: round(timed(fn, a.iters, a.warmup), 1)
    src_r = torch.empty(read_bytes // 2, dtype=torch.uint8, device=dev)
    src_b = torch.empty(bwd_bytes // 2, dtype=torch.uint8, device=dev)
    dst_r, dst_b = torch.empty_like(src_r), torch.empty_like(src_b)
    out = dict(bench='vq_rate', dtype=name, M=M, D=D, L=L, read_bytes=read_bytes, bwd_bytes=bwd_bytes)
    out['fwd_hard_us'] = t(lambda: ops.vq_quantize_fwd(x, c, SIGMA, True))
    out['fwd_hard_pmf_us'] = t(lambda: ops.vq_quantize_fwd(x, c, SIGMA, True, want_pmf=True))
    out['pmf_increment_us'] = round(out['fwd_hard_pmf_us'] - out['fwd_hard_us'], 1)
    out['copy_read_us'] = t(lambda: ops.copy_(src_r, dst_r))
    out['copy_bwd_us'] = t(lambda: ops.copy_(src_b, dst_b))
    out['bwd_us'] = t(lambda: ops.vq_quantize_bwd(dy, x, c, SIGMA))
    for G in GROUPS:
      out['rate_soft_g%d_us' % G] = t(lambda: ops.vq_rate_fwd(x, c, SIGMA, G, float(M), 1.0))
      out['rate_hard_g%d_us' % G] = t(lambda: ops.vq_rate_fwd(x, c, SIGMA, G, float(M), 1.0, hard=True, want_grad=False))
      _, _, dhist = ops.vq_rate_fwd(x, c, SIGMA, G, float(M), 1.0)
      out['bwd_grouped_g%d_us' % G] = t(lambda: ops.vq_quantize_bwd(dy, x, c, SIGMA, groups=G, dhist=dhist))
      out['bwd_grouped_no_dhist_g%d_us' % G] = t(lambda: ops.vq_quantize_bwd(dy, x, c, SIGMA, groups=G))
    print(json.dumps(out), flush=True)
  out = dict(bench='vq_rate_step', model='nef 8, 64 x 32, batch 2, bf16')
  out.update(step_times(a.iters, a.warmup))
  print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
