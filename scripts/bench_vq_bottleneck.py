"""Times the fused vector-quantizer bottleneck (vq_bottleneck.hip) at the bench shape of 4.13: M = 1048576
vectors of D = 8 against L = 64 centres, fp32 and bf16; medians of event-timed calls.  Next to each figure its two yardsticks:
  copy      ops.copy_ of a buffer whose read + write traffic equals the bytes the fused call must move -- forward
            M (2 D e + 4) (x in, y and the index out), backward 3 M D e (dy and x in, dx out), e the element size;
  unfused   the parent's calls on the stored [M][L] assignment: ops.vq_soft_fwd for the forward, ops.vq_soft_bwd for the
            backward (which reads a stored p and dp; the fused backward recomputes p and forms dp = <dy, c> itself).
Prints one JSON line per dtype.

Run:  python scripts/bench_vq_bottleneck.py [--iters 30] [--warmup 5]
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

M, D, L, SIGMA = 4 * 1024 * 32 * 64 // 8, 8, 64, 10.0


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
  dpmf = torch.randn(L, generator=g).to(dev)
  for name, td in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
    x, dy = x32.to(td).contiguous(), dy32.to(td).contiguous()
    e = x.element_size()
    fwd_bytes, bwd_bytes = M * (2 * D * e + 4), 3 * M * D * e
    t = lambda fn: round(timed(fn, a.iters, a.warmup), 1)
    src_f = torch.empty(fwd_bytes // 2, dtype=torch.uint8, device=dev)
    src_b = torch.empty(bwd_bytes // 2, dtype=torch.uint8, device=dev)
    dst_f, dst_b = torch.empty_like(src_f), torch.empty_like(src_b)
    out = dict(bench='vq_bottleneck', dtype=name, M=M, D=D, L=L, fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes)
    out['fwd_hard_us'] = t(lambda: ops.vq_quantize_fwd(x, c, SIGMA, True))
    out['fwd_soft_us'] = t(lambda: ops.vq_quantize_fwd(x, c, SIGMA, False))
    out['fwd_hard_pmf_us'] = t(lambda: ops.vq_quantize_fwd(x, c, SIGMA, True, want_pmf=True))
    out['bwd_us'] = t(lambda: ops.vq_quantize_bwd(dy, x, c, SIGMA))
    out['bwd_dpmf_us'] = t(lambda: ops.vq_quantize_bwd(dy, x, c, SIGMA, dpmf))
    out['bwd_dx_only_us'] = t(lambda: ops.vq_quantize_bwd(dy, x, c, SIGMA, want_dc=False))
    out['copy_fwd_us'] = t(lambda: ops.copy_(src_f, dst_f))
    out['copy_bwd_us'] = t(lambda: ops.copy_(src_b, dst_b))
    out['unfused_soft_fwd_us'] = t(lambda: ops.vq_soft_fwd(x, c, SIGMA))
    p = ops.vq_soft_fwd(x, c, SIGMA)
    dp = torch.randn(M, L, device=dev)
    out['unfused_soft_bwd_us'] = t(lambda: ops.vq_soft_bwd(dp, p, x, c, SIGMA))
    del p, dp
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
