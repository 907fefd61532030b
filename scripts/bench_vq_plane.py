"""Times and sizes the context coder of the S2HVQ index planes (vq_plane.hip) at the workload's code -- one
512 x 1024 image: h = 32, w = 64, G = 16 groups, L = 64 -- for strip_rows 4, 8 and 32, next to the order-0 coder (vq_coder.hip,
4.14) on the same indices at S = 128 in the same run.  The ops calls are host-synchronous (the encode ends with its one copy to
the host, the decode starts with the copy to the device and ends with the read of its status word), so the times are wall-clock
medians of whole calls.  One lane codes one stream serially: latency figures, not throughput ones.

Three sources: uniform iid indices; the correlated source of the tests (a cell repeats its left neighbour with probability
0.6, else its upper one with probability 0.5, else a fresh draw); and the eval-mode code of a freshly initialised encoder on a
ctu.utils.synthetic image -- an UNTRAINED encoder on a SYNTHETIC image: it says nothing about a trained one.  Prints one JSON
line per (source, coder, strip_rows).

Run:  python scripts/bench_vq_plane.py [--iters 10] [--warmup 2]
"""
import argparse
import contextlib
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

H, W, G, L = 32, 64, 16, 64
M = H * W * G
STRIP_ROWS = (4, 8, 32)
ORDER0_STREAMS = 128


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


def correlated(rng):
  """The correlated source of tests/vq_plane_cases.py, restated: int32 [H * W * G]."""
  v = np.zeros((H, W, G), dtype=np.int64)
  left, up, fresh = rng.random((H, W, G)) < 0.6, rng.random((H, W, G)) < 0.5, rng.integers(0, L, size=(H, W, G))
  for y in range(H):
    for x in range(W):
      cell = fresh[y, x].copy()
      if y > 0:
        cell = np.where(up[y, x], v[y - 1, x], cell)
      if x > 0:
        cell = np.where(left[y, x], v[y, x - 1], cell)
      v[y, x] = cell
  return v.reshape(-1).astype(np.int32)


def untrained_encoder_code(dev):
  """The eval-mode code of a freshly initialised encoder (seed 1234, the code book scaled to the features so that more than
  one centre is in use) on one synthetic 512 x 1024 image: int32 [H * W * G]."""
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt, synthetic_batch
  opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype='bf16', ngf=16, n_blocks_global=1, no_feat_encoding=False,
                    no_encoder_binarization=False, feat_num=3, nef=64, n_downsample_E=4, encoder_binarizer_out_channels=128,
                    encoder_quantizer='s2hvq', vq_n_center=L, vq_center_size=8, no_vgg_loss=True)
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    trainer = get_trainer(opt)(opt, 'train')
  with torch.no_grad():
    trainer.model.netE._vq.vq._code_book.mul_(0.05)
  code = trainer.get_vq_code(synthetic_batch(1, 16 * H, 16 * W, seed=3))
  assert tuple(code.shape) == (1, M), tuple(code.shape)
  return code.view(-1).to(torch.int32).to(dev)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  a = ap.parse_args()
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  rng = np.random.default_rng(0)
  sources = {'uniform': torch.from_numpy(rng.integers(0, L, size=M).astype(np.int32)).to(dev),
             'correlated': torch.from_numpy(correlated(rng)).to(dev),
             'untrained_encoder_on_synthetic': untrained_encoder_code(dev)}
  packed = M * ops.vq_index_bits(L) // 8
  for name, index in sources.items():
    common = {'bench': 'vq_plane', 'source': name, 'h': H, 'w': W, 'G': G, 'L': L, 'packed_bytes': packed,
              'distinct_indices': int(torch.unique(index).numel())}
    S = ORDER0_STREAMS
    payload = ops.vq_index_encode(index, L, S)
    assert torch.equal(ops.vq_index_decode(payload, M, L, S, dev), index)
    enc = timed(lambda: ops.vq_index_encode(index, L, S), a.iters, a.warmup)
    dec = timed(lambda: ops.vq_index_decode(payload, M, L, S, dev), a.iters, a.warmup)
    print(json.dumps(dict(common, coder='order0', S=S, encode_ms=round(enc, 3), decode_ms=round(dec, 3),
                          coded_bytes=len(payload))), flush=True)
    for rows in STRIP_ROWS:
      payload = ops.vq_plane_encode(index, H, W, G, L, rows)
      assert torch.equal(ops.vq_plane_decode(payload, H, W, G, L, rows, dev), index)
      enc = timed(lambda: ops.vq_plane_encode(index, H, W, G, L, rows), a.iters, a.warmup)
      dec = timed(lambda: ops.vq_plane_decode(payload, H, W, G, L, rows, dev), a.iters, a.warmup)
      print(json.dumps(dict(common, coder='context', strip_rows=rows, S=ops.vq_plane_streams(H, G, rows), encode_ms=round(enc, 3),
                            decode_ms=round(dec, 3), coded_bytes=len(payload))), flush=True)


if __name__ == '__main__':
  main()
