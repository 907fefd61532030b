"""Entropy coder of the learned codec at bench.py's workload, one process, one GPU: ms per call of the device range coder
(ops.code_entropy_encode: both kernels and the one copy to the host) and of its decoder (ops.code_entropy_decode: the copy
to the device and the kernel), next to trainer.get_code (the encoder network and the packed export) for scale.

The trainer is the codec one of scripts/bench_learned_codec.py (1024x512, batch 4, bf16, nef 64, n_downsample_E 4, B 128:
512 streams of 2048 symbols); its eval code is computed once and stays on the device.  The coder is timed on that code and
on an i.i.d. p = 0.5 code of the same shape (the worst case for the byte traffic).  Alternating blocks of `--steps` calls after
`--warmup` warm-up calls each; the reported figure is the median block.  Prints ONE JSON line on stdout.

  python scripts/bench_entropy.py [--steps 10] [--warmup 3] [--blocks 3]
"""
import argparse
import contextlib
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402


def build(args):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, use_compressed=True, ngf=64,
                    batch_size=args.batch, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=64,
                    n_downsample_E=4, encoder_binarizer_out_channels=128)
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    return get_trainer(opt)(opt, 'train')


def time_calls(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3)
  ap.add_argument('--batch', type=int, default=4)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  args = ap.parse_args()
  import jpdse_hip
  from jpdse_hip import ops
  from ctu.utils.synthetic import synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  tr = build(args)
  tr.eval()
  with torch.no_grad():
    b = tr.model._code_act(xd)
  N, H, W, C = b.N, b.H, b.W, b.C
  noise = ops.Act(torch.where(torch.rand(b.t.shape, device=b.t.device) < 0.5, 1.0, -1.0).to(b.t.dtype), C)
  noise.t[..., C:] = 0
  payloads, noise_payloads = ops.code_entropy_encode(b), ops.code_entropy_encode(noise)
  raw = ops.code_export(b, packed=True)
  same = bool(torch.equal(ops.code_export(ops.code_entropy_decode(payloads, N, H, W, C, b.dtype), packed=True), raw))
  fns = {'get_code': lambda: tr.get_code(xd, packed=True),
         'encode': lambda: ops.code_entropy_encode(b), 'decode': lambda: ops.code_entropy_decode(payloads, N, H, W, C, b.dtype),
         'encode_noise': lambda: ops.code_entropy_encode(noise),
         'decode_noise': lambda: ops.code_entropy_decode(noise_payloads, N, H, W, C, b.dtype)}
  gc.collect()
  gc.freeze()
  for fn in fns.values():
    for _ in range(args.warmup):
      fn()
  times = {k: [] for k in fns}
  for _ in range(args.blocks):
    for k, fn in fns.items():
      times[k].append(time_calls(fn, args.steps))
  ms = {k: round(statistics.median(v), 3) for k, v in times.items()}
  print(json.dumps(dict(metric='ms_per_call', workload='%dx%d batch %d %s' % (args.width, args.height, args.batch, args.dtype),
                        codec='nef 64, n_downsample_E 4, B 128, feat_num 3', code_shape=[N, C, H, W], streams=N * C,
                        symbols_per_stream=H * W, raw_bytes_per_image=int(raw.shape[1]),
                        coded_bytes_per_image=[len(p) for p in payloads],
                        noise_coded_bytes_per_image=[len(p) for p in noise_payloads], roundtrip_equal=same,
                        calls_per_block=args.steps, blocks=args.blocks, ms=ms,
                        blocks_ms={k: [round(x, 3) for x in v] for k, v in times.items()},
                        device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
  main()
