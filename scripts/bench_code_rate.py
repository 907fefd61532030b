"""Rate term of the learned codec at bench.py's workload, one process, one GPU: ms per call of
ops.code_rate_loss on the 4 x 128 x 32 x 64 code (soft mode with the gradient, as the train step calls it, and hard mode
without, as get_context_rate does), and ms per step of the learned-codec train step with and without --lambda_rate.

The trainers are the codec one of scripts/bench_learned_codec.py (1024x512, batch 4, bf16, nef 64, n_downsample_E 4, B 128),
built twice from one seed; the code and the tanh output behind it come from one training forward of the encoder and stay on the
device.  Alternating blocks of `--steps` calls / steps after `--warmup` warm-up ones each; the reported figure is the median
block.  Prints ONE JSON line on stdout.

  python scripts/bench_code_rate.py [--steps 10] [--warmup 3] [--blocks 3] [--lambda_rate 0.1]
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


def build(args, lambda_rate):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, use_compressed=True, ngf=64,
                    batch_size=args.batch, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=64,
                    n_downsample_E=4, encoder_binarizer_out_channels=128, lambda_rate=lambda_rate)
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
  ap.add_argument('--lambda_rate', type=float, default=0.1)
  args = ap.parse_args()
  import jpdse_hip
  from jpdse_hip import ops
  from ctu.utils.synthetic import synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  trainers = {'step': build(args, 0.0), 'step_lambda_rate': build(args, args.lambda_rate)}
  # the code and its tanh output: one training forward of the encoder's first half and the binarizer
  tr = trainers['step']
  tr.train()
  enc = tr.model.netE
  pre = tr.model.preprocess(xd, build_base=False)
  from jpdse_hip.layers import run_chain_fwd
  h, _ = run_chain_fwd(enc._pre, pre['src'])
  t, _ = enc._binarizer.conv.fwd(h)
  b = ops.binarize_fwd(t, True, 1234, 0, 0)
  pixels = args.height * args.width
  out = torch.empty(1, dtype=torch.float32, device=b.t.device)
  soft = ops.code_rate_loss(b, t, pixels, args.lambda_rate, want_grad=True, out=out)
  hard = ops.code_rate_loss(b, None, pixels, want_grad=False)
  values = dict(soft_bpp=round(float(soft[0].item()), 6), hard_bpp=round(float(hard[0].item()), 6))
  fns = {'code_rate': lambda: ops.code_rate_loss(b, t, pixels, args.lambda_rate, want_grad=True, out=out),
         'code_rate_hard': lambda: ops.code_rate_loss(b, None, pixels, want_grad=False, out=out)}
  for k, trn in trainers.items():
    fns[k] = lambda trn=trn: trn.step(xd)
  gc.collect()
  gc.freeze()
  for fn in fns.values():
    for _ in range(args.warmup):
      fn()
  times = {k: [] for k in fns}
  for _ in range(args.blocks):
    for k, fn in fns.items():
      times[k].append(time_calls(fn, args.steps))
  ms = {k: statistics.median(v) for k, v in times.items()}
  print(json.dumps(dict(metric='ms', workload='%dx%d batch %d %s ngf 64 use_compressed' % (args.width, args.height, args.batch,
                                                                                         args.dtype),
                        codec='nef 64, n_downsample_E 4, B 128, feat_num 3', code_shape=[b.N, b.C, b.H, b.W],
                        lambda_rate=args.lambda_rate, calls_per_block=args.steps, blocks=args.blocks,
                        code_rate_ms=round(ms['code_rate'], 4), code_rate_hard_ms=round(ms['code_rate_hard'], 4),
                        step_ms=round(ms['step'], 3), step_lambda_rate_ms=round(ms['step_lambda_rate'], 3),
                        step_delta_ms=round(ms['step_lambda_rate'] - ms['step'], 3),
                        g_rate=trainers['step_lambda_rate'].last_losses.get('G_Rate'), **values,
                        blocks_ms={k: [round(x, 4) for x in v] for k, v in times.items()},
                        device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
  main()
