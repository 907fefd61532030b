"""The MS-SSIM training distortion (jpdse_msssim_loss) in time, one process, one GPU.

One trainer (default 1024x512, batch 4, bf16, ngf 64: bench.py's workload) and four timed things, in alternating blocks of
`--calls` calls after `--warmup` warm-up calls each, the median block reported:
  loss_fwd       jpdse_msssim_loss, value only, on resident activations (device events around the enqueue)
  loss_fwd_bwd   the same call with the gradient
  step_l1        trainer.step under --distortion_loss_fn l1 (host clock around work that ends in a device synchronise)
  step_ms_ssim   trainer.step under --distortion_loss_fn ms_ssim, the same trainer and batch
Prints ONE JSON line on stdout.

  python scripts/bench_msssim_loss.py [--calls 10] [--warmup 3] [--blocks 5]
"""
import argparse
import contextlib
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=5)
  ap.add_argument('--batch', type=int, default=4)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  args = ap.parse_args()
  import jpdse_hip
  from jpdse_hip import ops
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt, synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, ngf=64, batch_size=args.batch)
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    tr = get_trainer(opt)(opt, 'train')
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}

  # resident activations for the kernel-only figures: the generator's output and the image in the compute dtype
  with torch.no_grad():
    pre = tr.model.preprocess(xd)
    fake, _ = tr.model.netG.fwd(tr.model._g_input_eval(pre))
    real = pre['real']
  slot = torch.zeros(1, dtype=torch.float32, device=fake.t.device)
  mean, std = opt.normalize_mean, opt.normalize_std

  def loss_fwd():
    ops.msssim_loss_fwd(fake, real, mean, std, slot)

  def loss_fwd_bwd():
    ops.msssim_loss_fwd_bwd(fake, real, mean, std, slot, 1.0)

  def step_as(flag):
    def fn():
      opt.distortion_loss_fn = flag
      tr.step(xd)
    return fn

  def host_block(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
      fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.calls

  def event_block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.calls):
      fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.calls

  things = dict(loss_fwd=(event_block, loss_fwd), loss_fwd_bwd=(event_block, loss_fwd_bwd),
                step_l1=(host_block, step_as('l1')), step_ms_ssim=(host_block, step_as('ms_ssim')))
  for _ in range(args.warmup):
    for _, fn in things.values():
      fn()
  torch.cuda.synchronize()
  value = float(slot.item())
  times = {k: [] for k in things}
  for _ in range(args.blocks):
    for k, (block, fn) in things.items():
      times[k].append(block(fn))
  opt.distortion_loss_fn = 'l1'
  ms = {k: statistics.median(v) for k, v in times.items()}
  L = jpdse_hip.lib()
  print(json.dumps(dict(
      metric='ms_per_call', workload='%dx%d batch %d %s ngf 64' % (args.width, args.height, args.batch, args.dtype),
      calls_per_block=args.calls, blocks=args.blocks, msssim_loss_fwd_ms=round(ms['loss_fwd'], 4),
      msssim_loss_fwd_bwd_ms=round(ms['loss_fwd_bwd'], 4), step_l1_ms=round(ms['step_l1'], 3),
      step_ms_ssim_ms=round(ms['step_ms_ssim'], 3), step_delta_ms=round(ms['step_ms_ssim'] - ms['step_l1'], 3),
      workspace_bytes=int(L.jpdse_msssim_loss_workspace_size(fake.N, fake.H, fake.W, fake.C, 1)),
      blocks_ms={k: [round(x, 4) for x in v] for k, v in times.items()}, loss_value=value,
      device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
  main()
