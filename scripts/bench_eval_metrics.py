"""get_eval_metrics against the two get_eval_loss calls it replaces, one process, one GPU.

One trainer (default 1024x512, batch 4, bf16, ngf 64: bench.py's generator) and three timed things, in alternating blocks of
`--calls` calls after `--warmup` warm-up calls each, the median block reported:
  metrics      trainer.get_eval_metrics(x): one generator forward + jpdse_eval_metrics + one read-back
  two_losses   the way to get the L1 / MSE pair without it: get_eval_loss under --distortion_loss_fn l1, then mse: two forwards
  kernels      jpdse_eval_metrics alone on resident activations (device events around the enqueue, no read-back)
and with --per-class two more in the same alternation:
  metrics_cls  trainer.get_eval_metrics(x, per_class=True): the same forward, jpdse_eval_metrics_sem, one read-back
  kernels_cls  jpdse_eval_metrics_sem alone on the same activations and the batch's label map
Host clock around work that ends in a device synchronise for the first two (each call reads a result back), hipEvents for the
third.  Prints ONE JSON line on stdout.  --once runs a single get_eval_metrics after warm-up (for a kernel trace).

  python scripts/bench_eval_metrics.py [--calls 10] [--warmup 3] [--blocks 5] [--once] [--per-class]
"""
import argparse
import contextlib
import ctypes
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
  ap.add_argument('--once', action='store_true')
  ap.add_argument('--per-class', action='store_true', help='also time the per-class call and its kernels')
  args = ap.parse_args()
  import jpdse_hip
  from jpdse_hip import ops, F32
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

  def metrics():
    return tr.get_eval_metrics(xd)

  def metrics_cls():
    return tr.get_eval_metrics(xd, per_class=True)

  def two_losses():
    out = []
    for flag in ('l1', 'mse'):
      opt.distortion_loss_fn = flag
      out.append(tr.get_eval_loss(xd))
    opt.distortion_loss_fn = 'l1'
    return out

  # resident activations for the kernel-only figure
  with torch.no_grad():
    pre = tr.model.preprocess(xd)
    fake, _ = tr.model.netG.fwd(tr.model._g_input_eval(pre))
    real32 = ops.nchw_to_nhwc(pre['image_nchw'], F32)
  L = jpdse_hip.lib()
  ws = ops.workspace(L.jpdse_eval_metrics_workspace_size(fake.N, fake.H, fake.W, fake.C), fake.t.device)
  out = torch.empty((fake.N, 14), dtype=torch.float64, device=fake.t.device)
  arr = ctypes.c_double * 3
  mean, std = arr(*opt.normalize_mean), arr(*opt.normalize_std)

  def kernels_enqueue():
    jpdse_hip.check(L.jpdse_eval_metrics(fake.dtype, real32.dtype, fake.N, fake.H, fake.W, fake.C, fake.t.data_ptr(),
                                         real32.t.data_ptr(), mean, std, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream), 'eval_metrics')

  n_cls = tr.model.n_onehot
  label = pre['label']
  ws_cls = ops.workspace(L.jpdse_eval_metrics_sem_workspace_size(fake.N, fake.H, fake.W, fake.C, n_cls), fake.t.device)
  cls = torch.empty((fake.N, n_cls + 1, 3), dtype=torch.int64, device=fake.t.device)

  def kernels_cls_enqueue():
    a = jpdse_hip.EvalMetricsSemArgs(fake.dtype, real32.dtype, fake.N, fake.H, fake.W, fake.C, fake.t.data_ptr(),
                                     real32.t.data_ptr(), label.data_ptr(), n_cls, mean, std, out.data_ptr(), cls.data_ptr(),
                                     ws_cls.data_ptr(), ws_cls.numel(), torch.cuda.current_stream().cuda_stream)
    jpdse_hip.check(L.jpdse_eval_metrics_sem(ctypes.byref(a)), 'eval_metrics_sem')

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

  for _ in range(args.warmup):
    m = metrics()
    pair = two_losses()
    kernels_enqueue()
    if args.per_class:
      mc = metrics_cls()
      kernels_cls_enqueue()
  torch.cuda.synchronize()
  if args.per_class:
    assert torch.equal(mc['raw'], m['raw']) and torch.equal(mc['per_class']['raw'], cls.cpu())
  assert [m['l1'], m['mse']] == pair, 'get_eval_metrics and get_eval_loss disagree: %r vs %r' % ((m['l1'], m['mse']), pair)
  if args.once:
    m = metrics()
    print(json.dumps({k: m[k] for k in ('l1', 'mse', 'psnr', 'ms_ssim')}))
    return
  times = dict(metrics=[], two_losses=[], kernels=[])
  if args.per_class:
    times.update(metrics_cls=[], kernels_cls=[])
  for _ in range(args.blocks):
    times['metrics'].append(host_block(metrics))
    times['two_losses'].append(host_block(two_losses))
    times['kernels'].append(event_block(kernels_enqueue))
    if args.per_class:
      times['metrics_cls'].append(host_block(metrics_cls))
      times['kernels_cls'].append(event_block(kernels_cls_enqueue))
  ms = {k: statistics.median(v) for k, v in times.items()}
  extra = {}
  if args.per_class:
    extra = dict(get_eval_metrics_per_class_ms=round(ms['metrics_cls'], 3),
                 eval_metrics_sem_kernels_ms=round(ms['kernels_cls'], 4), n_classes=n_cls,
                 per_class_ratio=round(ms['metrics_cls'] / ms['metrics'], 4))
  print(json.dumps(dict(
      metric='ms_per_call', workload='%dx%d batch %d %s ngf 64' % (args.width, args.height, args.batch, args.dtype),
      calls_per_block=args.calls, blocks=args.blocks, get_eval_metrics_ms=round(ms['metrics'], 3),
      two_get_eval_loss_ms=round(ms['two_losses'], 3), eval_metrics_kernels_ms=round(ms['kernels'], 4),
      ratio=round(ms['metrics'] / ms['two_losses'], 4), blocks_ms={k: [round(x, 4) for x in v] for k, v in times.items()},
      values={k: m[k] for k in ('l1', 'mse', 'psnr', 'ms_ssim')}, device=torch.cuda.get_device_name(0), **extra)))


if __name__ == '__main__':
  main()
