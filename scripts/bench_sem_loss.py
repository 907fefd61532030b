"""The semantics-weighted distortion (jpdse_sem_weighted_loss) in time, one process, one GPU.

One trainer (default 1024x512, batch 4, bf16, ngf 64: bench.py's workload) and six timed things, in alternating blocks of
`--calls` calls after `--warmup` warm-up calls each, the median block reported:
  l1_fwd_bwd        ops.l1_fwd_bwd on resident activations: the plain path's value and gradient (device events)
  sem_fwd_bwd       ops.sem_weighted_loss on the same tensors with class weights and the edge term, value and gradient
  sem_class_only    the same without the instance map (edge weight 1: the ids are not read)
  sem_value         the weighted call, value only
  step_plain        trainer.step with the default flags (host clock around work that ends in a device synchronise)
  step_weighted     trainer.step of the same trainer and batch under --class_distortion_weights 24:4,26:2
                    --edge_distortion_weight 3
Prints ONE JSON line on stdout, with the bytes each kernel moves per pixel beside the times.

  python scripts/bench_sem_loss.py [--calls 20] [--warmup 3] [--blocks 5]
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
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=5)
  ap.add_argument('--batch', type=int, default=4)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  args = ap.parse_args()
  import jpdse_hip
  from jpdse_hip import ops
  from ctu.models.pix2pixHD_model import parse_class_distortion_weights
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt, synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, ngf=64, batch_size=args.batch)
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    tr = get_trainer(opt)(opt, 'train')
  assert tr.model.sem_weights is None
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  table, edge_w = parse_class_distortion_weights('24:4,26:2', tr.model.n_onehot), 3.0

  # resident activations for the kernel-only figures: the generator's output, the image, and the two maps
  with torch.no_grad():
    pre = tr.model.preprocess(xd)
    fake, _ = tr.model.netG.fwd(tr.model._g_input_eval(pre))
    real, label, inst = pre['real'], pre['label'], pre['inst']
  slot = torch.zeros(1, dtype=torch.float32, device=fake.t.device)

  def step_as(weights):
    def fn():
      tr.model.sem_weights = weights
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

  things = dict(
      l1_fwd_bwd=(event_block, lambda: ops.l1_fwd_bwd(fake, real, slot, 1.0)),
      sem_fwd_bwd=(event_block, lambda: ops.sem_weighted_loss(fake, real, label, inst, table, edge_w, 'l1', slot, 1.0)),
      sem_class_only=(event_block, lambda: ops.sem_weighted_loss(fake, real, label, None, table, 1.0, 'l1', slot, 1.0)),
      sem_value=(event_block, lambda: ops.sem_weighted_loss(fake, real, label, inst, table, edge_w, 'l1', slot)),
      step_plain=(host_block, step_as(None)),
      step_weighted=(host_block, step_as((table, edge_w))))
  for _ in range(args.warmup):
    for _, fn in things.values():
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in things}
  for _ in range(args.blocks):
    for k, (block, fn) in things.items():
      times[k].append(block(fn))
  tr.model.sem_weights = None
  ms = {k: statistics.median(v) for k, v in times.items()}
  es = 2 if args.dtype == 'bf16' else 4
  act = fake.Cs * es                                 # one tensor's stored lanes of a pixel
  bytes_px = dict(l1_fwd_bwd=3 * act, sem_fwd_bwd=3 * act + 4 + 8, sem_class_only=3 * act + 4, sem_value=2 * act + 4 + 8)
  npix = fake.N * fake.H * fake.W
  out = dict(metric='ms_per_call', workload='%dx%d batch %d %s ngf 64' % (args.width, args.height, args.batch, args.dtype),
             calls_per_block=args.calls, blocks=args.blocks)
  for k in ('l1_fwd_bwd', 'sem_fwd_bwd', 'sem_class_only', 'sem_value'):
    out[k + '_ms'] = round(ms[k], 4)
    out[k + '_bytes_per_pixel'] = bytes_px[k]
    out[k + '_gb_per_s'] = round(bytes_px[k] * npix / (ms[k] * 1e-3) / 1e9, 1)
  out.update(time_ratio_sem_over_l1=round(ms['sem_fwd_bwd'] / ms['l1_fwd_bwd'], 3),
             bytes_ratio_sem_over_l1=round(bytes_px['sem_fwd_bwd'] / bytes_px['l1_fwd_bwd'], 3),
             step_plain_ms=round(ms['step_plain'], 3), step_weighted_ms=round(ms['step_weighted'], 3),
             step_delta_ms=round(ms['step_weighted'] - ms['step_plain'], 3),
             blocks_ms={k: [round(x, 4) for x in v] for k, v in times.items()}, device=torch.cuda.get_device_name(0))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
