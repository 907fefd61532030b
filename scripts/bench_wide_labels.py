"""Train step at ADE20K's label width, one process, one GPU: 512x512, batch 4, bf16, ngf 64, num_labels 150 + don't-care +
instance edge = 155 input channels in 160 storage channels (the Cityscapes step has 39 in 40).

Times `--blocks` blocks of `--steps` steps after `--warmup` warm-up steps and reports the median block as ms/step: ONE JSON
line on stdout.  --layers adds the launches whose size depends on the label count, each timed outside a step with hipEvent
pairs (median of `--reps` calls, its pad / pack helper kernels included, as scripts/layer_profile.py times a conv call):
the input builder (three destinations), G's first conv forward and weight gradient, and PatchGAN layer 0 forward, weight
gradient and image-channel data gradient at both scales.  Kernel names are not visible from inside the process: run the same
command under `rocprofv3 --kernel-trace --stats -- python scripts/bench_wide_labels.py --layers` and read them from its
kernel statistics (the per-item call counts: reps + 1 calls of every item).

  python scripts/bench_wide_labels.py [--steps 10] [--warmup 3] [--blocks 3] [--layers]
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

NUM_LABELS = 150


def build(args):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  opt = default_opt(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, use_compressed=True, ngf=64,
                    batch_size=args.batch, num_labels=NUM_LABELS, contain_dontcare_label=True)
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    return get_trainer(opt)(opt, 'train')


def time_block(tr, xd, steps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    tr.step(xd)
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / steps


def layer_profile(tr, xd, reps):
  """[(name, median ms, GFLOP or GB)] of the label-count-dependent launches, on tensors of the step's shapes."""
  from jpdse_hip import ops
  m = tr.model
  pre = m.preprocess(xd, build_base=False)
  real, src, label, inst = pre['real'], pre['src'], pre['label'], pre['inst']
  B, H, W, C = real.N, real.H, real.W, m.label_nc + m.feat_nc
  dev = real.t.device
  rows = []

  def timed(name, fn, work, unit):
    fn()                                                    # first call: packs, workspace growth
    evs = []
    for _ in range(reps):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      out = fn()
      b.record()
      evs.append((a, b))
    torch.cuda.synchronize()
    rows.append((name, statistics.median(a.elapsed_time(b) for a, b in evs), work, unit))
    return out

  g_in = ops.Act.empty(B, H, W, C, m.cdtype, dev)
  d_in = ops.Act.empty(2 * B, H, W, C, m.cdtype, dev)
  dsts = [g_in, d_in.batch_slice(B, 2 * B), d_in.batch_slice(0, B)]
  nbytes = 3.0 * g_in.t.numel() * g_in.t.element_size()
  timed('input builder, 3 destinations x %d storage channels' % g_in.Cs,
        lambda: ops.input_builder(label, inst, m.n_onehot, dsts, [src, real, None], m.label_nc), nbytes / 1e9, 'GB')

  def conv_rows(what, conv, x, slice_grad):
    fl = lambda n, oh, ow, c: 2.0 * n * oh * ow * c * conv.cout * conv.k * conv.k / 1e9
    y, ctx = timed('%s fwd' % what, lambda: conv.fwd(x), None, 'GFLOP')
    rows[-1] = rows[-1][:2] + (fl(x.N, y.H, y.W, conv.cin), 'GFLOP')
    dy = y.empty_like()
    dy.t.normal_()
    dy.t[..., y.C:] = 0
    timed('%s weight gradient' % what, lambda: conv.bwd(ctx, dy, need_dx=False, need_dw=True, dy_is_dz=True), fl(x.N, y.H, y.W, conv.cin), 'GFLOP')
    if slice_grad:
      timed('%s data gradient, image channels' % what, lambda: conv.bwd_input_slice(ctx, dy, m.label_nc, C, dy_is_dz=True),
            fl(x.N, y.H, y.W, C - m.label_nc), 'GFLOP')

  g_first = m.netG._stages[0].conv
  conv_rows('G conv0 %dx%d reflect %d->%d' % (g_first.k, g_first.k, g_first.cin, g_first.cout), g_first, g_in, False)
  x = d_in
  for s in range(m.netD.num_D):                             # scale s sees the s-times pooled input (MultiscaleDiscriminator.fwd)
    d0 = m.netD._scales[m.netD.num_D - 1 - s]._stages[0]
    conv_rows('D scale %d layer 0 %dx%d s2 %d->%d at %dx%d' % (s, d0.k, d0.k, d0.cin, d0.cout, x.H, x.W), d0, x, True)
    x = ops.avgpool3s2_fwd(x)
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--batch', type=int, default=4)
  ap.add_argument('--width', type=int, default=512)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  ap.add_argument('--layers', action='store_true')
  args = ap.parse_args()
  import jpdse_hip
  from ctu.utils.synthetic import synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234, num_labels=NUM_LABELS + 1)    # ids 0..150: don't-care included
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  tr = build(args)
  gc.collect()
  gc.freeze()
  for _ in range(args.warmup):
    tr.step(xd)
  times = [time_block(tr, xd, args.steps) for _ in range(args.blocks)]
  res = dict(metric='ms_per_step', workload='%dx%d batch %d %s ngf 64 use_compressed, %d classes (%d input channels)'
             % (args.width, args.height, args.batch, args.dtype, tr.model.n_onehot, tr.model.label_nc + tr.model.feat_nc),
             steps_per_block=args.steps, blocks=args.blocks, ms_per_step=round(statistics.median(times), 3),
             blocks_ms=[round(t, 3) for t in times], device=torch.cuda.get_device_name(0))
  if args.layers:
    rows = layer_profile(tr, xd, args.reps)
    res['layers'] = [dict(name=n, ms=round(ms, 4), work=round(w, 2), unit=u,
                          rate=round(w / ms, 2 if u == 'GB' else 1), rate_unit='TB/s' if u == 'GB' else 'TFLOP/s')
                     for n, ms, w, u in rows]
    sys.stderr.write('label-count-dependent launches (%s, batch %d, %dx%d; median of %d, ms)\n'
                     % (args.dtype, args.batch, args.width, args.height, args.reps))
    for n, ms, w, u in rows:
      sys.stderr.write('  %8.3f  %-70s %9.2f %s  %7.2f %s\n' % (ms, n, w, u, w / ms, 'TB/s' if u == 'GB' else 'TFLOP/s'))
    conv0 = sum(ms for n, ms, _, _ in rows if n.startswith('G conv0'))
    res['g_conv0_fwd_plus_wgrad_ms'] = round(conv0, 3)
    res['g_conv0_share_of_step'] = round(conv0 / res['ms_per_step'], 4)
  print(json.dumps(res))


if __name__ == '__main__':
  main()
