"""Learned-codec step against the BPG-config step at bench.py's workload, one process, one GPU.

Both trainers are built side by side (1024x512, batch 4, bf16, ngf 64, use_compressed; the codec one adds netE with nef 64,
n_downsample_E 4, B 128, feat_num 3) and timed in alternating blocks of `--steps` steps after `--warmup` warm-up steps each;
the reported ms/step is the median block.  Prints ONE JSON line on stdout.  --layers also writes a per-layer profile of the
encoder's launches (forward, backward and the generator's feature-channel data gradient, hipEvent pairs around each layer
call outside a step) to stderr.  --decode times the receiver instead: trainer.decode (code import, the encoder's second
half, the generator) against trainer.get_img (the whole encoder, the generator) on the codec trainer alone, same workload,
same alternating blocks, the code and the batch resident on the device; one JSON line with both medians.

  python scripts/bench_learned_codec.py [--steps 10] [--warmup 3] [--blocks 3] [--layers | --decode]
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


def build(codec, args):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, use_compressed=True, ngf=64,
            batch_size=args.batch)
  if codec:
    kw.update(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=64, n_downsample_E=4,
              encoder_binarizer_out_channels=128)
  opt = default_opt(**kw)
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


def time_calls(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / calls


def decode_bench(args, xd):
  """ms per call of trainer.decode and trainer.get_img, alternating blocks in one process."""
  tr = build(True, args)
  code = tr.get_code(xd, packed=True)
  receiver = dict(label=xd['label'], instance=xd['instance'])
  fns = {'decode': lambda: tr.decode(code, receiver), 'get_img': lambda: tr.get_img(xd)}
  same = bool(torch.equal(fns['decode'](), fns['get_img']()))
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
  return dict(metric='ms_per_call', workload='%dx%d batch %d %s ngf 64 use_compressed' % (args.width, args.height, args.batch,
                                                                                          args.dtype),
              codec='nef 64, n_downsample_E 4, B 128, feat_num 3', calls_per_block=args.steps, blocks=args.blocks,
              decode_ms=round(ms['decode'], 3), get_img_ms=round(ms['get_img'], 3),
              ratio=round(ms['decode'] / ms['get_img'], 4), decode_equals_get_img=same,
              blocks_ms={k: [round(x, 3) for x in v] for k, v in times.items()}, device=torch.cuda.get_device_name(0))


def layer_profile(tr, xd, reps=5):
  """Per-layer kernel time of the encoder's forward / backward and of the generator's feature-channel data gradient."""
  from jpdse_hip import ops
  m = tr.model
  enc = m.netE
  pre = m.preprocess(xd, build_base=False)
  src = pre['src']
  rows = {}

  def timed(name, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    rows.setdefault(name, []).append((a, b))
    return out

  enc.train()
  for _ in range(reps):
    ctx_pre, h = [], src
    for i, st in enumerate(enc._pre):
      h, c = timed('fwd %s' % _name(st), lambda st=st, h=h: st.fwd(h))
      ctx_pre.append(c)
    binz = enc._binarizer
    t, cb = timed('fwd binarizer 1x1 conv + tanh', lambda: binz.conv.fwd(h))
    b = timed('fwd binarize (Philox sign)', lambda: ops.binarize_fwd(t, True, 0, 0, 0))
    ctx_post, y = [], b
    for st in enc._post:
      y, c = timed('fwd %s' % _name(st), lambda st=st, y=y: st.fwd(y))
      ctx_post.append(c)
    d = y.empty_like()
    d.t.normal_()
    for i in range(len(enc._post) - 1, -1, -1):
      st = enc._post[i]
      d = timed('bwd %s' % _name(st), lambda st=st, i=i, d=d: st.bwd(ctx_post[i], d, True, True))
    d = timed('bwd binarizer (tanh\' + 1x1 dgrad/wgrad)', lambda d=d: binz.bwd(cb, d, True, True))
    for i in range(len(enc._pre) - 1, -1, -1):
      st = enc._pre[i]
      d = timed('bwd %s' % _name(st), lambda st=st, i=i, d=d: st.bwd(ctx_pre[i], d, i > 0, True))
      if d is None:
        break
    # the generator's first layer: 7x7 reflect conv 39->64 at full resolution, data gradient of the 3 feature channels only
    g_first = m.netG._stages[0]
    g_in = ops.Act.empty(src.N, src.H, src.W, m.label_nc + 3, src.dtype, src.t.device)
    g_in.t.normal_()
    hg, cg = g_first.conv.fwd(g_in)
    dg = hg.empty_like()
    dg.t.normal_()
    timed('G first conv: feature-channel data gradient (7x7 reflect, 64 -> 3, full res)',
          lambda: g_first.conv.bwd_input_slice(cg, dg, m.label_nc, m.label_nc + 3))
  torch.cuda.synchronize()
  out = []
  for name, evs in rows.items():
    ms = statistics.median(a.elapsed_time(b) for a, b in evs)
    out.append((name, ms))
  return out


def _name(st):
  conv = getattr(st, 'conv', st)
  kind = 'convT' if conv.transposed else 'conv%dx%d' % (conv.k, conv.k)
  norm = ' + IN + ReLU' if hasattr(st, 'norm') else (' + tanh' if conv.act else '')
  return '%s %d->%d%s' % (kind, conv.cin, conv.cout, norm)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3)
  ap.add_argument('--batch', type=int, default=4)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  ap.add_argument('--layers', action='store_true')
  ap.add_argument('--decode', action='store_true', help='time trainer.decode against trainer.get_img instead of the steps')
  args = ap.parse_args()
  import jpdse_hip
  from ctu.utils.synthetic import synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  if args.decode:
    print(json.dumps(decode_bench(args, xd)))
    return
  trainers = {'bpg': build(False, args), 'learned_codec': build(True, args)}
  gc.collect()
  gc.freeze()
  for tr in trainers.values():
    for _ in range(args.warmup):
      tr.step(xd)
  times = {k: [] for k in trainers}
  for _ in range(args.blocks):
    for k, tr in trainers.items():
      times[k].append(time_block(tr, xd, args.steps))
  ms = {k: statistics.median(v) for k, v in times.items()}
  res = dict(metric='ms_per_step', workload='%dx%d batch %d %s ngf 64 use_compressed' % (args.width, args.height, args.batch,
                                                                                           args.dtype),
             codec='nef 64, n_downsample_E 4, B 128, feat_num 3', steps_per_block=args.steps, blocks=args.blocks,
             bpg_ms=round(ms['bpg'], 3), learned_codec_ms=round(ms['learned_codec'], 3),
             ratio=round(ms['learned_codec'] / ms['bpg'], 4),
             blocks_ms={k: [round(x, 3) for x in v] for k, v in times.items()},
             device=torch.cuda.get_device_name(0))
  if args.layers:
    rows = layer_profile(trainers['learned_codec'], xd)
    sys.stderr.write('encoder layer profile (%s, batch %d, %dx%d; median of 5, ms)\n' % (args.dtype, args.batch, args.width,
                                                                                        args.height))
    for name, t in rows:
      sys.stderr.write('  %8.3f  %s\n' % (t, name))
    sys.stderr.write('  %8.3f  total\n' % sum(t for _, t in rows))
  print(json.dumps(res))


if __name__ == '__main__':
  main()
