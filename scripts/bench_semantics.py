"""Coder of the label and instance maps at bench.py's workload, one process, one GPU: ms per call of ops.semantics_encode
(both kernels and the one copy to the host) and of ops.semantics_decode (the copy to the device and the kernel) at 1024x512,
batch 4, both planes, next to trainer.get_code and ops.code_entropy_encode (the code tensor's coder) from the
same run for scale.  The `*_kernels` figures are the device time of the launches alone (an event pair around `--steps`
back-to-back calls of the C entry point on buffers that stay on the device): what the coder costs without the host copies.

The maps are the synthetic batch's (piecewise-constant regions) and, with --golden, the recorded Cityscapes pair of
tests/golden/semantics_cityscapes.npz repeated over the batch; they stay on the device.  Alternating blocks of `--steps`
calls after `--warmup` warm-up calls each; the reported figure is the median block.  Prints ONE JSON line on stdout.

  python scripts/bench_semantics.py [--steps 10] [--warmup 3] [--blocks 3] [--strip_rows 8] [--golden]
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


def device_only(label, inst, items, H, W, sr):
  """(encode, decode): closures that call the two C entry points on resident buffers -- launches only, no host copy."""
  import ctypes
  import jpdse_hip
  L = jpdse_hip.lib()
  N, dev = int(label.shape[0]), label.device
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  S = (H + sr - 1) // sr
  cap, off = L.jpdse_semantics_capacity(H, W, sr, 3), L.jpdse_semantics_capacity(H, W, sr, 1)
  out = torch.empty((N, cap), dtype=torch.uint8, device=dev)
  meta = torch.zeros(4 * N, dtype=torch.int32, device=dev)
  ws = torch.empty(L.jpdse_semantics_workspace_size(N, H, W, sr, 3), dtype=torch.uint8, device=dev)
  stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def encode():
    jpdse_hip.check(L.jpdse_semantics_encode(N, H, W, sr, 3, P(label), P(inst), P(out), cap, P(meta[:2 * N]), P(meta[2 * N:]),
                                             P(ws), ws.numel(), stream()), 'semantics_encode')
  # the decoder's input: the payloads of `items` at the encoder's plane offsets (raw planes, size 0, are skipped by the kernel)
  rows = torch.zeros((N, cap), dtype=torch.uint8)
  sizes = torch.zeros((N, 2), dtype=torch.int32)
  for n, item in enumerate(items):
    for p, (mode, payload) in enumerate(item):
      if mode == 1:
        at = off if p else 0
        rows[n, at:at + len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
        sizes[n, p] = len(payload)
  rows, sizes = rows.to(dev), sizes.to(dev)
  dl, di = torch.empty_like(label), torch.empty_like(inst)
  bad = torch.empty(N, dtype=torch.int32, device=dev)

  def decode():
    jpdse_hip.check(L.jpdse_semantics_decode(N, H, W, sr, 3, 256, P(rows), cap, off, P(sizes), P(dl), P(di), P(bad), stream()),
                    'semantics_decode')
  return encode, decode


def time_device(fn, calls):
  """ms per call on the device: an event pair around `calls` back-to-back launches."""
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  for _ in range(calls):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3)
  ap.add_argument('--batch', type=int, default=4)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--strip_rows', type=int, default=8)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  ap.add_argument('--golden', action='store_true', help='also time the recorded Cityscapes pair (1024x512 only)')
  args = ap.parse_args()
  import numpy as np
  import jpdse_hip
  from jpdse_hip import ops
  from ctu.utils.synthetic import synthetic_batch
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  tr = build(args)
  tr.eval()
  H, W, sr = args.height, args.width, args.strip_rows
  with torch.no_grad():
    b = tr.model._code_act(xd)
  label, inst = tr.model._semantics(xd)
  items = ops.semantics_encode(label, inst, sr)
  back = ops.semantics_decode(items, H, W, sr, 256)
  same = bool(torch.equal(back[0], label) and torch.equal(back[1], inst))
  fns = {'get_code': lambda: tr.get_code(xd, packed=True), 'code_entropy_encode': lambda: ops.code_entropy_encode(b),
         'semantics_encode': lambda: ops.semantics_encode(label, inst, sr),
         'semantics_decode': lambda: ops.semantics_decode(items, H, W, sr, 256)}
  sizes = {'synthetic': [[len(e[1]) for e in it] for it in items]}
  modes = {'synthetic': [[e[0] for e in it] for it in items]}
  if args.golden:
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'semantics_cityscapes.npz'))
    gl = torch.from_numpy(d['label']).cuda().float().expand(args.batch, 1, H, W).contiguous()
    gi = torch.from_numpy(d['instance'].astype(np.int64)).cuda().expand(args.batch, 1, H, W).contiguous()
    gitems = ops.semantics_encode(gl, gi, sr)
    gback = ops.semantics_decode(gitems, H, W, sr, 256)
    same = same and bool(torch.equal(gback[0], gl) and torch.equal(gback[1], gi))
    fns['semantics_encode_real'] = lambda: ops.semantics_encode(gl, gi, sr)
    fns['semantics_decode_real'] = lambda: ops.semantics_decode(gitems, H, W, sr, 256)
    sizes['real'] = [[len(e[1]) for e in it] for it in gitems]
    modes['real'] = [[e[0] for e in it] for it in gitems]
  dev_fns = {}
  dev_fns['semantics_encode_kernels'], dev_fns['semantics_decode_kernels'] = device_only(label, inst, items, H, W, sr)
  if args.golden:
    dev_fns['semantics_encode_real_kernels'], dev_fns['semantics_decode_real_kernels'] = device_only(gl, gi, gitems, H, W, sr)
  gc.collect()
  gc.freeze()
  for fn in fns.values():
    for _ in range(args.warmup):
      fn()
  for fn in dev_fns.values():
    for _ in range(args.warmup):
      fn()
  times = {k: [] for k in list(fns) + list(dev_fns)}
  for _ in range(args.blocks):
    for k, fn in fns.items():
      times[k].append(time_calls(fn, args.steps))
    for k, fn in dev_fns.items():
      times[k].append(time_device(fn, args.steps))
  ms = {k: round(statistics.median(v), 3) for k, v in times.items()}
  print(json.dumps(dict(metric='ms_per_call', workload='%dx%d batch %d %s' % (W, H, args.batch, args.dtype),
                        strip_rows=sr, streams_per_plane=args.batch * ((H + sr - 1) // sr), pixels_per_stream=min(sr, H) * W,
                        raw_bytes_per_image=[H * W, 4 * H * W], payload_bytes_per_image=sizes, modes=modes,
                        roundtrip_equal=same, calls_per_block=args.steps, blocks=args.blocks, ms=ms,
                        blocks_ms={k: [round(x, 3) for x in v] for k, v in times.items()},
                        spread_pct={k: round(100.0 * (max(v) - min(v)) / statistics.median(v), 1) for k, v in times.items()},
                        device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
  main()
