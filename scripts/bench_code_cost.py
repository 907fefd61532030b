"""Code-length map of the learned codec at bench.py's workload, one process, one GPU: ms per call of
ops.code_cost next to ops.code_entropy_encode -- the yardstick: existing code, the same serial walk with byte output instead
of a table lookup and a 4-byte store per symbol -- on the same tensor in the same run.

The trainer is the codec one of scripts/bench_entropy.py (1024x512, batch 4, bf16, nef 64, n_downsample_E 4, B 128: 512
streams of 2048 symbols, 32 x 64 cells); its eval code is computed once and stays on the device.  Two kinds of figure:
  device_ms   the library calls alone (jpdse_code_cost / jpdse_code_entropy_encode), back to back on one stream between two
              events: kernels, the table copy and the memsets, no host copy of a result.  The figure the 25 % rule is about.
  ms          the Python wrappers as a caller meets them, wall time: ops.code_entropy_encode ends in its one copy of the
              payload rows to the host, ops.code_cost is followed by the copy of its aggregates to the host, as the trainer
              does it.
code_cost runs in three forms: aggregates only, with the per-symbol tensor, and with the class tables of the batch's label map
(35 classes).  Alternating blocks of `--steps` calls after `--warmup` warm-up calls each; the reported figure is the median
block.  Prints ONE JSON line on stdout.

  python scripts/bench_code_cost.py [--steps 10] [--warmup 3] [--blocks 3]
"""
import argparse
import ctypes
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.join(ROOT, 'scripts')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402


def wall_ms(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / calls


def device_ms(fn, calls):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  start.record()
  for _ in range(calls):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / calls


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
  from jpdse_hip import ops, CodeCostArgs
  from ctu.utils.synthetic import synthetic_batch
  import bench_entropy
  jpdse_hip.require_gpu(0)
  torch.cuda.set_device(0)
  xd = synthetic_batch(args.batch, args.height, args.width, seed=1234)
  xd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in xd.items()}
  tr = bench_entropy.build(args)
  tr.eval()
  with torch.no_grad():
    b = tr.model._code_act(xd)
    label, _ = tr.model._semantics(xd)
  n_classes = tr.model.n_onehot
  N, h, w, C = b.N, b.H, b.W, b.C
  dev = b.t.device
  L = jpdse_hip.lib()
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  # the library calls alone, on buffers made once
  cap = L.jpdse_code_entropy_capacity(h, w, C)
  enc_ws = torch.empty(L.jpdse_code_entropy_workspace_size(N, h, w, C), dtype=torch.uint8, device=dev)
  enc_out = torch.empty(N * cap, dtype=torch.uint8, device=dev)
  enc_meta = torch.empty(2 * N, dtype=torch.int32, device=dev)

  def raw_encode():
    jpdse_hip.check(L.jpdse_code_entropy_encode(b.dtype, N, h, w, C, b.t.data_ptr(), enc_out.data_ptr(), cap, enc_meta[:N].data_ptr(),
                                                enc_meta[N:].data_ptr(), enc_ws.data_ptr(), enc_ws.numel(), stream), 'code_entropy_encode')
  cost_ws = torch.empty(L.jpdse_code_cost_workspace_size(N, h, w, C, n_classes), dtype=torch.uint8, device=dev)
  symbol = torch.empty((N, h, w, C), dtype=torch.int32, device=dev)
  cell = torch.empty((N, h, w), dtype=torch.int64, device=dev)
  channel = torch.empty((N, C), dtype=torch.int64, device=dev)
  units = torch.empty((N, n_classes + 1), dtype=torch.int64, device=dev)
  pixels = torch.empty((N, n_classes + 1), dtype=torch.int64, device=dev)

  def raw_cost(with_symbols=False, with_classes=False):
    a = CodeCostArgs(b.dtype, N, h, w, C, b.t.data_ptr(), int(label.shape[2]), int(label.shape[3]),
                     label.data_ptr() if with_classes else None, n_classes, symbol.data_ptr() if with_symbols else None,
                     cell.data_ptr(), channel.data_ptr(), units.data_ptr(), pixels.data_ptr(), cost_ws.data_ptr(), cost_ws.numel(),
                     stream.value)
    jpdse_hip.check(L.jpdse_code_cost(ctypes.byref(a)), 'code_cost')

  def cost_to_host(**kw):
    r = ops.code_cost(b, **kw)
    return [v.cpu() for k, v in r.items() if v is not None and k != 'symbol']

  device_fns = {'encode': raw_encode, 'cost': raw_cost, 'cost_symbols': lambda: raw_cost(with_symbols=True),
                'cost_classes': lambda: raw_cost(with_classes=True)}
  wall_fns = {'encode': lambda: ops.code_entropy_encode(b), 'cost': cost_to_host,
              'cost_classes': lambda: cost_to_host(label=label, n_classes=n_classes)}
  gc.collect()
  gc.freeze()
  for fn in list(device_fns.values()) + list(wall_fns.values()):
    for _ in range(args.warmup):
      fn()
  dev_t, wall_t = {k: [] for k in device_fns}, {k: [] for k in wall_fns}
  for _ in range(args.blocks):
    for k, fn in device_fns.items():
      dev_t[k].append(device_ms(fn, args.steps))
    for k, fn in wall_fns.items():
      wall_t[k].append(wall_ms(fn, args.steps))
  dms = {k: round(statistics.median(v), 4) for k, v in dev_t.items()}
  wms = {k: round(statistics.median(v), 4) for k, v in wall_t.items()}
  payloads = ops.code_entropy_encode(b)
  bits = ops.code_cost(b)['channel'].sum(dim=1).cpu().to(torch.float64) / ops.CODE_COST_UNIT
  print(json.dumps(dict(metric='ms_per_call', workload='%dx%d batch %d %s' % (args.width, args.height, args.batch, args.dtype),
                        codec='nef 64, n_downsample_E 4, B 128, feat_num 3', code_shape=[N, C, h, w], streams=N * C,
                        symbols_per_stream=h * w, n_classes=n_classes, device_ms=dms, ms=wms,
                        cost_over_encode_device=round(dms['cost'] / dms['encode'], 4),
                        stream_bytes_per_image=[len(p) - 4 * C for p in payloads], model_bits_per_image=[round(float(v), 3) for v in bits],
                        calls_per_block=args.steps, blocks=args.blocks,
                        device_blocks_ms={k: [round(x, 4) for x in v] for k, v in dev_t.items()},
                        blocks_ms={k: [round(x, 4) for x in v] for k, v in wall_t.items()},
                        device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
  main()
