"""Dump what the residual S2HVQ entry points compute, as arrays: every output tensor of ops.vq_res_fwd, vq_res_rows_fwd, vq_res_decode,
vq_res_bwd, vq_res_ec_assign and vq_res_rate_fwd on a fixed, seeded list of small cases into one .npz, for comparing two builds of
the library byte for byte (needs a GPU; under a minute).  The cases are the smallest shapes at which the kernels of vq_residual.hip,
vq_res_ec.hip and vq_res_rate.hip take another path: every D in {3, 4, 8, 12, 16, 20, 32} (each DP with and without
padding) against L in {5, 64, 512} (the book staged in LDS or not), M in {1, 255, 257, 700, 704, 1344} (tails; the last two for the
groups 16 and 64), n in {1, 3, 4} of S = 4 stages, fp32 and bf16, an x that starts at an odd element (the non-vector row path),
G in {1, 3, 16, 64} (the shuffle and the general path of the grouped kernels), the EC bias absent, finite and with +inf rows, the
backward plain, grouped with a dhist slice that fits LDS and one that does not, with a mixed depth map and with dx or dbooks
absent, and one M per launch geometry at which a block walks more than one tile.  A combination that an entry point refuses (G
does not divide M) is skipped.

  JPDSE_HIP_LIB=/path/to/libjpdse_hip.so python scripts/dump_vq_res_surface.py --out a.npz    # one build per process
  python scripts/dump_vq_res_surface.py --compare a.npz b.npz                                   # no GPU: names and a count
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

S, SIGMA = 4, 4.0
DS, LS, MS, NS, GS = (3, 4, 8, 12, 16, 20, 32), (5, 64, 512), (1, 255, 257, 700, 704, 1344), (1, 3, 4), (1, 3, 16, 64)


def compare(a_path, b_path):
  a, b = np.load(a_path), np.load(b_path)
  names = sorted(set(a.files) | set(b.files))
  bad = [n for n in names if n not in a.files or n not in b.files or a[n].dtype != b[n].dtype or a[n].shape != b[n].shape or
         a[n].tobytes() != b[n].tobytes()]
  for n in bad:
    print('differs: ' + n)
  print('%d arrays compared, %d differ' % (len(names), len(bad)))
  return 1 if bad else 0


def dump(out_path):
  import torch
  import jpdse_hip
  from jpdse_hip import ops
  jpdse_hip.require_gpu(0)
  dev = torch.device('cuda', 0)
  g = torch.Generator(device=dev).manual_seed(20261021)
  arrays = {}

  def put(case, **tensors):
    for k, t in tensors.items():
      if t is None:
        continue
      t = t.detach().cpu().contiguous()
      arrays['%s %s' % (case, k)] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()

  def make(M, D, L, dtype, odd=False):
    books = torch.stack([(torch.rand(L, D, generator=g, device=dev) * 2 - 1) * 0.5 ** s for s in range(S)]).contiguous()
    flat = torch.randn(M * D + 1, generator=g, device=dev).to(dtype)
    x = flat[1:].view(M, D) if odd else flat[:M * D].view(M, D)
    dy = torch.randn(M, D, generator=g, device=dev).to(dtype)
    return x, dy, books

  def depth_map(cells):                            # mixed: every depth 0 .. S + 1 (clamped on the device), no two neighbours alike
    return (torch.arange(cells, device=dev, dtype=torch.int32) * 5 + 1) % (S + 2)

  def plain(case, M, D, L, n, dtype, odd=False, light=False):
    x, dy, books = make(M, D, L, dtype, odd)
    y, index, sse, residual = ops.vq_res_fwd(x, books, n, want_sse=True, want_residual=True)
    put(case + ' fwd', y=y, index=index, sse=sse, residual=residual)
    yr, ir = ops.vq_res_rows_fwd(x, books, n)
    put(case + ' rows', y=yr, index=ir)
    dx, dc = ops.vq_res_bwd(dy, x, books, ir, SIGMA)
    put(case + ' bwd', dx=dx, dbooks=dc)
    if light:
      return
    yd, st = ops.vq_res_decode(ir, books, n, dtype=dtype)
    put(case + ' decode', y=yd, status=st)
    put(case + ' bwd no dx', dbooks=ops.vq_res_bwd(dy, x, books, ir, SIGMA, want_dx=False)[1])
    put(case + ' bwd no dbooks', dx=ops.vq_res_bwd(dy, x, books, ir, SIGMA, want_dc=False)[0])
    for cell in (1, 3, 16):
      if M % cell:
        continue
      depth = depth_map(M // cell)
      yq, iq = ops.vq_res_rows_fwd(x, books, n, depth=depth, groups=cell)
      put('%s depth cell %d rows' % (case, cell), y=yq, index=iq)
      yd, st = ops.vq_res_decode(iq, books, n, dtype=dtype, depth=depth, groups=cell)
      put('%s depth cell %d decode' % (case, cell), y=yd, status=st)
      dx, dc = ops.vq_res_bwd(dy, x, books, iq, SIGMA, groups=cell, depth=depth)
      put('%s depth cell %d bwd' % (case, cell), dx=dx, dbooks=dc)
      put('%s depth cell %d bwd no dbooks' % (case, cell), dx=ops.vq_res_bwd(dy, x, books, iq, SIGMA, want_dc=False, groups=cell, depth=depth)[0])

  def grouped(case, M, D, L, n, G, dtype, odd=False, bwd=True):
    if M % G or n * G * L > 65536:
      return
    x, dy, books = make(M, D, L, dtype, odd)
    y, index, hist, sse = ops.vq_res_ec_assign(x, books, None, G, n)
    put(case + ' ec', y=y, index=index, hist=hist, sse=sse)
    bias = ops.vq_ec_lengths(hist.view(n * G, L), 0.5)[0].view(n, G, L).contiguous()      # +inf on every empty bin
    finite = torch.where(torch.isfinite(bias), bias, torch.full_like(bias, 3.0))
    walls = finite.clone()
    walls[:, ::2, :] = float('inf')                # whole rows of +inf: index 0
    for name, b in (('finite bias', finite), ('lengths bias', bias), ('inf rows', walls)):
      y, index, hist, sse = ops.vq_res_ec_assign(x, books, b, G, n)
      put('%s ec %s' % (case, name), y=y, index=index, hist=hist, sse=sse)
    put(case + ' ec finite bias, index alone', index=ops.vq_res_ec_assign(x, books, finite, G, n, want_y=False, want_stats=False)[1])
    rate, rates, hist, dhist, y, index = ops.vq_res_rate_fwd(x, books, SIGMA, G, float(M * D), 0.5, n, want_code=True, want_hist=True)
    put(case + ' rate', rate=rate, rates=rates, hist=hist, dhist=dhist, y=y, index=index)
    rate, rates, _, dhist2, _, _ = ops.vq_res_rate_fwd(x, books, SIGMA, G, float(M * D), 0.5, n)
    put(case + ' rate without a code', rate=rate, rates=rates, dhist=dhist2)
    if not bwd:
      return
    dx, dc = ops.vq_res_bwd(dy, x, books, index, SIGMA, groups=G, dhist=dhist)
    put(case + ' bwd grouped', dx=dx, dbooks=dc)
    put(case + ' bwd grouped no dbooks', dx=ops.vq_res_bwd(dy, x, books, index, SIGMA, want_dc=False, groups=G, dhist=dhist)[0])
    put(case + ' bwd grouped no dhist', dx=ops.vq_res_bwd(dy, x, books, index, SIGMA, want_dc=False, groups=G)[0])

  f32, bf16 = torch.float32, torch.bfloat16
  names = {f32: 'fp32', bf16: 'bf16'}
  for dtype in (f32, bf16):
    for D in DS:                                   # every DP, padded or not, against every book path
      for L in LS:
        plain('%s M 257 D %d L %d n 3' % (names[dtype], D, L), 257, D, L, 3, dtype)
        grouped('%s M 704 D %d L %d n 3 G 16' % (names[dtype], D, L), 704, D, L, 3, 16, dtype)
    for M in MS:                                   # the tails, the stages, the groups
      for n in NS:
        plain('%s M %d D 8 L 64 n %d' % (names[dtype], M, n), M, 8, 64, n, dtype)
        for G in GS:
          grouped('%s M %d D 8 L 64 n %d G %d' % (names[dtype], M, n, G), M, 8, 64, n, G, dtype)
    for D, L in ((8, 64), (16, 512)):              # x from an odd element: no 16-byte rows
      plain('%s odd M 257 D %d L %d n 4' % (names[dtype], D, L), 257, D, L, 4, dtype, odd=True)
      grouped('%s odd M 255 D %d L %d n 4 G 3' % (names[dtype], D, L), 255, D, L, 4, 3, dtype, odd=True)
    for G in GS:                                   # G 64: a dhist slice of 64 x 513 words does not fit LDS
      grouped('%s M 704 D 32 L 512 n 2 G %d' % (names[dtype], G), 704, 32, 512, 2, G, dtype)
      grouped('%s M 1344 D 32 L 64 n 4 G %d' % (names[dtype], G), 1344, 32, 64, 4, G, dtype)
    # a block walks more than one tile: rows forward and backward (1024 blocks of 256); the grouped kernels with 64 blocks of 256
    # (G 64: the general path; G does not divide 16384 + 300, the next multiple is taken) and with 512 blocks of 128 (the shuffle path)
    plain('%s M 262444 D 4 L 5 n 4' % names[dtype], 262144 + 300, 4, 5, 4, dtype, light=True)
    grouped('%s M 16704 D 8 L 256 n 4 G 64' % names[dtype], 16384 + 320, 8, 256, 4, 64, dtype, bwd=False)
    grouped('%s M 262464 D 4 L 5 n 4 G 16' % names[dtype], 262144 + 320, 4, 5, 4, 16, dtype, bwd=False)
    grouped('%s M 65856 D 8 L 64 n 4 G 16' % names[dtype], 65536 + 320, 8, 64, 4, 16, dtype, bwd=False)
  torch.cuda.synchronize()
  np.savez(out_path, **arrays)
  print(out_path)


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--out')
  ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
  args = ap.parse_args()
  if (args.out is None) == (args.compare is None):
    sys.exit(__doc__)
  sys.exit(compare(*args.compare) if args.compare else dump(args.out))
