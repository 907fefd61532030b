"""Rate-distortion evaluation loop on the device path: the numbers of the reference's test.py (its per-batch and test-set lines:
L1 / MSE / MS-SSIM, bpp before / after entropy coding when the learned codec is on) plus PSNR, without the visualiser and the
HTML page.  Per batch: trainer.get_eval_metrics (one generator forward) and, with the codec, trainer.get_eval_rate and
trainer.get_context_rate (the context model's estimate of the code's length in bits per pixel).

Batches: seeded synthetic ones (ctu.utils.synthetic), or --data DIR holding pre-decoded batches as *.pt files, each a dict with
the x_dict keys (label, instance, image, optionally compressed_img, path).  The test-set line averages the per-batch values
over the batches, as the reference does (so, like there, a ragged last batch weighs as much as a full one); a second line
gives the per-image averages, which are the ones to quote.  PSNR is the mean of the per-image PSNRs.  --per-class adds the
table of the distortion per semantic class over the whole test set (pixel-weighted: the raw integer sums of every batch are
added before the division), from the same device pass; --zero_sem / --zero_ins / --zero_vis run the reference's ablations.

--roundtrip DIR (needs --codec) evaluates what a receiver reconstructs: every image's packed code is written to
DIR/b<batch>_i<image>.jpdc (ctu.utils.bitstream), read back, and the batch is decoded from the files and the label /
instance maps alone (trainer.get_eval_metrics_decoded).  The reported distortion is then that of the decoded images, the
line gains the bpp of the files (header included) beside get_eval_rate's actual_bpp, and the largest absolute difference
between the decoded image and get_img's: 0 unless the eval code holds an exact zero, which is stored as a 0 bit and decoded
as -1 while get_img feeds the 0 forward.

--entropy (needs --codec) adds the bpp a coder actually produced: trainer.get_coded_rate, the size of each image's .jpda file
(ctu.utils.entropy: the range-coded payload of DESIGN.md 4.8, or the raw one where coding does not pay), header included,
beside get_eval_rate's Shannon estimate.  With --roundtrip the files written and decoded from are those .jpda files.

  python scripts/eval_rd.py [--batches 4] [--batch 2] [--width 1024] [--height 512] [--dtype bf16] [--codec]
                            [--checkpoints_dir DIR] [--data DIR] [--per-class] [--zero_sem] [--zero_ins] [--zero_vis]
                            [--roundtrip DIR] [--entropy] [--semantics] [--rate-map DIR]

--semantics (needs --codec --entropy --roundtrip DIR) completes the stream: every image's label and instance maps are coded
(trainer.get_coded_semantics) and written as a .jpds file beside the .jpda one, the receiver's maps come from
those files alone (trainer.decode_semantics), the decoded image is checked against get_img under the zero rule above, and
the line gains the three rates trainer.get_total_rate reports (code, semantics and total bpp, headers included), taken from
the sizes of the files just written.

With --codec, --per-class also says where the bits go: next to each class's L1 / MSE / PSNR the table gains
the bits of the code attributed to the class (trainer.get_class_rates: the code length under the 4.8 coder's own adaptive
model, a cell's bits shared evenly among the pixels it covers), its bpp (bits / pixels of the class) and its share of all
bits.  --rate-map DIR (needs --codec) writes the map behind it, trainer.get_rate_map's float64 [h, w] bits per code cell, as
DIR/b<batch>_i<image>.npy, and the line gains the model's bpp.  With --encoder_quantizer s2hvq the same columns and the same
map come from trainer.get_vq_class_rates / get_vq_rate_map: the code length under the model of the coder
whose file get_coded keeps for each image.
"""
import argparse
import contextlib
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402


def batches(args):
  if args.data:
    files = sorted(glob.glob(os.path.join(args.data, '*.pt')))
    if not files:
      raise SystemExit('no *.pt batch under %s' % args.data)
    for f in files:
      yield torch.load(f)
  else:
    from ctu.utils.synthetic import synthetic_batch
    for i in range(args.batches):
      yield synthetic_batch(args.batch, args.height, args.width, seed=1234 + i)


def roundtrip(trainer, x_dict, folder, batch_index, coded=False):
  """Encode x_dict, store one file per image, read the files back: (code [N, bytes] uint8 tensor, file bpp per image).
  coded: .jpda files (ctu.utils.entropy) instead of .jpdc ones; the rows of their range-coded payloads are decoded on the
  device (ops.code_entropy_decode) and re-packed, so the receiver below is the same for both kinds of file."""
  from ctu.utils import bitstream, entropy
  from jpdse_hip import ops
  code = trainer.get_code(x_dict, packed=True).cpu()
  payloads = trainer.get_coded(x_dict) if coded else None
  H, W = int(x_dict['label'].shape[-2]), int(x_dict['label'].shape[-1])
  shape = trainer.model.netE.code_shape(H, W)
  rows, bpp = [], []
  for j in range(code.shape[0]):
    path = os.path.join(folder, 'b%04d_i%02d%s' % (batch_index, j, entropy.SUFFIX if coded else '.jpdc'))
    if coded:
      entropy.write_coded(path, payloads[j], code[j], shape)
      row, mode, got = entropy.read_coded(path)
      if mode == entropy.MODE_CODED:
        C, h, w = got
        b = ops.code_entropy_decode([row], 1, h, w, C, trainer.model.cdtype, trainer.model._device())
        row = ops.code_export(b, packed=True)[0].cpu()
    else:
      bitstream.write_code(path, code[j], shape)
      row, got = bitstream.read_code(path)
    if tuple(got) != tuple(shape):
      raise SystemExit('%s: code shape %s, expected %s' % (path, got, shape))
    rows.append(row)
    bpp.append(8.0 * os.path.getsize(path) / (H * W))
  return torch.stack(rows), bpp


def semantics_roundtrip(trainer, x_dict, folder, batch_index):
  """Code the maps of x_dict, store one .jpds file per image, read the files back: (the receiver's {'label', 'instance'},
  file bpp per image)."""
  from ctu.utils import semantics
  blobs = trainer.get_coded_semantics(x_dict)
  pixels = int(x_dict['label'].shape[-2]) * int(x_dict['label'].shape[-1])
  back, bpp = [], []
  for j, blob in enumerate(blobs):
    path = os.path.join(folder, 'b%04d_i%02d%s' % (batch_index, j, semantics.SUFFIX))
    bpp.append(8.0 * semantics.write(path, blob) / pixels)
    back.append(semantics.read(path))
  return trainer.decode_semantics(back), bpp


def rate_lambda_rows(trainer, args, lambdas):
  """One row per multiplier: the files of the entropy-constrained code and the distortion of the images decoded from it."""
  data = list(batches(args))
  print('%10s %10s %10s %10s %10s' % ('lambda', 'coded bpp', 'L1', 'PSNR', 'MS-SSIM'))
  for lam in lambdas:
    bpp, l1, psnr, ms, n = 0.0, 0.0, 0.0, 0.0, 0
    for x_dict in data:
      code = trainer.get_vq_code(x_dict, rate_lambda=lam, n_iter=args.vq_rate_iters)
      m = trainer.get_eval_metrics_decoded(code, x_dict)
      bpp += trainer.get_coded_rate_ec(x_dict, rate_lambda=lam, n_iter=args.vq_rate_iters)[0]
      l1, psnr, ms, n = l1 + m['l1'], psnr + m['psnr'], ms + m['ms_ssim'], n + 1
    print('%10g %10.5f %10.4f %10.3f %10.5f' % (lam, bpp / n, l1 / n, psnr / n, ms / n))


def stage_curve_rows(trainer, args):
  """One row per stage prefix of the residual bottleneck's stream: trainer.get_stage_curve, batch means."""
  rows, n = None, 0
  for x_dict in batches(args):
    curve = trainer.get_stage_curve(x_dict)
    rows = curve if rows is None else [{k: a[k] + b[k] for k in a} for a, b in zip(rows, curve)]
    n += 1
  print('%10s %10s %10s %10s %10s' % ('stages', 'coded bpp', 'L1', 'PSNR', 'MS-SSIM'))
  for r in rows:
    print('%10d %10.5f %10.4f %10.3f %10.5f' % (r['stages'] // n, r['bpp'] / n, r['l1'] / n, r['psnr'] / n, r['ms_ssim'] / n))


def stage_lambda_grid(trainer, args, lambdas):
  """--vq-stages S with --vq-rate-lambda: the grid of (multiplier, stage prefix) against bpp and distortion --
  trainer.get_stage_curve(x, rate_lambda), batch means; the rows of lambda 0 are stage_curve_rows'.  Then the centres in use
  per stage (trainer.get_stage_usage, over all batches) and the entropy estimate of every stage (trainer.get_stage_rates)."""
  data = list(batches(args))
  print('%10s %10s %10s %10s %10s %10s' % ('lambda', 'stages', 'coded bpp', 'L1', 'PSNR', 'MS-SSIM'))
  for lam in lambdas:
    rows = None
    for x_dict in data:
      curve = trainer.get_stage_curve(x_dict, rate_lambda=lam, n_iter=args.vq_rate_iters)
      rows = curve if rows is None else [{k: a[k] + b[k] for k in a} for a, b in zip(rows, curve)]
    n = len(data)
    for r in rows:
      print('%10g %10d %10.5f %10.4f %10.3f %10.5f' % (lam, r['stages'] // n, r['bpp'] / n, r['l1'] / n, r['psnr'] / n,
                                                      r['ms_ssim'] / n))
  usage = sum(trainer.get_stage_usage(x_dict) for x_dict in data)
  rates = [sum(v) / len(data) for v in zip(*(trainer.get_stage_rates(x_dict) for x_dict in data))]
  print('%10s %16s %16s %14s' % ('stage', 'centres in use', 'dead in a group', 'entropy bpp'))
  for s in range(usage.shape[0]):
    used = int((usage[s].sum(0) > 0).sum())
    dead = int((usage[s] == 0).sum())
    print('%10d %10d / %-3d %16d %14.5f' % (s + 1, used, usage.shape[2], dead, rates[s]))


def class_stage_rows(trainer, args):
  """--vq-class-stages SPEC --per-class: the coded bpp (files of trainer.get_coded_rate) and the per-class L1 / PSNR
  of the SAME model under three depth maps -- the given one, uniform vq_stages and uniform 1 (the codec's table swapped between the
  calls; the books and every weight stay)."""
  from jpdse_hip import ops
  codec, S = trainer.model.codec, trainer.model.vq_stages
  given = codec.class_stages
  n = len(given[0])
  arms = (('map', given), ('uniform %d' % S, ((S,) * n, S)), ('uniform 1', ((1,) * n, 1)))
  bpp, sums, images = dict.fromkeys([a for a, _ in arms], 0.0), {}, 0
  try:
    for x_dict in batches(args):
      b = int(x_dict['image'].shape[0])
      images += b
      for name, cs in arms:
        codec.class_stages = cs
        bpp[name] += trainer.get_coded_rate(x_dict)[0] * b
        tab = trainer.get_eval_metrics(x_dict, per_class=True)['per_class']['raw'].sum(dim=0, keepdim=True)
        sums[name] = tab if name not in sums else sums[name] + tab
  finally:
    codec.class_stages = given      # whatever happened, the model leaves under its own table
  res = {name: ops.eval_metrics_per_class(sums[name]) for name, _ in arms}
  print('coded bpp (.jpdm files, %d images): ' % images + ', '.join('%s %.5f' % (name, bpp[name] / images) for name, _ in arms))
  print('{:>5} {:>6} {:>12}'.format('class', 'depth', 'pixels') + ''.join(' {:>14} {:>9}'.format(name + ' L1', 'PSNR dB') for name, _ in arms))
  first = res['map']
  for k in range(first['pixels'].numel()):
    if int(first['pixels'][k]):
      depth = given[0][k] if k < n else given[1]
      print('{:>5} {:>6} {:>12}'.format(k, depth, int(first['pixels'][k])) +
            ''.join(' {:>14.4f} {:>9.3f}'.format(float(res[name]['l1'][k]), float(res[name]['psnr'][k])) for name, _ in arms))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, default=4)
  ap.add_argument('--batch', type=int, default=2)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
  ap.add_argument('--ngf', type=int, default=64)
  ap.add_argument('--codec', action='store_true', help='learned codec (netE + binarizer): also report bpp')
  ap.add_argument('--encoder_quantizer', default='binarizer', choices=['binarizer', 's2hvq'],
                  help='with --codec: the encoder\'s bottleneck, as the training flag (DESIGN.md 4.15).  s2hvq reports the sizes of the '
                       '.jpdv blobs of the code (trainer.get_coded_rate) in place of the binarizer\'s Shannon / context figures')
  ap.add_argument('--vq_n_center', type=int, default=64, help='the training flag of the same name')
  ap.add_argument('--vq_center_size', type=int, default=8, help='the training flag of the same name')
  ap.add_argument('--vq_sigma', type=float, default=10.0, help='the training flag of the same name')
  ap.add_argument('--vq_context_coder', action='store_true',
                  help='with --codec --encoder_quantizer s2hvq: the training flag of the same name (DESIGN.md 4.19).  Also prints '
                       'the bpp of both forms of every code, .jpdv and .jpdw, and how many images took which container')
  ap.add_argument('--vq-rate-lambda', default=None, metavar='L0,L1,..',
                  help='with --codec --encoder_quantizer s2hvq: the rate-distortion curve of ONE model (DESIGN.md 4.22).  Prints one '
                       'row per multiplier -- the coded bpp of the files trainer.get_coded_ec writes and L1 / PSNR / MS-SSIM of '
                       'what a receiver decodes from that code -- and nothing else.  With --vq-stages S > 1 (DESIGN.md 4.25): the grid '
                       'of (multiplier, stage prefix), then the centres in use per stage')
  ap.add_argument('--vq-stages', type=int, default=1,
                  help='with --codec --encoder_quantizer s2hvq: code books of the residual bottleneck (opt.vq_stages, DESIGN.md 4.24).  '
                       'More than 1 prints the rate-distortion points of ONE stream cut after every stage (trainer.get_stage_curve)')
  ap.add_argument('--vq-class-stages', default=None, metavar='SPEC',
                  help="with --vq-stages S > 1 and --per-class: opt.vq_class_stages, e.g. '24:3,26:3,*:1' (DESIGN.md 4.27): bpp and the "
                       'per-class L1 / PSNR rows under the map, next to uniform S and uniform 1 of the same model')
  ap.add_argument('--vq-train-stages', default='all', choices=['all', 'uniform'], help='opt.vq_train_stages (DESIGN.md 4.24)')
  ap.add_argument('--vq-rate-iters', type=int, default=2, help='rounds of the entropy-constrained assignment per image')
  ap.add_argument('--checkpoints_dir', default=None, help='load net_G.pth (and net_E.pth) from here')
  ap.add_argument('--data', default=None, help='directory of pre-decoded *.pt batches instead of synthetic ones')
  ap.add_argument('--per-class', action='store_true', help='also print L1 / MSE / PSNR per semantic class')
  for flag in ('zero_sem', 'zero_ins', 'zero_vis'):
    ap.add_argument('--' + flag, action='store_true', help='ablation input of the reference (same flag)')
  ap.add_argument('--roundtrip', default=None, metavar='DIR',
                  help='with --codec: store every code under DIR, decode from the files, report the decoded images')
  ap.add_argument('--entropy', action='store_true',
                  help='with --codec: also report the bpp of the entropy-coded files; --roundtrip then stores and decodes those')
  ap.add_argument('--semantics', action='store_true',
                  help='with --codec --entropy --roundtrip: also store the label / instance maps as .jpds files and decode from files only')
  ap.add_argument('--rate-map', default=None, metavar='DIR',
                  help='with --codec: write every image\'s code-length map (bits per code cell, float64 [h, w]) as DIR/*.npy')
  ap.add_argument('--class_distortion_weights', default='',
                  help='label:weight pairs of the training flag (DESIGN.md 4.11): also print the weighted, un-quantised distortion')
  ap.add_argument('--edge_distortion_weight', type=float, default=1.0, help='the training flag of the same name (DESIGN.md 4.11)')
  args = ap.parse_args()
  if args.roundtrip and not args.codec:
    ap.error('--roundtrip needs --codec')
  if args.entropy and not args.codec:
    ap.error('--entropy needs --codec')
  if args.semantics and not (args.codec and args.entropy and args.roundtrip):
    ap.error('--semantics needs --codec --entropy --roundtrip DIR')
  if args.rate_map and not args.codec:
    ap.error('--rate-map needs --codec')
  vq = args.codec and args.encoder_quantizer == 's2hvq'
  if args.vq_context_coder and not vq:
    ap.error('--vq_context_coder needs --codec --encoder_quantizer s2hvq')
  lambdas = None
  if args.vq_rate_lambda is not None:
    if not vq:
      ap.error('--vq-rate-lambda needs --codec --encoder_quantizer s2hvq')
    try:
      lambdas = [float(v) for v in args.vq_rate_lambda.split(',')]
    except ValueError:
      ap.error('--vq-rate-lambda takes numbers separated by commas, e.g. 0,0.5,2,8')
  if args.vq_stages != 1 and not vq:
    ap.error('--vq-stages needs --codec --encoder_quantizer s2hvq')
  if args.vq_class_stages is not None and not (vq and args.vq_stages > 1 and args.per_class):
    ap.error('--vq-class-stages needs --codec --encoder_quantizer s2hvq --vq-stages S > 1 and --per-class')
  if vq and args.roundtrip:
    ap.error('--roundtrip stores the binarizer\'s code: not available with --encoder_quantizer s2hvq '
             '(trainer.get_coded / decode_coded are its files)')
  if args.roundtrip:
    os.makedirs(args.roundtrip, exist_ok=True)
  if args.rate_map:
    os.makedirs(args.rate_map, exist_ok=True)
  import jpdse_hip
  from jpdse_hip import ops
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  jpdse_hip.require_gpu(0)
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=args.dtype, ngf=args.ngf, batch_size=args.batch,
            zero_sem=args.zero_sem, zero_ins=args.zero_ins, zero_vis=args.zero_vis,
            class_distortion_weights=args.class_distortion_weights, edge_distortion_weight=args.edge_distortion_weight)
  if args.codec:
    kw.update(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=args.ngf, n_downsample_E=4,
              encoder_binarizer_out_channels=128, encoder_quantizer=args.encoder_quantizer, vq_n_center=args.vq_n_center,
              vq_center_size=args.vq_center_size, vq_sigma=args.vq_sigma, vq_context_coder=args.vq_context_coder)
  if args.checkpoints_dir:
    kw.update(is_train=False, load_model=True, checkpoints_dir=args.checkpoints_dir)
  opt = default_opt(**kw)
  if vq:      # fields without a training flag: set on the namespace
    opt.vq_stages, opt.vq_train_stages = args.vq_stages, args.vq_train_stages
    if args.vq_class_stages is not None:
      opt.vq_class_stages = args.vq_class_stages
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    trainer = get_trainer(opt)(opt, 'test' if args.checkpoints_dir else 'train')
  if args.vq_class_stages is not None:
    return class_stage_rows(trainer, args)
  if lambdas is not None and vq and args.vq_stages > 1:
    return stage_lambda_grid(trainer, args, lambdas)
  if lambdas is not None:
    return rate_lambda_rows(trainer, args, lambdas)
  if vq and args.vq_stages > 1:
    return stage_curve_rows(trainer, args)
  keys = ('l1', 'mse', 'ms_ssim', 'psnr')
  by_batch = dict.fromkeys(keys + ('shannon', 'actual', 'context', 'file', 'coded', 'semantics', 'total', 'weighted', 'model'), 0.0)
  by_image = dict.fromkeys(keys + ('shannon', 'actual', 'context', 'file', 'coded', 'semantics', 'total', 'weighted', 'model'), 0.0)
  weighted = trainer.model.sem_weights is not None      # class / edge weights are set
  images, n_batches, worst_diff = 0, 0, 0.0
  containers = {'jpdw': 0, 'jpdv': 0}                   # with --vq_context_coder: images whose kept blob is of that kind
  class_sums = None                  # int64 [1, n_classes + 1, 3]: the raw class tables of every image so far, added up
  class_bits = None                  # float64 [n_classes + 1]: the bits of the code attributed to each class so far (with --codec)
  start = time.time()
  for i, x_dict in enumerate(batches(args)):
    if args.roundtrip:
      code, file_bpp = roundtrip(trainer, x_dict, args.roundtrip, i, coded=args.entropy)
      receiver = dict(label=x_dict['label'], instance=x_dict['instance'])      # all the receiver has besides the files
      if args.semantics:
        receiver, sem_file_bpp = semantics_roundtrip(trainer, x_dict, args.roundtrip, i)     # ... unless the maps come from files too
      decoded = trainer.decode(code, receiver)
      diff = float((decoded - trainer.get_img(x_dict)).abs().max())
      worst_diff = max(worst_diff, diff)
      m = trainer.get_eval_metrics_decoded(code, x_dict, per_class=args.per_class)
    else:
      m = trainer.get_eval_metrics(x_dict, per_class=args.per_class)
    if args.per_class:
      tab = m['per_class']['raw'].sum(dim=0, keepdim=True)
      class_sums = tab if class_sums is None else class_sums + tab
    b = int(m['per_image']['l1'].numel())
    line = 'batch {}, recon loss (L1/MSE/MS-SSIM) {:.4f}/{:.4f}/{:.4f}, PSNR {:.3f} dB'.format(i + 1, m['l1'], m['mse'], m['ms_ssim'],
                                                                                         m['psnr'])
    if weighted:
      wd = trainer.get_weighted_distortion(x_dict)      # the training distortion under the weights: un-quantised, normalised scale
      by_batch['weighted'] += wd
      by_image['weighted'] += wd * b
      line += ', weighted {} (un-quantised) {:.6f}'.format(opt.distortion_loss_fn, wd)
    if vq:
      # the vector-quantised code: sizes of the .jpdv blobs and of the packed-index file, and a check that the
      # blobs decode to get_img's image
      coded_bpp, packed_bpp = trainer.get_coded_rate(x_dict)
      receiver = dict(label=x_dict['label'], instance=x_dict['instance'])
      diff = float((trainer.decode_coded(trainer.get_coded(x_dict), receiver) - trainer.get_img(x_dict)).abs().max())
      worst_diff = max(worst_diff, diff)
      by_batch['coded'] += coded_bpp
      by_image['coded'] += coded_bpp * b
      by_batch['actual'] += packed_bpp
      by_image['actual'] += packed_bpp * b
      line += ', vq code: coded file bpp {:.4f} (packed indices {:.4f}), max |decoded - get_img| {:.3e}'.format(coded_bpp, packed_bpp,
                                                                                                        diff)
      if args.vq_context_coder:
        # both forms of every code: the .jpdv blobs of a flag-off run, the .jpdw blobs whether or not they
        # are the smaller ones, and which container get_coded kept
        from ctu.utils import vqplane
        codec, pixels = trainer.model.codec, int(x_dict['image'].shape[-2]) * int(x_dict['image'].shape[-1])
        kept = trainer.get_coded(x_dict)
        codec.context_coder = False
        try:
          jpdv_bpp, _ = trainer.get_coded_rate(x_dict)
        finally:
          codec.context_coder = True
        code = trainer.get_vq_code(x_dict)
        _, ih, iw, _, n_center, groups = codec.geometry(x_dict, 'eval_rd')
        planes = [vqplane.write_planes(None, code[j], codec._planes(ih, iw, groups), n_center) for j in range(b)]
        jpdw_bpp = sum(8.0 * len(p) / pixels for p in planes) / b
        n_jpdw = sum(1 for blob in kept if blob[:4] == vqplane.MAGIC)
        containers['jpdw'] += n_jpdw
        containers['jpdv'] += b - n_jpdw
        line += ', .jpdv / .jpdw file bpp {:.4f}/{:.4f}, kept {} .jpdw and {} .jpdv'.format(jpdv_bpp, jpdw_bpp, n_jpdw, b - n_jpdw)
      # the per-group zero-order entropy of the same code over the batch: an estimate, not a size, and on
      # either side of the coded figure (the coder adapts per image and pays headers and flushes)
      line += ', per-group entropy bpp {:.4f}'.format(trainer.get_vq_rate(x_dict))
      # the centres each channel group's code uses at all: a count below n_center means dead centres
      used = (trainer.get_vq_usage(x_dict) > 0).sum(dim=1).tolist()
      line += ', centres in use per group {}'.format('/'.join(str(int(u)) for u in used))
    elif args.codec:
      shannon, actual = trainer.get_eval_rate(x_dict)
      shannon = float(shannon)
      by_batch['shannon'] += shannon
      by_batch['actual'] += actual
      by_image['shannon'] += shannon * b
      by_image['actual'] += actual * b
      line += ', pre-/(estimated) post-entropy coding bpp {:.4f}/{:.4f}'.format(actual, shannon)
      context = trainer.get_context_rate(x_dict)       # the context model's estimate, in bits (a lower bound
      by_batch['context'] += context                   # of the coded size, not a size)
      by_image['context'] += context * b
      line += ', context-model bpp {:.4f}'.format(context)
    if args.codec and args.per_class:
      # bits are sums of k / 2^16: adding batches stays exact
      cr = trainer.get_vq_class_rates(x_dict) if vq else trainer.get_class_rates(x_dict)
      class_bits = cr['bits'] if class_bits is None else class_bits + cr['bits']
    if args.rate_map:
      import numpy as np
      rm = trainer.get_vq_rate_map(x_dict) if vq else trainer.get_rate_map(x_dict)
      for j in range(b):
        np.save(os.path.join(args.rate_map, 'b%04d_i%02d.npy' % (i, j)), rm['map'][j].numpy())
      model_bpp = float(rm['bpp'].mean())
      by_batch['model'] += model_bpp
      by_image['model'] += float(rm['bpp'].sum())
      line += ', model code length bpp {:.4f}'.format(model_bpp)
    if args.entropy and not vq:
      coded_bpp, raw_file_bpp = trainer.get_coded_rate(x_dict)
      by_batch['coded'] += coded_bpp
      by_image['coded'] += coded_bpp * b
      line += ', coded file bpp {:.4f} (raw file {:.4f})'.format(coded_bpp, raw_file_bpp)
    if args.semantics:
      # trainer.get_total_rate's three figures, from the .jpda rate and the .jpds files already in hand
      code_bpp, sem_bpp = coded_bpp, sum(sem_file_bpp) / len(sem_file_bpp)
      total_bpp = code_bpp + sem_bpp
      by_batch['semantics'] += sem_bpp
      by_image['semantics'] += sem_bpp * b
      by_batch['total'] += total_bpp
      by_image['total'] += total_bpp * b
      line += ', code/semantics/total file bpp {:.4f}/{:.4f}/{:.4f}'.format(code_bpp, sem_bpp, total_bpp)
    if args.roundtrip:
      by_batch['file'] += sum(file_bpp) / len(file_bpp)
      by_image['file'] += sum(file_bpp)
      line += ', decoded from files: file bpp {:.4f}, max |decoded - get_img| {:.3e}'.format(sum(file_bpp) / len(file_bpp), diff)
    end = time.time()
    print(line + ', batch processing time (s) {:.4f}'.format(end - start))
    start = end
    for k in keys:
      by_batch[k] += m[k]
      by_image[k] += float(m['per_image'][k].sum())
    images += b
    n_batches += 1
  print('\ntest done!\n')

  def summary(head, t, n):
    line = '{} (L1/MSE/MS-SSIM) {:.4f}/{:.4f}/{:.4f}, avg PSNR {:.3f} dB'.format(head, t['l1'] / n, t['mse'] / n,
                                                                            t['ms_ssim'] / n, t['psnr'] / n)
    if weighted:
      line += ', avg weighted {} (un-quantised) {:.6f}'.format(opt.distortion_loss_fn, t['weighted'] / n)
    if vq:
      line += ', avg vq coded file / packed-index bpp {:.4f}/{:.4f}'.format(t['coded'] / n, t['actual'] / n)
    elif args.codec:
      line += ', avg pre-/(estimated) post-entropy coding bpp {:.4f}/{:.4f}'.format(t['actual'] / n, t['shannon'] / n)
      line += ', avg context-model bpp {:.4f}'.format(t['context'] / n)
    if args.rate_map:
      line += ', avg model code length bpp {:.4f}'.format(t['model'] / n)
    if args.entropy and not vq:
      line += ', avg coded file bpp {:.4f}'.format(t['coded'] / n)
    if args.semantics:
      line += ', avg semantics/total file bpp {:.4f}/{:.4f}'.format(t['semantics'] / n, t['total'] / n)
    if args.roundtrip:
      line += ', avg file bpp {:.4f}'.format(t['file'] / n)
    return line
  print('\n' + summary('test set avg recon loss', by_batch, n_batches))
  print(summary('per-image avg recon loss', by_image, images) + '\n')
  if args.vq_context_coder:
    print('context coder: {} of {} images kept the .jpdw container, {} the .jpdv one\n'.format(containers['jpdw'], images,
                                                                                             containers['jpdv']))
  if args.roundtrip:
    print('distortion above: images decoded from the files under %s; largest |decoded - get_img| over the test set %.3e\n'
          % (args.roundtrip, worst_diff))
  if args.per_class:
    r = ops.eval_metrics_per_class(class_sums)
    total = int(r['pixels'].sum()) + r['unlabelled']
    print('per-class distortion over the test set (classes that occur; %d pixels, %d without a class)' % (total, r['unlabelled']))
    rate_head = ' {:>12} {:>8} {:>9}'.format('bits', 'bpp', 'bit share') if class_bits is not None else ''
    print('{:>5} {:>12} {:>8} {:>9} {:>11} {:>9}'.format('class', 'pixels', 'share', 'L1', 'MSE', 'PSNR dB') + rate_head)
    all_bits = float(class_bits.sum()) if class_bits is not None else 0.0

    def rate_columns(k, n):
      if class_bits is None:
        return ''
      return ' {:>12.1f} {:>8.4f} {:>8.2f}%'.format(float(class_bits[k]), float(class_bits[k]) / n, 100.0 * float(class_bits[k]) / all_bits)
    for k in range(r['pixels'].numel()):
      n = int(r['pixels'][k])
      if n:
        print('{:>5} {:>12} {:>7.2f}% {:>9.4f} {:>11.4f} {:>9.3f}'.format(k, n, 100.0 * n / total, float(r['l1'][k]),
                                                                      float(r['mse'][k]), float(r['psnr'][k])) + rate_columns(k, n))
    if class_bits is not None and r['unlabelled']:
      print('{:>5} {:>12} {:>7.2f}% {:>9} {:>11} {:>9}'.format('none', r['unlabelled'], 100.0 * r['unlabelled'] / total, '', '', '')
            + rate_columns(-1, r['unlabelled']))
    if class_bits is not None:
      print('bits: the code length under the coder\'s own adaptive model (DESIGN.md %s), %.1f in all, %.4f bpp'
            % ('4.20' if vq else '4.12', all_bits, all_bits / total))
    print('')


if __name__ == '__main__':
  main()
