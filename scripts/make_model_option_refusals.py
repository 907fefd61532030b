"""Pin what the model's constructor refuses, in which order, and the flag table it parses: writes
tests/golden/model_option_refusals.json, a list of [case id, exception type, full message], and
tests/golden/model_option_table.json, a list of [dest, option strings, action, type, default, choices, help] per flag.  No GPU:
torch.cuda.is_available answers False and the library loader raises AssertionError('library touched'), so a configuration that
passes every check ends at the constructor's device check, JpdseError('... no GPU visible ...'), before any network exists; a
check that moved behind network construction, or in front of another check, shows as a changed row.

The cases: every member of the NotImplementedError list alone and three at once (the joined message); every ValueError in front
of network construction -- distortion_loss_fn, lambda_rate, lambda_vq_rate, vq_context_coder, encoder_quantizer and the
bottleneck's own check, class_distortion_weights, edge_distortion_weight, the ms_ssim conflict -- with negative, NaN and infinite
weights; pairs of broken rules whose first message pins the order of the checks; and the configurations that pass, None values
for the flags whose code tolerates None among them.

Both committed fixtures were generated on the parent commit of the model's split into model_options / coded_calls /
pix2pixHD_model -- this script runs on either layout of the model -- and are replayed by tests/test_model_option_refusals.py;
regenerate them only for a deliberate change of a flag or a message, never to make that test pass.

  python scripts/make_model_option_refusals.py [--out tests/golden/model_option_refusals.json] [--table tests/golden/model_option_table.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402

NAN, INF = float('nan'), float('inf')
NET = dict(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1)
CODEC = dict(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=2,
             encoder_binarizer_out_channels=16)
S2HVQ = dict(CODEC, encoder_quantizer='s2hvq', vq_n_center=8, vq_center_size=4)


def cases():
  """[(case id, option overrides)] on top of NET."""
  out = []
  add = lambda cid, *dicts: out.append((cid, {k: v for d in dicts for k, v in d.items()}))
  # ---- the NotImplementedError list: each member alone, then three at once
  add('unsupported/label-encoder', dict(no_label_encoding=False))
  add('unsupported/generator-binarization', dict(no_generator_binarization=False))
  add('unsupported/encoder-netG-local', CODEC, dict(netG='local'))
  add('unsupported/encoder-netE_groups-2', CODEC, dict(netE_groups=2))
  add('unsupported/encoder-n_downsample_E-0', CODEC, dict(n_downsample_E=0))
  add('unsupported/encoder-pool_size-4', CODEC, dict(pool_size=4))
  for flag in ('sem_masking', 'no_label', 'no_feat', 'match_raw_feat', 'no_lsgan', 'use_netE_output', 'binary_mask', 'inst_wise_pool'):
    add('unsupported/' + flag, {flag: True})
  add('unsupported/norm-batch', dict(norm='batch'))
  add('unsupported/three-at-once', CODEC, dict(no_label_encoding=False, netE_groups=4, norm='batch'))
  add('unsupported/no-encoder-ignores-encoder-flags', dict(netG='local', netE_groups=2, n_downsample_E=0))      # passes
  # ---- distortion_loss_fn
  add('distortion_loss_fn/huber', dict(distortion_loss_fn='huber'))
  add('distortion_loss_fn/none', dict(distortion_loss_fn=None))
  # ---- lambda_rate
  for name, v in (('negative', -0.5), ('nan', NAN), ('inf', INF), ('text', 'much')):
    add('lambda_rate/' + name, dict(lambda_rate=v))
    add('lambda_rate/%s/binarizer' % name, CODEC, dict(lambda_rate=v))
  add('lambda_rate/positive/no_feat_encoding', CODEC, dict(lambda_rate=0.5, no_feat_encoding=True))
  add('lambda_rate/positive/no_encoder_binarization', CODEC, dict(lambda_rate=0.5, no_encoder_binarization=True))
  add('lambda_rate/positive/zero_vis', CODEC, dict(lambda_rate=0.5, zero_vis=True))
  # ---- lambda_vq_rate
  for name, v in (('negative', -0.5), ('nan', NAN), ('inf', INF), ('text', 'much')):
    add('lambda_vq_rate/' + name, dict(lambda_vq_rate=v))
    add('lambda_vq_rate/%s/s2hvq' % name, S2HVQ, dict(lambda_vq_rate=v))
  add('lambda_vq_rate/positive/no-encoder', dict(lambda_vq_rate=0.5))
  add('lambda_vq_rate/positive/binarizer', CODEC, dict(lambda_vq_rate=0.5))
  add('lambda_vq_rate/positive/s2hvq-zero_vis', S2HVQ, dict(lambda_vq_rate=0.5, zero_vis=True))
  # ---- vq_context_coder
  add('vq_context_coder/no-encoder', dict(vq_context_coder=True))
  add('vq_context_coder/binarizer', CODEC, dict(vq_context_coder=True))
  # ---- encoder_quantizer and the bottleneck's check
  add('encoder_quantizer/lattice', CODEC, dict(encoder_quantizer='lattice'))
  add('encoder_quantizer/none', CODEC, dict(encoder_quantizer=None))
  add('s2hvq/no_feat_encoding', S2HVQ, dict(no_feat_encoding=True))
  add('s2hvq/no_encoder_binarization', S2HVQ, dict(no_encoder_binarization=True))
  add('s2hvq/lambda_rate', S2HVQ, dict(lambda_rate=0.5))
  add('s2hvq/vq_center_size-3', S2HVQ, dict(vq_center_size=3))
  add('s2hvq/vq_center_size-0', S2HVQ, dict(vq_center_size=0))
  add('s2hvq/channels-12', S2HVQ, dict(encoder_binarizer_out_channels=12))
  add('s2hvq/vq_n_center-1', S2HVQ, dict(vq_n_center=1))
  add('s2hvq/vq_n_center-513', S2HVQ, dict(vq_n_center=513))
  add('s2hvq/vq_center_size-64', S2HVQ, dict(vq_center_size=64, encoder_binarizer_out_channels=64))
  add('s2hvq/vq_sigma-0', S2HVQ, dict(vq_sigma=0.0))
  add('s2hvq/vq_sigma-nan', S2HVQ, dict(vq_sigma=NAN))
  add('s2hvq/vq_sigma-inf', S2HVQ, dict(vq_sigma=INF))
  # ---- class_distortion_weights: every malformed form of parse_class_distortion_weights
  for name, text in (('no-colon', '24'), ('two-colons', '24:4:1'), ('empty-pair', '24:4,,26:2'), ('label-word', 'road:4'),
                     ('label-fraction', '2.5:4'), ('weight-word', '24:heavy'), ('weight-negative', '24:-1'), ('weight-nan', '24:nan'),
                     ('weight-inf', '24:inf'), ('label-negative', '-1:2'), ('label-35', '35:2'), ('label-twice', '24:4,24:2')):
    add('class_distortion_weights/' + name, dict(class_distortion_weights=text))
  add('class_distortion_weights/label-35-with-dontcare', dict(class_distortion_weights='35:2', contain_dontcare_label=True))   # passes
  add('class_distortion_weights/label-36-with-dontcare', dict(class_distortion_weights='36:2', contain_dontcare_label=True))
  add('class_distortion_weights/label-256-of-300', dict(class_distortion_weights='256:2', num_labels=300))
  # ---- edge_distortion_weight, and the ms_ssim conflict
  for name, v in (('negative', -0.5), ('nan', NAN), ('inf', INF), ('text', 'sharp')):
    add('edge_distortion_weight/' + name, dict(edge_distortion_weight=v))
  add('edge_distortion_weight/3-no_instance', dict(edge_distortion_weight=3.0, no_instance=True))
  add('edge_distortion_weight/0-no_instance', dict(edge_distortion_weight=0.0, no_instance=True))
  add('ms_ssim/class-weights', dict(class_distortion_weights='24:4', distortion_loss_fn='ms_ssim'))
  add('ms_ssim/edge-weight', dict(edge_distortion_weight=2.0, distortion_loss_fn='ms_ssim'))
  # ---- order: two broken rules, the first message tells which check comes first
  add('order/unsupported+distortion_loss_fn', dict(sem_masking=True, distortion_loss_fn='huber'))
  add('order/unsupported+lambda_rate', dict(norm='batch', lambda_rate=-1.0))
  add('order/distortion_loss_fn+lambda_rate', dict(distortion_loss_fn='huber', lambda_rate=-1.0))
  add('order/lambda_rate-negative+lambda_vq_rate-negative', dict(lambda_rate=-1.0, lambda_vq_rate=-1.0))
  add('order/lambda_rate-positive+lambda_vq_rate-negative', dict(lambda_rate=0.5, lambda_vq_rate=-1.0))
  add('order/lambda_vq_rate-negative+vq_context_coder', dict(lambda_vq_rate=-1.0, vq_context_coder=True))
  add('order/lambda_vq_rate-positive+vq_context_coder', dict(lambda_vq_rate=0.5, vq_context_coder=True))
  add('order/lambda_vq_rate-positive+encoder_quantizer', CODEC, dict(lambda_vq_rate=0.5, encoder_quantizer='lattice'))
  add('order/vq_context_coder+encoder_quantizer', CODEC, dict(vq_context_coder=True, encoder_quantizer='lattice'))
  add('order/encoder_quantizer+class-weights', CODEC, dict(encoder_quantizer='lattice', class_distortion_weights='24'))
  add('order/s2hvq-no_feat_encoding+lambda_rate', S2HVQ, dict(no_feat_encoding=True, lambda_rate=0.5))
  add('order/s2hvq-no_encoder_binarization+center_size', S2HVQ, dict(no_encoder_binarization=True, vq_center_size=3))
  add('order/s2hvq-lambda_rate+center_size', S2HVQ, dict(lambda_rate=0.5, vq_center_size=3))
  add('order/s2hvq-center_size+sigma', S2HVQ, dict(vq_center_size=3, vq_sigma=0.0))
  add('order/s2hvq-center_size+class-weights', S2HVQ, dict(vq_center_size=3, class_distortion_weights='24'))
  add('order/class-weights+edge-weight', dict(class_distortion_weights='24', edge_distortion_weight=-1.0))
  add('order/edge-weight-negative+no_instance', dict(edge_distortion_weight=-1.0, no_instance=True))
  add('order/edge-weight-no_instance+ms_ssim', dict(edge_distortion_weight=3.0, no_instance=True, distortion_loss_fn='ms_ssim'))
  add('order/lambda_rate+ms_ssim-weights', dict(lambda_rate=-1.0, class_distortion_weights='24:4', distortion_loss_fn='ms_ssim'))
  # ---- configurations that pass every check: they end at the device check
  add('passes/defaults')
  add('passes/binarizer', CODEC)
  add('passes/binarizer-lambda_rate', CODEC, dict(lambda_rate=0.5))
  add('passes/s2hvq', S2HVQ)
  add('passes/s2hvq-rate-and-context-coder', S2HVQ, dict(lambda_vq_rate=0.5, vq_context_coder=True, vq_soft_forward=True))
  add('passes/encoder-without-bottleneck', CODEC, dict(no_encoder_binarization=True))
  add('passes/class-weights-all-ones', dict(class_distortion_weights='0:1,34:1.0'))
  add('passes/class-weights', dict(class_distortion_weights='24:4,26:2', edge_distortion_weight=3.0, distortion_loss_fn='mse'))
  add('passes/ones-with-ms_ssim', dict(class_distortion_weights='3:1', edge_distortion_weight=1.0, distortion_loss_fn='ms_ssim'))
  add('passes/edge-1-no_instance', dict(edge_distortion_weight=1.0, no_instance=True))
  add('passes/none-values', S2HVQ, dict(lambda_rate=None, lambda_vq_rate=None, edge_distortion_weight=None,
                                        class_distortion_weights=None, seed=None, vq_context_coder=None, compute_dtype=None))
  add('passes/lambda_vq_rate-false', dict(lambda_vq_rate=False, lambda_rate=False))
  add('passes/zero-flags-bf16', dict(zero_vis=True, zero_sem=True, zero_ins=True, no_instance=True, contain_dontcare_label=True,
                                     compute_dtype='bf16'))
  return out


def hidden_device():
  """Context: no GPU visible, and every way to the library raises AssertionError('library touched')."""
  import contextlib
  import jpdse_hip
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401,F401

  @contextlib.contextmanager
  def ctx():
    saved = torch.cuda.is_available, jpdse_hip.lib, jpdse_hip.ops.lib
    touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
    torch.cuda.is_available, jpdse_hip.lib, jpdse_hip.ops.lib = (lambda: False), touched, touched
    try:
      yield
    finally:
      torch.cuda.is_available, jpdse_hip.lib, jpdse_hip.ops.lib = saved
  return ctx()


def run():
  """[[case id, exception type, message]] on the code this file sits beside; 'returned' for a constructor that raised nothing."""
  from oracle.ctu_cpu import model as omodel
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  rows = []
  with hidden_device():
    for cid, over in cases():
      try:
        Pix2PixHDModel(omodel.default_opt(**dict(NET, **over)))
        rows.append([cid, 'returned', ''])
      except Exception as e:      # every outcome is a row
        rows.append([cid, type(e).__name__, str(e)])
  return rows


def flag_table(setter):
  """[[dest, option strings, action, type, default, choices, help]] of the parser `setter(parser, train)` fills, for train True
  and False (one table each, in the parser's order)."""
  tables = []
  for train in (True, False):
    parser = argparse.ArgumentParser(add_help=False)
    setter(parser, train)
    tables.append([[a.dest, list(a.option_strings), type(a).__name__, a.type.__name__ if a.type is not None else None, a.default,
                    list(a.choices) if a.choices is not None else None, a.help] for a in parser._actions])
  return tables


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'model_option_refusals.json'))
  ap.add_argument('--table', default=os.path.join(ROOT, 'tests', 'golden', 'model_option_table.json'))
  args = ap.parse_args()
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  table = flag_table(Pix2PixHDModel.modify_commandline_options)
  with open(args.table, 'w') as f:
    json.dump(table, f, indent=0)
    f.write('\n')
  rows = run()
  with open(args.out, 'w') as f:
    json.dump(rows, f, indent=0)
    f.write('\n')
  kinds = {}
  for _, kind, _ in rows:
    kinds[kind] = kinds.get(kind, 0) + 1
  print('%d flags -> %s' % (len(table[0]), args.table))
  print('%d cases -> %s (%s)' % (len(rows), args.out, ', '.join('%s: %d' % kv for kv in sorted(kinds.items()))))


if __name__ == '__main__':
  main()
