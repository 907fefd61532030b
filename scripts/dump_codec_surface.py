"""Dump what the codec surface of the trainer computes, as hashes: one JSON file of the sha256 of the bytes of every public
call's result, for comparing two commits bit for bit (needs a GPU).  The configuration is the smallest one the codec tests use
(ngf 8, nef 8, n_downsample_E 2, 16 bottleneck channels, 8 centres of size 4), the input a seeded batch of 2 at 64 x 32, in
fp32 and bf16, for the binarizer and for S2HVQ with the hard and the soft training forward; S2HVQ also under --zero_vis and
--zero_sem.  Per case: get_img, get_code (both forms), get_vq_code, get_vq_rate, get_context_rate, get_eval_rate, get_rate_map,
get_class_rates, get_coded, get_coded_rate, get_total_rate, and decode, get_eval_metrics_decoded, decode_coded and
decode_from_files of the call's own outputs (get_eval_metrics_decoded, which refuses a side under 176, also on one 192 x 192
image); a call the quantizer does not serve is recorded by its exception, as is decode of
an index outside the code book.  Then two train steps with the quantizer's rate term at weight 0.5 (--lambda_rate /
--lambda_vq_rate): the loss dict of each and a hash over all netE and netG parameters.

  python scripts/dump_codec_surface.py --out surface.json      # twice on one commit shows what, if anything, does not repeat
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402

from ctu.utils.synthetic import synthetic_batch  # noqa: E402

N, H, W, C, D, L, DOWN = 2, 64, 32, 16, 4, 8, 2
QUANTIZERS = {'binarizer': dict(encoder_quantizer='binarizer'), 's2hvq-hard': dict(encoder_quantizer='s2hvq'),
              's2hvq-soft': dict(encoder_quantizer='s2hvq', vq_soft_forward=True)}
RATE_OPTION = {'binarizer': 'lambda_rate', 's2hvq-hard': 'lambda_vq_rate', 's2hvq-soft': 'lambda_vq_rate'}


def digest(value):
  """The sha256 of a tensor's bytes (with its dtype and shape), the repr of a number, and the same through lists and dicts."""
  if torch.is_tensor(value):
    t = value.detach().cpu().contiguous()
    raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
    return '%s%s:%s' % (str(t.dtype).replace('torch.', ''), list(t.shape), hashlib.sha256(raw).hexdigest())
  if isinstance(value, (bytes, bytearray)):
    return 'bytes[%d]:%s' % (len(value), hashlib.sha256(bytes(value)).hexdigest())
  if isinstance(value, dict):
    return {str(k): digest(v) for k, v in value.items()}
  if isinstance(value, (list, tuple)):
    return [digest(v) for v in value]
  return repr(value)


def attempt(fn):
  try:
    return digest(fn())
  except Exception as e:      # a call this quantizer does not serve: its refusal is the result
    return 'raised %s: %s' % (type(e).__name__, e)


def trainer(dtype, **over):
  from ctu.trainers import get_trainer
  from ctu.utils.synthetic import default_opt
  kw = dict(gpu_ids=[0], print_losses=False, compute_dtype=dtype, ngf=8, ndf=8, n_blocks_global=1, n_downsample_global=2,
            no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=DOWN,
            encoder_binarizer_out_channels=C, vq_n_center=L, vq_center_size=D, vq_sigma=10.0, seed=20261020,
            no_vgg_loss=True, no_gan_feat_loss=True, no_g_gan_loss=True, no_d_gan_loss=True, skip_unused_losses=True)
  kw.update(over)
  opt = default_opt(**kw)
  torch.manual_seed(1234)
  with contextlib.redirect_stdout(sys.stderr):
    tr = get_trainer(opt)(opt, 'train')
  if tr.model.netE._vq is not None:      # a code book at the scale of the bottleneck's features: more than one centre in use
    with torch.no_grad():
      tr.model.netE._vq.vq._code_book.mul_(0.05)
  return tr


def surface(tr, xd):
  receiver = dict(label=xd['label'], instance=xd['instance'])
  out = {}
  for name in ('get_img', 'get_vq_code', 'get_vq_rate', 'get_context_rate', 'get_eval_rate', 'get_rate_map', 'get_class_rates',
               'get_coded', 'get_coded_rate', 'get_total_rate', 'get_code'):
    out[name] = attempt(lambda: getattr(tr, name)(xd))
  out['get_code packed'] = attempt(lambda: tr.get_code(xd, packed=True))
  codes = {}
  with contextlib.suppress(ValueError):
    codes['get_code'] = tr.get_code(xd)
    codes['get_code packed'] = tr.get_code(xd, packed=True)
  with contextlib.suppress(ValueError):
    codes['get_vq_code'] = tr.get_vq_code(xd)
    codes['get_vq_code on the host, int32'] = codes['get_vq_code'].cpu().to(torch.int32)
    bad = codes['get_vq_code'].clone()
    bad[1, 7] = L
    codes['an index outside the book'] = bad
    far = codes['get_vq_code'].clone()
    far[0, 0] = -1 - (1 << 32)
    codes['an index that int32 would fold into range'] = far
  for cid, code in codes.items():
    out['decode(%s)' % cid] = attempt(lambda: tr.decode(code, receiver))
    out['get_eval_metrics_decoded(%s)' % cid] = attempt(lambda: tr.get_eval_metrics_decoded(code, xd, per_class=True))
  # get_eval_metrics_decoded refuses 64 x 32 (MS-SSIM needs a shorter side of 176): its figures come from one 192 x 192 image
  big = synthetic_batch(1, 192, 192, seed=5)
  for cid, get in (('get_code packed', lambda: tr.get_code(big, packed=True)), ('get_vq_code', lambda: tr.get_vq_code(big))):
    with contextlib.suppress(ValueError):
      code = get()
      out['get_eval_metrics_decoded(%s) at 192 x 192' % cid] = attempt(lambda: tr.get_eval_metrics_decoded(code, big, per_class=True))
  coded = tr.get_coded(xd)
  out['decode_coded(get_coded)'] = attempt(lambda: tr.decode_coded(coded, receiver))
  out['decode_from_files'] = attempt(lambda: tr.decode_from_files(coded, tr.get_coded_semantics(xd)))
  return out


def train(tr, xd):
  out = {}
  for step in (1, 2):
    tr.step(xd)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for net in (tr.model.netE, tr.model.netG):
      for k, p in net.state_dict().items():
        h.update(k.encode())
        h.update(p.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    out['step %d' % step] = dict(losses={k: repr(v) for k, v in tr.last_losses.items()}, netE_netG=h.hexdigest())
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', required=True)
  args = ap.parse_args()
  import jpdse_hip
  jpdse_hip.require_gpu(0)
  xd = synthetic_batch(N, H, W, seed=3)
  result = {}
  for dtype in ('fp32', 'bf16'):
    for qname, q in QUANTIZERS.items():
      variants = [('', {})]
      if qname == 's2hvq-hard':
        variants += [(' --zero_vis', dict(zero_vis=True)), (' --zero_sem', dict(zero_sem=True))]
      for vname, v in variants:
        result['%s %s%s' % (dtype, qname, vname)] = surface(trainer(dtype, **q, **v), xd)
      result['%s %s train, %s 0.5' % (dtype, qname, RATE_OPTION[qname])] = train(trainer(dtype, **q, **{RATE_OPTION[qname]: 0.5}), xd)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print('%d cases, %d entries -> %s' % (len(result), sum(len(v) for v in result.values()), args.out))


if __name__ == '__main__':
  main()
