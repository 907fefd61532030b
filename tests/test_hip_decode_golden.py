"""GPU: the receiver of the learned codec -- ops.code_import, Encoder.decode_code, trainer.decode and
trainer.get_eval_metrics_decoded -- on the networks of tests/golden/learned_codec_nef8.npz (recorded from the reference:
batch 2, 64x128, nef 8 / n_downsample_E 4 / B 32 / feat_num 3, G ngf 8 with one ResnetBlock).

The encoder's second half is tied to the reference's own features through the fixture's code; everything else is an
equality with the sender-side calls of the same trainer (get_img, get_eval_metrics), bit for bit, under the zero rule:
an exact zero of the eval code is stored as a 0 bit and decoded as -1."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import code_import_ref as cref  # noqa: E402
import test_hip_learned_codec_golden as tg  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402

NET_TOL = tg.NET_TOL      # 2e-4 of the reference's largest magnitude: the bound the whole encoder is held to there


@pytest.fixture(scope='module')
def gold(golden_dir):
  z = np.load(os.path.join(golden_dir, 'learned_codec_nef8.npz'))
  return {k: z[k] for k in z.files}


def _same(a, b):
  """torch.equal that takes nan (the PSNR of an absent class) as equal to nan."""
  return torch.equal(a.double().nan_to_num(nan=-1.0), b.double().nan_to_num(nan=-1.0))


def _receiver(xd):
  """What the receiver has: the semantics.  No 'image', no 'compressed_img'."""
  return dict(label=xd['label'].clone(), instance=xd['instance'].clone())


def _no_zero(te, xd):
  """The stated precondition of every equality below: the eval code of xd holds no exact zero."""
  from jpdse_hip import ops
  with torch.no_grad():
    te.eval()
    zeros = ops.code_stats(te.model._code_act(xd))[:, 1]
  return bool((zeros == 0).all())


def _flag_trainer(gold, dtype='fp32', **flags):
  """A train-mode trainer on the fixture's weights with extra flags (the ablation inputs)."""
  from ctu.trainers import get_trainer
  opt = tg._opt(dtype, **flags)
  tr = get_trainer(opt)(opt, 'train')
  sd_G, sd_D, sd_E = tg._weights(gold)
  tr.model.netG.load_state_dict(sd_G)
  tr.model.netD.load_state_dict(sd_D)
  tr.model.netE.load_state_dict(sd_E)
  return tr


def test_second_half_of_the_encoder_against_the_reference_features(gold, tmp_path):
  """The reference's own eval code, as the fp32 code (code + 1) / 2, through ops.code_import and Encoder.decode_code:
  image 0's features against the reference's, without the encoder's front half in between."""
  from jpdse_hip import ops, F32
  te = tg._test_trainer(gold, tmp_path)
  code = torch.from_numpy(gold['eval_code']).float()
  N, C, h, w = code.shape
  assert (C, h, w) == te.model.netE.code_shape(int(gold['height']), int(gold['width'])) == (32, 4, 8)
  assert bool((code.abs() == 1).all())
  flat = ((code.reshape(N, -1) + 1) / 2).contiguous()
  with torch.no_grad():
    b = ops.code_import(flat.cuda(), N, h, w, C, F32)
    assert torch.equal(ops.nhwc_to_nchw(b).cpu(), code)
    feat = ops.nhwc_to_nchw(te.model.netE.decode_code(b))[0].cpu().double()
  ref = torch.from_numpy(gold['eval_feat0']).double()
  err, bound = (feat - ref).abs().max().item(), NET_TOL * ref.abs().max().item()
  print('decode_code vs reference features: max abs error %.3e, bound %.3e' % (err, bound))
  assert err <= bound


# bf16: the fixture's own batch (img_seed of the golden file) was measured free of exact zeros on the MI355X, so no other
# synthetic_batch seed had to be picked
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_decode_equals_get_img_bit_for_bit(gold, tmp_path, dtype):
  te = tg._test_trainer(gold, tmp_path, dtype)
  xd = tg._batch(gold)
  assert _no_zero(te, xd), 'precondition: the eval code of this batch holds an exact zero'
  want = te.get_img(xd)
  packed = te.get_code(xd, packed=True)
  plain = te.get_code(xd)
  assert packed.dtype == torch.uint8 and tuple(packed.shape) == (2, 128) and tuple(plain.shape) == (2, 1024)
  rx = _receiver(xd)
  got = te.decode(packed, rx)
  assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device
  assert torch.equal(got, want)
  assert torch.equal(te.decode(plain, rx), want)
  # from the host, as a stored code arrives
  assert torch.equal(te.decode(packed.cpu(), rx), want)
  assert torch.equal(te.decode(plain.cpu(), rx), want)
  # and the stored bits are the yardstick's
  assert np.array_equal(cref.import_packed(packed.cpu().numpy(), 2, 32, 4, 8).reshape(2, -1) * 0.5 + 0.5, plain.cpu().numpy())


def test_an_exact_zero_is_decoded_as_minus_one(gold, tmp_path):
  """The zero rule on a code with forced zeros: exported, a zero is a 0 bit (0.5 in the fp32 form); imported, it is -1, and
  decode reconstructs from -1 -- not from the 0 the sender's own forward pass would use."""
  from jpdse_hip import ops
  te = tg._test_trainer(gold, tmp_path)
  xd = tg._batch(gold)
  rx = _receiver(xd)
  with torch.no_grad():
    te.eval()
    b = te.model._code_act(xd)
    assert int(ops.code_stats(b)[:, 1].sum()) == 0
    # force the first three +1 entries of image 0 and one of image 1 to the exact-zero case
    hit = torch.zeros_like(b.t, dtype=torch.bool)
    for n, count in ((0, 3), (1, 1)):
      idx = (b.t[n] > 0).nonzero()[:count]
      hit[n][tuple(idx.t())] = True
    assert int(hit.sum()) == 4
    b0 = ops.Act(torch.where(hit, torch.zeros_like(b.t), b.t), b.C)
    bm = ops.Act(torch.where(hit, -torch.ones_like(b.t), b.t), b.C)
    assert ops.code_stats(b0)[:, 1].tolist() == [3, 1]
    for packed in (True, False):
      c0, cm = ops.code_export(b0, packed), ops.code_export(bm, packed)
      if packed:
        assert torch.equal(c0, cm)                           # a zero and a -1 are the same stored bit
      else:
        assert int((c0 == 0.5).sum()) == 4 and int((cm == 0.5).sum()) == 0
      back = ops.code_import(c0, b.N, b.H, b.W, b.C, b.dtype)
      assert torch.equal(back.t, bm.t)
      img = te.decode(c0, rx)
      assert torch.equal(img, te.decode(cm, rx))
      assert not torch.equal(img, te.get_img(xd))            # four bits differ from the unforced code
    # the sender's view of the same tensor (0 fed forward) is a different set of features
    f_zero = te.model.netE.decode_code(b0).t
    f_minus = te.model.netE.decode_code(bm).t
    assert not torch.equal(f_zero, f_minus)


@pytest.mark.parametrize('per_class', [False, True], ids=['plain', 'per_class'])
def test_decoded_metrics_equal_the_sender_side_metrics(gold, tmp_path, per_class):
  """192x192: the smallest multiple of the encoder's factor 16 at which MS-SSIM's fifth scale exists (176)."""
  te = tg._test_trainer(gold, tmp_path)
  xd = omodel.synthetic_batch(2, 192, 192, seed=61)
  assert _no_zero(te, xd), 'precondition: the eval code of this batch holds an exact zero'
  want = te.get_eval_metrics(xd, per_class=per_class)
  got = te.get_eval_metrics_decoded(te.get_code(xd, packed=True).cpu(), xd, per_class=per_class)
  assert set(got) == set(want) and tuple(want['raw'].shape) == (2, 14)
  assert torch.equal(got['raw'], want['raw'])
  for k in ('l1', 'mse', 'psnr', 'ms_ssim'):
    assert got[k] == want[k], k
    assert torch.equal(got['per_image'][k], want['per_image'][k]), k
  assert ('per_class' in got) == per_class
  if per_class:
    a, b = got['per_class'], want['per_class']
    assert set(a) == set(b) and torch.equal(a['raw'], b['raw']) and a['unlabelled'] == b['unlabelled']
    for k in ('pixels', 'l1', 'mse', 'psnr'):
      assert _same(a[k], b[k]) and _same(a['per_image'][k], b['per_image'][k]), k
  # the fp32 code gives the same table
  again = te.get_eval_metrics_decoded(te.get_code(xd), xd, per_class=per_class)
  assert torch.equal(again['raw'], want['raw'])


@pytest.mark.parametrize('flag', ['zero_sem', 'zero_ins', 'zero_vis'])
def test_decode_builds_the_ablation_inputs_as_get_img_does(gold, flag):
  tr = _flag_trainer(gold, **{flag: True})
  xd = tg._batch(gold)
  assert _no_zero(tr, xd), 'precondition: the eval code of this batch holds an exact zero'
  want = tr.get_img(xd)
  rx = _receiver(xd)
  code = tr.get_code(xd, packed=True)
  assert torch.equal(tr.decode(code, rx), want)
  plain = _flag_trainer(gold).get_img(xd)
  assert not torch.equal(plain, want)                        # the flag is a different computation
  if flag == 'zero_vis':
    assert torch.equal(tr.decode(torch.full_like(code, 0xff), rx), want)       # the code is ignored ...
    assert torch.equal(tr.decode(torch.ones(2, 1024), rx), want)
    with pytest.raises(ValueError, match='decode'):
      tr.decode(code[:, :-1], rx)                            # ... but still has to be a code of this label map
  else:
    assert not torch.equal(tr.decode(torch.full_like(code, 0xff), rx), want)


def test_refusals(gold, tmp_path):
  from ctu.trainers import get_trainer
  xd = tg._batch(gold)
  rx = _receiver(xd)
  code = torch.zeros(2, 128, dtype=torch.uint8)
  for over in (dict(no_encoder_binarization=True), dict(no_feat_encoding=True)):
    opt = tg._opt(**over)
    tr = get_trainer(opt)(opt, 'train')
    with pytest.raises(ValueError, match='binary codes need the learned codec with encoder binarization'):
      tr.decode(code, rx)
    with pytest.raises(ValueError, match='binary codes need the learned codec with encoder binarization'):
      tr.get_eval_metrics_decoded(code, xd)
  te = tg._test_trainer(gold, tmp_path)
  good = te.get_code(xd, packed=True)
  for bad in (good[:, :-1], good[:1], good.cpu()[:, :-1], te.get_code(xd)[:, :-1], good.to(torch.int32), good.reshape(-1)):
    with pytest.raises(ValueError, match='decode'):
      te.decode(bad, rx)
  with pytest.raises(ValueError, match='decode'):
    te.decode(good, dict(label=xd['label'][..., :120], instance=xd['instance'][..., :120]))    # 120 is no multiple of 16
  assert torch.equal(te.decode(good, rx), te.get_img(xd))    # and the trainer is still usable
