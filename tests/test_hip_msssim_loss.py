"""GPU tests of the MS-SSIM training loss (jpdse_msssim_loss through ops.msssim_loss_fwd / _fwd_bwd, and
--distortion_loss_fn ms_ssim in the trainer).  Definition and measured figures: DESIGN.md 4.6.

Yardstick: tests/msssim_loss_ref.py, torch float64 on the CPU, 2-D F.conv2d, gradient from autograd (no code shared with the
kernel), evaluated on the values the device sees (the bf16-rounded images for a bf16 case).
  loss value    |kernel - fp64| <= 2 x |plain fp32 torch-CPU evaluation of the definition - fp64| on the same batch
  gradient fp32 max |g - g64| <= 1e-3 max |g64|                       (the project's fp32 contract)
  gradient bf16 |g - g64| <= 1e-3 max |g64| + 2^-8 |g64| per element  (the fp32 bound + one bf16 rounding of the stored value)
Every pair of a tolerance comparison has all five yardstick means > 0 for every image (asserted), so the zero-gradient rule
is not what is being compared; that rule has its own constructed pair.  Both value figures go to the parity report."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_util as hu  # noqa: E402
import msssim_loss_ref as ref  # noqa: E402
from hip_util import DEV  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402
from ctu.utils import synthetic  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_metrics_pairs.npz')
MEAN, STD = (0.5, 0.5, 0.5), (1.0, 1.0, 1.0)          # the project's normalisation (ctu.utils.synthetic.default_opt)
MEAN2, STD2 = (0.5, 0.4, 0.45), (1.0, 0.9, 1.1)       # a per-channel one: the std_c factor of the gradient
MARGIN = 2.0
DTYPE_NAME = {F32: 'fp32', BF16: 'bf16'}


# ---- image pairs -----------------------------------------------------------------------------------------------------------
def _tile(img_hwc, H, W):
  h, w = img_hwc.shape[:2]
  a = np.pad(img_hwc, ((0, max(H - h, 0)), (0, max(W - w, 0)), (0, 0)), mode='symmetric')[:H, :W]
  return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def _normalised(u8):
  return (torch.from_numpy(u8.astype(np.float32)) / 255.0 - 0.5).to(torch.float32)


def _pairs(H, W, kinds):
  """(fake, real) fp32 normalised NCHW tensors [len(kinds), 3, H, W]."""
  z = np.load(GOLDEN)
  fake, real = [], []
  for k in kinds:
    if k.startswith('jpeg_q'):
      f, r = _normalised(_tile(z[k], H, W)), _normalised(_tile(z['original'], H, W))
    elif k == 'synthetic':
      xd = synthetic.synthetic_batch(1, H, W, seed=77)
      f, r = xd['compressed_img'][0].to(torch.float32), xd['image'][0].to(torch.float32)
    elif k == 'identical':
      r = _normalised(_tile(z['original'], H, W))
      f = r.clone()
    elif k == 'mirrored':        # real = 2 * mean_image - fake on a textured image: s_xy = -s_xx, cs < 0 where s_xx > C2 / 2
      f = _normalised(_tile(z['original'], H, W))
      r = 2.0 * f.mean(dim=(1, 2), keepdim=True) - f
    else:
      raise KeyError(k)
    fake.append(f)
    real.append(r)
  return torch.stack(fake).contiguous(), torch.stack(real).contiguous()


_CACHE = {}


def _case(H, W, kinds, dtype, mean=MEAN, std=STD):
  """The pair as the device sees it, its float64 yardstick (value and gradient) and the plain fp32 value: computed once."""
  key = (H, W, tuple(kinds), dtype, tuple(mean), tuple(std))
  if key not in _CACHE:
    fake, real = _pairs(H, W, kinds)
    fake, real = hu.quantize_like(fake, dtype), hu.quantize_like(real, dtype)
    want = ref.loss_and_grad(fake, real, mean, std)
    plain = ref.loss(fake, real, mean, std, dtype=torch.float32)['loss'].item()
    _CACHE[key] = (fake, real, want, plain)
  return _CACHE[key]


def _run(fake, real, dtype, scale=None, mean=MEAN, std=STD):
  """(loss bits as a float32 tensor on the host, stats [N, 11] float64, gradient NCHW fp32 or None)."""
  fa, ra = hu.to_act(fake, dtype), hu.to_act(real, dtype)
  slot = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
  stats = torch.zeros((fake.shape[0], 11), dtype=torch.float64, device=DEV)
  if scale is None:
    ops.msssim_loss_fwd(fa, ra, mean, std, slot, stats=stats)
    return slot.cpu(), stats.cpu(), None
  d = ops.msssim_loss_fwd_bwd(fa, ra, mean, std, slot, scale, stats=stats)
  assert d.dtype == dtype and tuple(d.t.shape) == tuple(fa.t.shape)
  assert torch.all(d.t[..., 3:] == 0), 'padding lanes of the gradient must be zero'
  return slot.cpu(), stats.cpu(), hu.to_nchw(d)


def _value_bound(name, got, want, plain):
  ek, et = abs(float(got) - float(want)), abs(plain - float(want))
  print('%s: loss %.9f, yardstick %.9f: kernel error %.3e, torch fp32 error %.3e' % (name, float(got), float(want), ek, et))
  hu.record('msssim_loss value vs fp64 yardstick [abs]: ' + name, ek, MARGIN * et, 'torch fp32 (uncentred) error %.3e' % et)
  assert ek <= MARGIN * et, '%s: kernel error %.3e > %g x torch-fp32 error %.3e' % (name, ek, MARGIN, et)


MIXED = ('synthetic', 'jpeg_q10', 'jpeg_q40', 'jpeg_q85')
CASES = [
    ('176x176', 176, 176, MIXED, MEAN, STD),                # exactly one window at scale 5
    ('177x203', 177, 203, MIXED, MEAN2, STD2),              # odd sizes at every pooling step, partial 64x16 tiles
    ('192x224 batch 2', 192, 224, ('synthetic', 'jpeg_q40'), MEAN, STD),
]


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_value_and_gradient_against_the_fp64_yardstick(case, dtype):
  name, H, W, kinds, mean, std = case
  fake, real, want, plain = _case(H, W, kinds, dtype, mean, std)
  terms = torch.cat([want['cs'][:, :4], want['ssim'][:, 4:5]], dim=1)
  assert terms.min().item() > 0, (name, 'pair unfit for a tolerance comparison')
  label = '%s %s' % (name, DTYPE_NAME[dtype])
  loss, stats, g = _run(fake, real, dtype, scale=1.0, mean=mean, std=std)
  _value_bound(label, loss.item(), want['loss'].item(), plain)
  # the per-scale means behind the loss are the yardstick's (a sanity bound, not the contract: one fp32 rounding of a moment
  # against C2, 2^-24 / 9e-4 = 7e-5, is the worst a single position can be off; a wrong scale or window shows at 1e-2)
  assert (stats[:, :5] - want['cs']).abs().max().item() < 1e-4 and (stats[:, 5:10] - want['ssim']).abs().max().item() < 1e-4
  assert (stats[:, 10] - want['ms_ssim']).abs().max().item() < 1e-4
  g64 = want['grad']
  gmax = g64.abs().max().item()
  err = (g.double() - g64).abs()
  if dtype == F32:
    hu.record('msssim_loss gradient vs fp64 yardstick [max abs / max |g64|]: ' + label, err.max().item() / gmax, 1e-3)
    print('%s: gradient error %.3e of max |g64| = %.3e' % (label, err.max().item() / gmax, gmax))
    assert err.max().item() <= 1e-3 * gmax, '%s: max |g - g64| = %.3e > 1e-3 x %.3e' % (label, err.max().item(), gmax)
  else:
    slack = (err - (1e-3 * gmax + 2.0 ** -8 * g64.abs())).max().item()
    worst = (err / (1e-3 * gmax + 2.0 ** -8 * g64.abs())).max().item()
    hu.record('msssim_loss gradient vs fp64 yardstick [|g - g64| / (1e-3 max|g64| + 2^-8 |g64|), worst element]: ' + label,
              worst, 1.0)
    print('%s: worst element at %.3f of its bound (max |g64| = %.3e)' % (label, worst, gmax))
    assert slack <= 0.0, '%s: an element misses 1e-3 max|g64| + 2^-8 |g64| by %.3e' % (label, slack)
  # forward alone writes the same loss bits; a second call of either is bit-identical
  only, stats_f, _ = _run(fake, real, dtype, mean=mean, std=std)
  assert torch.equal(only, loss) and torch.equal(stats_f, stats)
  loss2, stats2, g2 = _run(fake, real, dtype, scale=1.0, mean=mean, std=std)
  assert torch.equal(loss2, loss) and torch.equal(stats2, stats) and torch.equal(g2, g)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(176, 176), (177, 203), (192, 224)], ids=['176x176', '177x203', '192x224'])
def test_identical_images_give_loss_zero(shape, dtype):
  H, W = shape
  fake, real, want, plain = _case(H, W, ('identical',), dtype)
  assert want['loss'].item() == 0.0
  loss, stats, g = _run(fake, real, dtype, scale=1.0)
  _value_bound('%dx%d identical %s' % (H, W, DTYPE_NAME[dtype]), loss.item(), 0.0, plain)
  assert torch.all(stats == 1.0) and torch.isfinite(g).all()


def test_zero_rule_gives_exact_zeros_and_leaves_the_other_image_alone():
  kinds = ('jpeg_q40', 'mirrored')
  fake, real, want, _ = _case(176, 200, kinds, F32)
  terms = torch.cat([want['cs'][:, :4], want['ssim'][:, 4:5]], dim=1)
  assert terms[1].min().item() < 0 and want['ms_ssim'][1].item() == 0.0 and terms[0].min().item() > 0
  assert torch.all(want['grad'][1] == 0)
  loss, stats, g = _run(fake, real, F32, scale=1.0)
  assert stats[1, 10].item() == 0.0 and stats[0, 10].item() > 0.9
  assert torch.equal(torch.cat([stats[1, :4], stats[1, 9:10]]) <= 0, terms[1] <= 0)
  assert torch.all(g[1] == 0), 'an image under the zero rule must get a gradient of exact zeros'
  # the loss is the fixed-order fp64 sum of the two images' 1 - ms_ssim_n, halved, rounded once to fp32
  assert loss.item() == float(np.float32(((1.0 - stats[0, 10].item()) + 1.0) / 2.0))
  gmax = want['grad'][0].abs().max().item()
  assert (g[0].double() - want['grad'][0]).abs().max().item() <= 1e-3 * gmax
  # image 0's gradient does not depend on its neighbour (the 1 / N factor is the same): replace image 1
  fake_b, real_b, _, _ = _case(176, 200, ('jpeg_q40', 'jpeg_q10'), F32)
  assert torch.equal(fake_b[0], fake[0]) and torch.equal(real_b[0], real[0])
  _, stats_b, g_b = _run(fake_b, real_b, F32, scale=1.0)
  assert torch.equal(g_b[0], g[0]) and torch.equal(stats_b[0], stats[0])
  assert g_b[1].abs().max().item() > 0


def test_scale_is_linear_in_fp32():
  fake, real, _, _ = _case(192, 224, ('synthetic', 'jpeg_q40'), F32)
  l1, _, g1 = _run(fake, real, F32, scale=1.0)
  l2, _, g2 = _run(fake, real, F32, scale=2.0)
  assert torch.equal(l1, l2) and torch.equal(g2, 2.0 * g1)
  assert g1.abs().max().item() > 0


def test_bad_shapes_raise_through_check():
  import jpdse_hip
  slot = torch.zeros(1, dtype=torch.float32, device=DEV)
  for h, w, c in ((175, 256, 3), (256, 175, 3), (256, 256, 4)):
    a = ops.Act.empty(1, h, w, c, F32, DEV)
    a.t.zero_()
    with pytest.raises(jpdse_hip.JpdseError):
      ops.msssim_loss_fwd(a, a, (0.5,) * c, (1.0,) * c, slot)
    with pytest.raises(jpdse_hip.JpdseError):
      ops.msssim_loss_fwd_bwd(a, a, (0.5,) * c, (1.0,) * c, slot, 1.0)


# ---- the trainer ------------------------------------------------------------------------------------------------------------
CODEC = dict(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4,
             encoder_binarizer_out_channels=32)
GRAD_TOL = 1e-3        # tests/test_hip_step.py: weight gradients, max-abs relative


def _trainer(**kw):
  from ctu.trainers import get_trainer
  base = dict(ngf=8, ndf=8, n_blocks_global=1, distortion_loss_fn='ms_ssim')
  base.update(kw)
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, **base)
  torch.manual_seed(4321)
  return get_trainer(opt)(opt, 'train'), opt


def test_trainer_step_reports_the_yardstick_and_moves_the_generator():
  tr, opt = _trainer()
  xd = synthetic.synthetic_batch(1, 192, 192, seed=5)
  tr.train()
  state, _, _ = tr.model._forward_losses(xd)           # the forward the step is about to repeat, bit for bit
  fake = hu.to_nchw(state['fake'])
  real = hu.to_nchw(state['real'])
  del state
  before = {k: v.clone() for k, v in tr.model.netG.state_dict().items()}
  tr.step(xd)
  torch.cuda.synchronize()
  want = ref.loss(fake, real, opt.normalize_mean, opt.normalize_std)
  plain = ref.loss(fake, real, opt.normalize_mean, opt.normalize_std, dtype=torch.float32)['loss'].item()
  assert want['ms_ssim'].min().item() > 0
  _value_bound('trainer step 192x192 G_Distortion', tr.last_losses['G_Distortion'], want['loss'].item(), plain)
  moved = [k for k, v in tr.model.netG.state_dict().items() if k.endswith('.weight') and not torch.equal(v, before[k])]
  assert moved, 'generator weights must change'
  # evaluation figure: 1 - ms_ssim of the quantised images, the number get_eval_metrics reports
  want_ev = float(np.float32(1.0 - tr.get_eval_metrics(xd)['ms_ssim']))
  assert tr.get_eval_loss(xd) == want_ev
  ev = tr.model(xd, opt, mode='get_eval_loss')
  assert torch.is_tensor(ev) and ev.dim() == 0 and ev.dtype == torch.float32 and ev.is_cuda and ev.item() == want_ev


def test_trainer_distortion_only_gradient_is_the_yardsticks_through_netG():
  tr, opt = _trainer(no_g_gan_loss=True, no_d_gan_loss=True, no_gan_feat_loss=True, no_vgg_loss=True, skip_unused_losses=True)
  m = tr.model
  tr.train()
  xd = synthetic.synthetic_batch(1, 192, 192, seed=6)
  w = opt.lambda_distortion
  grads = lambda: {k: p.grad.detach().clone() for k, p in m.netG.named_parameters() if k.endswith('.weight')}
  # (a) the step's own route: gradient from the forward call (d_dist), then from backward_G's own call: the same bits
  state, _, _ = m._forward_losses(xd, grad_w=dict(feat=0.0, vgg=0.0, dist=w))
  assert state['d_dist'] is not None
  fake, real = hu.to_nchw(state['fake']), hu.to_nchw(state['real'])
  assert m.backward_G(state, 0.0, 0.0, 0.0, w)
  got = grads()
  state, _, _ = m._forward_losses(xd)
  assert state['d_dist'] is None
  assert m.backward_G(state, 0.0, 0.0, 0.0, w)
  for k, v in grads().items():
    assert torch.equal(v, got[k]), k
  # (b) netG.bwd fed the yardstick's gradient
  g64 = ref.loss_and_grad(fake, real, opt.normalize_mean, opt.normalize_std)['grad']
  state, _, _ = m._forward_losses(xd)
  m.netG.bwd(state['g_ctx'], hu.to_act((w * g64).to(torch.float32), F32), need_dx=False, need_dw=True)
  for k, v in grads().items():
    assert v.abs().max().item() > 0, k
    hu.assert_close(got[k].cpu(), v.cpu(), GRAD_TOL, 'ms_ssim-only generator gradient vs netG.bwd(yardstick gradient)',
                    elementwise=False, detail=k)


def test_learned_codec_step_moves_the_encoder():
  tr, opt = _trainer(**CODEC)
  assert tr.model.netE is not None
  xd = synthetic.synthetic_batch(1, 192, 192, seed=7)
  before = {k: v.clone() for k, v in tr.model.netE.state_dict().items()}
  tr.step(xd)
  torch.cuda.synchronize()
  assert 0.0 < tr.last_losses['G_Distortion'] <= 1.0
  moved = [k for k, v in tr.model.netE.state_dict().items() if k.endswith('.weight') and not torch.equal(v, before[k])]
  assert moved, 'netE weights must change'


def test_small_images_raise_a_value_error_that_names_the_limit():
  tr, opt = _trainer()
  xd = synthetic.synthetic_batch(1, 128, 192, seed=8)
  before = {k: v.clone() for k, v in tr.model.netG.state_dict().items()}
  with pytest.raises(ValueError, match='176'):
    tr.step(xd)
  with pytest.raises(ValueError, match='176'):
    tr.get_eval_loss(xd)
  for k, v in tr.model.netG.state_dict().items():
    assert torch.equal(v, before[k]), k
