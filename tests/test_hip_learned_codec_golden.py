"""GPU: the learned codec against tests/golden/learned_codec_nef8.npz, recorded from the REAL reference by
scripts/make_golden_learned_codec.py (batch 2, 64x128, encoder nef 8 / n_downsample_E 4 / B 32 / feat_num 3, G ngf 8 with one
ResnetBlock, D ndf 8).  E's weights are in the fixture with the reference's keys; G and D regenerate from the recorded seed
(oracle.ctu_cpu.nets, pinned to the reference's define_G / define_D).  The reference's own binarizer noise u is replayed
through the noise_override hook; the fixture's seeds keep every threshold margin above 1e-4."""
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

from oracle.ctu_cpu import model as omodel, nets  # noqa: E402

NET_TOL = 2e-4
GRAD_TOL = 1e-3
LOSS_TOL = 1e-3
WEIGHT_TOL = 3e-3
LIVE_BIAS = 'model.30.bias'      # the only bias not followed by an affine-less InstanceNorm, in both G (ngf 8, 1 block) and E


@pytest.fixture(scope='module')
def gold(golden_dir):
  z = np.load(os.path.join(golden_dir, 'learned_codec_nef8.npz'))
  return {k: z[k] for k in z.files}


def _opt(dtype='fp32', **over):
  kw = dict(gpu_ids=[0], print_losses=False, ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False,
            no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32,
            compute_dtype=dtype)
  kw.update(over)
  return omodel.default_opt(**kw)


def _weights(gold):
  torch.manual_seed(int(gold['seed']))
  opt = _opt()
  sd_G = nets.init_generator(omodel.gen_cfg(opt), 36 + 3, 3)
  sd_D = nets.init_discriminator(36 + 3, 8, 3, 2)
  sd_E = {str(k): torch.from_numpy(gold['E:' + str(k)]) for k in gold['Ekeys']}
  return sd_G, sd_D, sd_E


def _train_trainer(gold, dtype='fp32'):
  from ctu.trainers import get_trainer
  opt = _opt(dtype)
  tr = get_trainer(opt)(opt, 'train')
  sd_G, sd_D, sd_E = _weights(gold)
  tr.model.netG.load_state_dict(sd_G)
  tr.model.netD.load_state_dict(sd_D)
  tr.model.netE.load_state_dict(sd_E)
  return tr


def _test_trainer(gold, tmp_path, dtype='fp32'):
  """The test.py flow: a test-mode trainer loading net_G.pth and a reference-keyed net_E.pth from checkpoints_dir."""
  from ctu.trainers import get_trainer
  sd_G, _, sd_E = _weights(gold)
  torch.save(sd_G, os.path.join(str(tmp_path), 'net_G.pth'))
  torch.save(sd_E, os.path.join(str(tmp_path), 'net_E.pth'))
  opt = _opt(dtype, is_train=False, checkpoints_dir=str(tmp_path))
  te = get_trainer(opt)(opt, 'test')
  for k, v in te.model.netE.state_dict().items():
    assert torch.equal(v.cpu(), sd_E[k]), k
  return te


def _batch(gold):
  return omodel.synthetic_batch(int(gold['batch']), int(gold['height']), int(gold['width']), seed=int(gold['img_seed']))


def _rel(a, b):
  return abs(a - b) / max(abs(b), 1e-30)


def test_golden_encoder_keys_and_reference_net_E_pth(gold, tmp_path):
  from ctu.models.pix2pixHD_networks import networks
  enc = networks.define_G(3, 3, 8, 'encoder', 4, binarize_encoder=True, encoder_binarizer_out_channels=32)
  want = {str(k): tuple(gold['E:' + str(k)].shape) for k in gold['Ekeys']}
  assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want
  _test_trainer(gold, tmp_path)          # loads the reference-keyed net_E.pth exactly (checked tensor by tensor)


def test_golden_eval_features_code_rate(gold, tmp_path):
  te = _test_trainer(gold, tmp_path)
  xd = _batch(gold)
  te.eval()
  # rate first, then image, then code: the reference test.py order (test.py:78-99)
  shannon, actual = te.get_eval_rate(xd)
  assert _rel(shannon.item(), float(gold['rate_shannon'])) <= 1e-6, (shannon.item(), float(gold['rate_shannon']))
  assert actual == float(gold['rate_actual'])
  te.get_img(xd)
  code = te.get_code(xd).cpu()
  want = (torch.from_numpy(gold['eval_code']).reshape(code.shape[0], -1) + 1) / 2
  assert torch.equal(code, want)          # every |t| > 1e-4 in the fixture
  feat = te.model.netE(xd['image'].cuda())[0].cpu().double()
  ref = torch.from_numpy(gold['eval_feat0']).double()
  assert (feat - ref).abs().max().item() <= NET_TOL * ref.abs().max().item()


def test_golden_eval_code_bf16(gold, tmp_path):
  te = _test_trainer(gold, tmp_path, 'bf16')
  xd = _batch(gold)
  code = te.get_code(xd).cpu()
  t = torch.from_numpy(gold['eval_t']).reshape(code.shape[0], -1)
  want = (torch.from_numpy(gold['eval_code']).reshape(code.shape[0], -1) + 1) / 2
  sure = t.abs() > 2e-2
  assert sure.float().mean().item() > 0.75              # a comparison over most of the code, not a handful of bits
  assert torch.equal(code[sure], want[sure])


def _check_grads(params, norms, keys, full, what, fp64=None):
  """Gradient norms (every live tensor) and full gradients (the fixture's small layers) within 1e-3 of the reference.  fp64
  (step only: {key: (torch-fp32, torch-fp64) gradients of the oracle composition}) is tests/test_hip_step.py's yardstick for a
  tensor that misses the direct bound: the L1 terms have sign() gradients, so two correct fp32 implementations differ by
  more than 1e-3 on some tensors; HIP must then be as close to fp64 as fp32 torch is, within a factor 2."""
  for k, gn in zip(keys, norms):
    k = str(k)
    if k.endswith('.bias') and k != LIVE_BIAS:
      continue                             # dead bias: rounding noise on both sides
    g = params[k].grad.detach().cpu().double()
    checks = [('norm', _rel(g.norm().item(), float(gn)))]
    if k in full:
      r = torch.from_numpy(full[k]).double()
      checks.append(('relative L2', ((g - r).norm() / r.norm()).item()))
    for kind, err in checks:
      if err <= GRAD_TOL:
        continue
      assert fp64 is not None and k in fp64, '%s: %s gradient %s error %.3e' % (what, k, kind, err)
      r32, r64 = fp64[k]
      e_hip, e_t32 = ((g - r64).norm() / r64.norm()).item(), ((r32 - r64).norm() / r64.norm()).item()
      assert e_hip <= max(GRAD_TOL, 2.0 * e_t32), \
          '%s: %s gradient %s error %.3e; vs fp64 HIP %.2e, torch-fp32 %.2e' % (what, k, kind, err, e_hip, e_t32)
      print('%s: %s %s %.2e vs the reference; vs fp64: HIP %.2e, torch-fp32 %.2e' % (what, k, kind, err, e_hip, e_t32))


def test_golden_encoder_train_forward_backward(gold):
  from jpdse_hip import ops, F32
  tr = _train_trainer(gold)
  enc = tr.model.netE
  enc.train()
  xd = _batch(gold)
  enc._binarizer.noise_override = torch.from_numpy(gold['enc_u']).cuda()
  y, ctx = enc.fwd(ops.nchw_to_nhwc(xd['image'].cuda().contiguous(), F32))
  r = torch.rand(y.N, 3, y.H, y.W, generator=torch.Generator().manual_seed(int(gold['enc_r_seed']))) - 0.5
  enc.bwd(ctx, ops.nchw_to_nhwc(r.cuda().contiguous(), F32))
  torch.cuda.synchronize()
  loss = (ops.nhwc_to_nchw(y).cpu().double() * r.double()).sum().item()
  assert _rel(loss, float(gold['enc_loss'])) <= 1e-4, (loss, float(gold['enc_loss']))
  full = {k[len('enc_g:'):]: v for k, v in gold.items() if k.startswith('enc_g:')}
  _check_grads(dict(enc.named_parameters()), gold['enc_gradnorms'], gold['enc_gradkeys'], full, 'encoder')


def test_golden_step_with_reference_noise(gold):
  """One trainer step with the reference's own binarizer noise against the reference's trainer.step: the six losses, every G and
  E gradient, and the post-Adam E weights (tests/test_hip_step.py's rule: relative L2 <= 3e-3, no element beyond 2 lr)."""
  from test_hip_learned_codec import CodecOracle
  tr = _train_trainer(gold)
  xd = _batch(gold)
  u = torch.from_numpy(gold['step_u'])
  # the oracle composition on the same weights and noise: pinned to the reference by its fp32 gradients below, and the fp64
  # yardstick for tensors whose fp32 gradients scatter by more than 1e-3
  sd_G, sd_D, sd_E = _weights(gold)
  ora_opt = omodel.default_opt(ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False, no_encoder_binarization=False,
                               feat_num=3, nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32, seed=0)
  ora = CodecOracle(ora_opt, sd_E, sd_G=sd_G, sd_D=sd_D)
  ora.u_override = u
  g32, _ = ora.grads_in_dtype(xd, torch.float32)
  g64, _ = ora.grads_in_dtype(xd, torch.float64)
  fp64 = {k: (g32['E.' + k].double(), g64['E.' + k].double()) for k in sd_E}
  fp64_G = {k: (g32[k].double(), g64[k].double()) for k in sd_G}
  for k, gn in zip(gold['enc_gradkeys'], gold['step_E_gradnorms']):
    k = str(k)
    if k.endswith('.weight'):
      assert _rel(g32['E.' + k].double().norm().item(), float(gn)) <= GRAD_TOL, 'oracle composition vs reference: ' + k
  tr.model.netE._binarizer.noise_override = u.cuda()
  tr.step(xd)
  torch.cuda.synchronize()
  for name, v in zip(gold['step_loss_names'], gold['step_losses']):
    got = tr.last_losses[str(name)]
    assert abs(got - v) <= LOSS_TOL * max(abs(v), 1e-6), (str(name), got, float(v))
  _check_grads(dict(tr.model.netG.named_parameters()), gold['step_G_gradnorms'], gold['step_G_gradkeys'], {}, 'step G',
               fp64_G)
  full = {k[len('step_E_g:'):]: v for k, v in gold.items() if k.startswith('step_E_g:')}
  params = dict(tr.model.netE.named_parameters())
  _check_grads(params, gold['step_E_gradnorms'], gold['enc_gradkeys'], full, 'step E', fp64)
  lr = tr.opt.lr
  for k, wn in zip(gold['enc_gradkeys'], gold['step_E_wnorms']):
    k = str(k)
    if k.endswith('.bias') and k != LIVE_BIAS:
      continue                             # dead bias: the reference's Adam steps on rounding noise, the HIP gradient is 0
    w = params[k].detach().cpu().double()
    assert _rel(w.norm().item(), float(wn)) <= WEIGHT_TOL, k
    if 'step_E_w:' + k in gold and k.endswith('.weight'):
      r = torch.from_numpy(gold['step_E_w:' + k]).double()
      assert ((w - r).norm() / r.norm()).item() <= WEIGHT_TOL, k
      assert (w - r).abs().max().item() <= 2.05 * lr, '%s exceeds the Adam sign-flip bound' % k
