"""GPU: the learned codec (feature encoder netE with the stochastic binarizer, get_code / get_eval_rate).

Kernels against the numpy Philox4x32-10 of tests/learned_codec_util.py; the encoder and the whole train step against a
torch-CPU composition of oracle.ctu_cpu.nets pieces (reference networks.py:307-369, binarize.py:13-65) fed the same noise;
checkpoints, codes, rates and data parallelism through the trainer API."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import learned_codec_util as lcu  # noqa: E402
from jpdse_hip import F32, BF16, ops  # noqa: E402
from oracle.ctu_cpu import model as omodel, nets  # noqa: E402

NET_TOL = 2e-4        # fp32 network outputs, max-abs relative to the output's max
GRAD_TOL = 1e-3       # fp32 weight gradients, relative L2
LOSS_TOL = 1e-3
WEIGHT_TOL = 3e-3
CODEC = dict(no_feat_encoding=False, no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4,
             encoder_binarizer_out_channels=32, ngf=8, ndf=8, n_blocks_global=1, seed=20261016)


def _act(x_nchw, dtype):
  return ops.nchw_to_nhwc(x_nchw.float().contiguous().cuda(), dtype)


def _stored(x, dtype):
  """x as the kernels see it after nchw_to_nhwc in `dtype` (bf16 rounding)."""
  return x.to(torch.bfloat16).float() if dtype == BF16 else x.float()


# =============================================================================================
# kernels
# =============================================================================================
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('seed,draw,n0', [(0, 0, 0), (20261016, 3, 5), ((1 << 63) + 12345, (1 << 33) + 7, 1000)])
def test_binarize_train_bits_match_numpy_philox(dtype, seed, draw, n0):
  N, C, H, W = 2, 13, 9, 11                 # C = 13: padding lanes in both dtypes
  g = torch.Generator().manual_seed(seed % 1000 + draw % 1000)
  t = torch.rand(N, C, H, W, generator=g) * 2 - 1
  x = _act(t, dtype)
  out = x.empty_like()
  out.t.fill_(7.0)
  b = ops.binarize_fwd(x, True, seed, draw, n0, out=out)
  got = ops.nhwc_to_nchw(b).cpu().numpy()
  u = lcu.batch_noise(N, C, H, W, seed, draw, n0)
  want = lcu.soft_sign(_stored(t, dtype).numpy(), u)
  assert np.array_equal(got, want)
  assert torch.all(b.t[..., C:] == 0)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_binarize_eval_sign_and_override(dtype):
  N, C, H, W = 2, 5, 7, 6
  g = torch.Generator().manual_seed(3)
  t = torch.rand(N, C, H, W, generator=g) * 2 - 1
  t[0, 1, 2, :] = 0.0                       # exact zeros: sign(0) = 0 (torch.sign)
  t[1, 4, :, 3] = 0.0
  x = _act(t, dtype)
  got = ops.nhwc_to_nchw(ops.binarize_fwd(x, False)).cpu()
  assert torch.equal(got, torch.sign(_stored(t, dtype)))
  # the override replaces the generator exactly
  u = torch.rand(N, C, H, W, generator=g)
  got = ops.nhwc_to_nchw(ops.binarize_fwd(x, True, 99, 1, 0, u=u.cuda())).cpu().numpy()
  assert np.array_equal(got, lcu.soft_sign(_stored(t, dtype).numpy(), u.numpy()))


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_code_stats_and_export(dtype):
  N, C, H, W = 3, 13, 10, 9                 # bits = 1170, not a multiple of 8
  g = torch.Generator().manual_seed(5)
  v = torch.randint(-1, 2, (N, C, H, W), generator=g).float()
  b = _act(v, dtype)
  counts = ops.code_stats(b).cpu().numpy()
  vn = v.numpy().reshape(N, -1)
  assert np.array_equal(counts[:, 0], (vn > 0).sum(1)) and np.array_equal(counts[:, 1], (vn == 0).sum(1))
  exp = ops.code_export(b).cpu().numpy()
  assert exp.shape == (N, C * H * W) and np.array_equal(exp, (vn + 1) / 2)
  packed = ops.code_export(b, packed=True).cpu().numpy()
  assert np.array_equal(packed, np.packbits((vn > 0).astype(np.uint8), axis=1))


def test_code_stats_large_image():
  """The bench shape's code (B 128 at 1/16 of 1024x512): counts exact over 262,144 bits per image."""
  N, C, H, W = 2, 128, 32, 64
  g = torch.Generator().manual_seed(9)
  v = torch.randint(-1, 2, (N, C, H, W), generator=g).float()
  counts = ops.code_stats(_act(v, BF16)).cpu().numpy()
  vn = v.numpy().reshape(N, -1)
  assert np.array_equal(counts[:, 0], (vn > 0).sum(1)) and np.array_equal(counts[:, 1], (vn == 0).sum(1))


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_binarize_batch_split_invariance(dtype):
  N, C, H, W = 2, 32, 8, 16
  t = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(11)) * 2 - 1
  x = _act(t, dtype)
  whole = ops.binarize_fwd(x, True, 42, 9, 0)
  for i in range(N):
    part = ops.binarize_fwd(x.batch_slice(i, i + 1), True, 42, 9, i)
    assert torch.equal(part.t, whole.t[i:i + 1])


def test_binarize_is_unbiased():
  """E[b] = t (SoftSignFunction: P(b = 1) = (1 + t) / 2): 16 channels of constant t, 65,536 draws each, within 4 sigma."""
  C, H, W = 16, 256, 256
  tv = torch.linspace(-0.9, 0.9, C)
  t = tv.view(1, C, 1, 1).expand(1, C, H, W).contiguous()
  b = ops.nhwc_to_nchw(ops.binarize_fwd(_act(t, F32), True, 1234, 0, 0)).cpu().double()
  mean = b.mean(dim=(0, 2, 3))
  sigma = torch.sqrt((1 - tv.double() ** 2) / (H * W))
  assert torch.all((mean - tv.double()).abs() <= 4 * sigma), (mean, tv)


# =============================================================================================
# encoder vs a torch-CPU composition
# =============================================================================================
class _STE(torch.autograd.Function):
  """SoftSignFunction with given noise (binarize.py:17-28): forward soft sign, backward identity."""

  @staticmethod
  def forward(ctx, t, u):
    return torch.where((1 - t) / 2 <= u, torch.ones_like(t), -torch.ones_like(t))

  @staticmethod
  def backward(ctx, g):
    return g, None


def oracle_encoder(sd, x, n_down, train=False, u=None, bits=None, code_only=False):
  """Encoder.forward (networks.py:307-369) with InstanceNorm, binarizer (no bias) and ConvT; `bits` replaces the binarizer's
  output (the GPU's own bits, so that a flipped bit is not charged to the decoder)."""
  q, qw = nets.q, nets.qw                 # bf16-storage emulation points (identity unless nets.storage_bf16(True))
  h = q(F.relu(nets.inorm(nets.conv_reflect(x, sd['model.1.weight'], sd['model.1.bias'], 3))))
  for i in range(n_down):
    k = 4 + 3 * i
    h = q(F.relu(nets.inorm(q(F.conv2d(h, qw(sd['model.%d.weight' % k]), sd['model.%d.bias' % k], stride=2, padding=1)))))
  kb = 4 + 3 * n_down
  t = q(torch.tanh(F.conv2d(h, qw(sd['model.%d.conv.weight' % kb]))))
  if bits is not None:
    b = t + (bits - t).detach()
  elif train:
    b = _STE.apply(t, u)
  else:
    b = torch.sign(t)
  if code_only:
    return b, t
  h = b
  for i in range(n_down):
    k = kb + 1 + 3 * i
    h = q(F.conv_transpose2d(h, qw(sd['model.%d.weight' % k]), sd['model.%d.bias' % k], stride=2, padding=1,
                             output_padding=1))
    h = q(F.relu(nets.inorm(h)))
  last = kb + 1 + 3 * n_down + 1
  y = q(torch.tanh(F.conv2d(F.pad(h, (3, 3, 3, 3), mode='reflect'), qw(sd['model.%d.weight' % last]),
                            sd['model.%d.bias' % last])))
  return y, t


def _encoder(dtype, seed=7):
  from ctu.models.pix2pixHD_networks import networks
  torch.manual_seed(seed)
  enc = networks.define_G(3, 3, 8, 'encoder', 4, gpu_ids=[0], binarize_encoder=True, encoder_binarizer_out_channels=32,
                          compute_dtype='bf16' if dtype == BF16 else 'fp32')
  sd = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
  return enc, sd


def _img(seed, N=2, H=64, W=128):
  return torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(seed)) - 0.5


def test_encoder_eval_forward_and_code_fp32():
  enc, sd = _encoder(F32)
  enc.eval()
  x = _img(1)
  y = enc(x.cuda()).cpu().double()
  code = enc(x.cuda(), mode='get_binary_code').cpu().double()
  want, t = oracle_encoder(sd, x.double(), 4)
  assert (y - want).abs().max().item() <= NET_TOL * want.abs().max().item()
  sure = t.abs() > 1e-4
  assert sure.float().mean().item() > 0.99
  assert torch.equal(code[sure], torch.sign(t)[sure])


def test_encoder_train_forward_and_gradients_fp32():
  enc, sd = _encoder(F32)
  enc.train()
  x = _img(2)
  _, t0 = oracle_encoder(sd, x.double(), 4, code_only=True)
  u = torch.rand(t0.shape, generator=torch.Generator().manual_seed(3))
  enc._binarizer.noise_override = u.cuda()
  xa = _act(x, F32)
  y, ctx = enc.fwd(xa)
  dy = torch.randn(y.N, y.C, y.H, y.W, generator=torch.Generator().manual_seed(4)) * 0.1
  enc.bwd(ctx, _act(dy, F32))
  torch.cuda.synchronize()
  sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
  want, t = oracle_encoder(sdr, x.double(), 4, train=True, u=u.double())
  margin = ((1 - t) / 2 - u.double()).abs().min().item()
  assert margin > 1e-5, 'noise too close to a threshold for a like-for-like comparison (%.2e)' % margin
  got = ops.nhwc_to_nchw(y).cpu().double()
  assert (got - want.detach()).abs().max().item() <= NET_TOL * want.abs().max().item()
  (want * dy.double()).sum().backward()
  params = dict(enc.named_parameters())
  for k, p in sdr.items():
    if k.endswith('.bias') and k != 'model.30.bias':
      continue                # in front of an affine-less InstanceNorm: no gradient (dead bias)
    g = params[k].grad.detach().cpu().double()
    err = ((g - p.grad).norm() / p.grad.norm()).item()
    assert err <= GRAD_TOL, '%s: relative L2 gradient error %.3e' % (k, err)


def test_encoder_bf16_bits_and_features():
  """bf16: bits equal the fp32 composition wherever the threshold margin exceeds 2e-2; the features equal the composition fed
  the GPU's own bits to bf16 accuracy."""
  enc, sd = _encoder(BF16)
  enc.eval()
  x = _img(5)
  code = enc(x.cuda(), mode='get_binary_code').cpu().double()
  _, t = oracle_encoder(sd, x.double(), 4, code_only=True)
  sure = t.abs() > 2e-2
  assert torch.equal(code[sure], torch.sign(t)[sure])
  y = enc(x.cuda()).cpu().double()
  want, _ = oracle_encoder(sd, x.double(), 4, bits=code)
  cos = F.cosine_similarity(y.flatten(), want.flatten(), dim=0).item()
  assert cos >= 0.995 and (y - want).abs().max().item() <= 0.1, (cos, (y - want).abs().max().item())


# =============================================================================================
# whole step, checkpoints, codes
# =============================================================================================
class CodecOracle(omodel.OracleTrainer):
  """OracleTrainer with the learned codec: G sees [semantics | netE(image)], netE's parameters join optimizer G after G's
  (model.py:269-270), training forwards draw the binarizer noise from the numpy Philox with the model's (seed, n_global,
  draw) addressing -- or take `u_override`."""

  def __init__(self, opt, sd_E, **kw):
    super(CodecOracle, self).__init__(opt, **kw)
    for k, v in sd_E.items():
      self.G['E.' + k] = v.detach().clone().float().requires_grad_(True)
    self.optimizer_G = torch.optim.Adam(list(self.G.values()), lr=opt.lr, betas=(opt.beta1, opt.beta2))
    self.seed, self.draw, self.training, self.u_override = opt.seed, 0, True, None

  def generate(self, input_label, src):
    E = {k[2:]: v for k, v in self.G.items() if k.startswith('E.')}
    n_down = self.opt.n_downsample_E
    if self.training:
      _, t = oracle_encoder({k: v.detach() for k, v in E.items()}, src, n_down, code_only=True)
      u = self.u_override
      if u is None:
        u = torch.from_numpy(lcu.batch_noise(t.shape[0], t.shape[1], t.shape[2], t.shape[3], self.seed, self.draw))
      self.last_margin = ((1 - t) / 2 - u).abs().min().item()
      feat, _ = oracle_encoder(E, src, n_down, train=True, u=u)
      self.draw += 1
    else:
      feat, _ = oracle_encoder(E, src, n_down)
    return nets.generator(self.G, nets.q(torch.cat((input_label, feat), dim=1)), self.cfg)

  def get_img(self, x_dict):
    self.training = False
    try:
      return super(CodecOracle, self).get_img(x_dict)
    finally:
      self.training = True


def _codec_pair(dtype='fp32', seed=1234, **over):
  from ctu.trainers import get_trainer
  kw = dict(CODEC)
  kw.update(over)
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, compute_dtype=dtype, **kw)
  torch.manual_seed(seed)
  tr = get_trainer(opt)(opt, 'train')
  sd_E = {k: v.detach().cpu() for k, v in tr.model.netE.state_dict().items()}
  ora_opt = omodel.default_opt(**kw)
  sd_G = None
  if kw['feat_num'] != ora_opt.input_nc:     # G's input: semantics (36) + feat_num encoded channels
    sd_G = nets.init_generator(omodel.gen_cfg(ora_opt), 36 + kw['feat_num'], ora_opt.num_out_channels)
  ora = CodecOracle(ora_opt, sd_E, sd_G=sd_G)
  tr.model.netG.load_state_dict({k: v.detach() for k, v in ora.G.items() if not k.startswith('E.')})
  tr.model.netD.load_state_dict({k: v.detach() for k, v in ora.D.items()})
  return tr, ora, opt


def _check_weights(tr, ora, tol, what):
  """tests/test_hip_step.py's rule: relative L2 <= tol per weight tensor, no element beyond the 2 lr Adam sign-flip bound."""
  lr = tr.opt.lr
  pairs = [(tr.model.netG.state_dict(), ''), (tr.model.netE.state_dict(), 'E.')]
  for sd, pre in pairs:
    for k, v in sd.items():
      if not k.endswith('.weight'):
        continue
      a, b = v.cpu().double(), ora.G[pre + k].detach().double()
      l2 = ((a - b).norm() / b.norm()).item()
      assert l2 <= tol, '%s: %s%s relative L2 error %.3e' % (what, pre, k, l2)
      assert (a - b).abs().max().item() <= 2.05 * lr, '%s: %s%s exceeds the Adam sign-flip bound' % (what, pre, k)
  for k, v in tr.model.netD.state_dict().items():
    if k.endswith('.weight'):
      a, b = v.cpu().double(), ora.D[k].detach().double()
      assert ((a - b).norm() / b.norm()).item() <= tol, '%s: %s' % (what, k)


def _check_losses(tr, ora, tol, what):
  for k, v in ora.last_losses.items():
    got = tr.last_losses[k]
    assert abs(got - v) <= tol * max(1.0, abs(v)), '%s: loss %s %.6f vs %.6f' % (what, k, got, v)


@pytest.mark.parametrize('use_compressed', [False, True], ids=['image', 'compressed'])
def test_step_with_philox_stream_matches_oracle(use_compressed):
  """The HIP step on its own noise stream against the oracle drawing u from the numpy Philox with (seed, n_global, draw):
  checks the wiring of seed, image index and the draw counter (two steps: draw 0 then 1)."""
  tr, ora, opt = _codec_pair(use_compressed=use_compressed)
  for s in range(2):
    xd = omodel.synthetic_batch(2, 64, 128, seed=31 + s)
    tr.step(xd)
    ora.step(xd)
    torch.cuda.synchronize()
    assert ora.last_margin > 1e-5, 'noise within 1e-5 of a threshold: pick another seed'
    _check_losses(tr, ora, LOSS_TOL, 'step %d' % s)
    _check_weights(tr, ora, WEIGHT_TOL, 'step %d' % s)
    tr.model.netG.load_state_dict({k: v.detach() for k, v in ora.G.items() if not k.startswith('E.')})
    tr.model.netE.load_state_dict({k[2:]: v.detach() for k, v in ora.G.items() if k.startswith('E.')})
    tr.model.netD.load_state_dict({k: v.detach() for k, v in ora.D.items()})
    hip_g = dict(tr.model.netG.named_parameters())
    hip_g.update({'E.' + k: v for k, v in tr.model.netE.named_parameters()})
    for opt_h, opt_o, hip, ref in ((tr.optimizer_G, ora.optimizer_G, hip_g, ora.G),
                                   (tr.optimizer_D, ora.optimizer_D, dict(tr.model.netD.named_parameters()), ora.D)):
      for k, p_o in ref.items():
        st_o = opt_o.state.get(p_o)
        if not st_o:
          continue
        st = opt_h._ensure_state(hip[k])
        st['exp_avg'].copy_(st_o['exp_avg'])
        st['exp_avg_sq'].copy_(st_o['exp_avg_sq'])
        st['step'] = torch.tensor(float(st_o['step']))
  assert tr.model.codec_draw == 2 and ora.draw == 2


def test_step_feat_num_5_matches_oracle():
  """--feat_num 5 != input_nc: the 41-channel generator input, the encoder's 5-channel head and the generator's data gradient
  restricted to channels [36, 41), against the oracle on its Philox stream."""
  tr, ora, opt = _codec_pair(feat_num=5)
  assert tr.model.netG.input_nc == 36 + 5 and tr.model.netE.output_nc == 5
  xd = omodel.synthetic_batch(2, 64, 128, seed=45)
  tr.step(xd)
  ora.step(xd)
  torch.cuda.synchronize()
  assert ora.last_margin > 1e-5
  _check_losses(tr, ora, LOSS_TOL, 'feat_num 5 step')
  _check_weights(tr, ora, WEIGHT_TOL, 'feat_num 5 step')
  a1 = tr.get_img(xd)
  assert torch.equal(a1, tr.get_img(xd)) and tuple(a1.shape) == (2, 3, 64, 128)


def test_step_with_noise_override_matches_oracle():
  tr, ora, opt = _codec_pair()
  xd = omodel.synthetic_batch(2, 64, 128, seed=41)
  u = torch.rand(2, 32, 4, 8, generator=torch.Generator().manual_seed(8))
  tr.model.netE._binarizer.noise_override = u.cuda()
  ora.u_override = u
  tr.step(xd)
  ora.step(xd)
  torch.cuda.synchronize()
  assert ora.last_margin > 1e-5
  _check_losses(tr, ora, LOSS_TOL, 'override step')
  _check_weights(tr, ora, WEIGHT_TOL, 'override step')


def test_step_bf16_tracks_fp32_oracle():
  """bf16, with the criterion of tests/test_hip_configs.py: losses within 5 % of the fp32 oracle's, and every encoder weight
  gradient at least as close in direction to the fp32 oracle's as the oracle's own bf16-storage emulation is (cosine within
  0.02 of it).  The noise is given (noise_override) and keeps every threshold 0.1 away from the fp32 tanh output, so that the
  bf16 tanh output -- within bf16 rounding of it -- yields the same bits everywhere."""
  tr, ora, opt = _codec_pair('bf16')
  xd = omodel.synthetic_batch(2, 64, 128, seed=51)
  E = {k: v.detach().cpu().double() for k, v in tr.model.netE.state_dict().items()}
  _, t = oracle_encoder(E, xd['image'].double(), 4, code_only=True)
  h = ((1 - t) / 2).float()
  up = torch.rand(h.shape, generator=torch.Generator().manual_seed(12)) < 0.5
  u = torch.where(up, h + 0.1, h - 0.1).clamp(0.0, 1.0 - 2 ** -24)
  u = torch.where((u - h).abs() < 0.05, torch.where(up, torch.zeros_like(h), torch.full_like(h, 1.0 - 2 ** -24)), u)
  sd_E = {k: v.detach().cpu() for k, v in tr.model.netE.state_dict().items()}
  emu = CodecOracle(omodel.default_opt(**CODEC), sd_E,
                    sd_G={k: v.detach() for k, v in ora.G.items() if not k.startswith('E.')},
                    sd_D={k: v.detach() for k, v in ora.D.items()})
  tr.model.netE._binarizer.noise_override = u.cuda()
  ora.u_override = emu.u_override = u
  tr.step(xd)
  ora.step(xd)
  nets.storage_bf16(True)
  try:
    emu.step(xd)
  finally:
    nets.storage_bf16(False)
  torch.cuda.synchronize()
  for k, v in ora.last_losses.items():
    assert abs(tr.last_losses[k] - v) <= 0.05 * max(1.0, abs(v)), k
  cos = lambda a, b: F.cosine_similarity(a, b, dim=0).item()
  for k, p in tr.model.netE.named_parameters():
    if k.endswith('.weight'):
      a = p.grad.detach().cpu().double().flatten()
      r = ora.G['E.' + k].grad.detach().double().flatten()
      e = emu.G['E.' + k].grad.detach().double().flatten()
      print('%s: bf16 vs fp32 oracle %.4f, emulation vs fp32 oracle %.4f' % (k, cos(a, r), cos(e, r)))
      assert cos(a, r) >= cos(e, r) - 0.02, '%s: bf16 %.4f, emulation %.4f' % (k, cos(a, r), cos(e, r))


def test_codes_rates_checkpoints(tmp_path):
  from ctu.trainers import get_trainer
  tr, ora, opt = _codec_pair()
  xd = omodel.synthetic_batch(2, 64, 128, seed=61)
  tr.step(xd)
  # get_code: [N, bits] fp32 of 0 / 1 on the GPU, equal to the composition's eval code where the margin is clear
  code = tr.get_code(xd)
  assert code.is_cuda and code.dtype == torch.float32 and tuple(code.shape) == (2, 32 * 4 * 8)
  E = {k: v.detach().cpu().double() for k, v in tr.model.netE.state_dict().items()}
  b, t = oracle_encoder(E, xd['image'].double(), 4, code_only=True)
  want = ((b.reshape(2, -1) + 1) / 2)
  sure = (t.abs() > 1e-4).reshape(2, -1)
  assert torch.equal(code.cpu().double()[sure], want[sure])
  packed = tr.get_code(xd, packed=True)
  assert packed.dtype == torch.uint8 and np.array_equal(packed.cpu().numpy(),
                                                        np.packbits(code.cpu().numpy() > 0.5, axis=1))
  # get_eval_rate: the reference's formula (nats) on the code
  shannon, actual = tr.get_eval_rate(xd)
  assert torch.is_tensor(shannon) and shannon.dim() == 0 and isinstance(actual, float)
  pix = 64 * 128
  c = code.cpu().float()
  tot = 0.
  for j in range(2):
    p = torch.mean(c[j])
    tot += (-p * torch.log(p) - (1 - p) * torch.log(1 - p)) * c.shape[1] / pix
  assert abs(shannon.item() - (tot / 2).item()) <= 1e-6 * abs((tot / 2).item())
  assert actual == c.shape[1] / pix
  # inference is deterministic (eval-mode binarizer)
  a1, a2 = tr.get_img(xd), tr.get_img(xd)
  assert torch.equal(a1, a2)
  assert tr.get_eval_loss(xd) == tr.get_eval_loss(xd)
  # checkpoints: net_E.pth with reference keys, optimizer G state = G then E
  opt.save_dir = str(tmp_path)
  tr.save(0, 1.0)
  sd = torch.load(os.path.join(str(tmp_path), 'net_E.pth'))
  assert 'model.16.conv.weight' in sd and tuple(sd['model.16.conv.weight'].shape) == (32, 128, 1, 1)
  rec = torch.load(os.path.join(str(tmp_path), 'stats_and_optim.pt'))
  n_g, n_e = len(list(tr.model.netG.parameters())), len(list(tr.model.netE.parameters()))
  assert len(rec['optimizer_G_state_dict']['param_groups'][0]['params']) == n_g + n_e
  st = rec['optimizer_G_state_dict']['state']
  assert tuple(st[n_g]['exp_avg'].shape) == tuple(tr.model.netE.model[1].weight.shape)
  # a test-mode trainer loads the checkpoint and reproduces the codes and the image (test.py flow)
  import copy
  topt = copy.copy(opt)
  topt.is_train, topt.checkpoints_dir = False, str(tmp_path)
  te = get_trainer(topt)(topt, 'test')
  te.eval()
  assert torch.equal(te.get_code(xd), code)
  assert torch.equal(te.get_img(xd), a1)
  s2, a2_ = te.get_eval_rate(xd)
  assert torch.equal(s2.cpu(), shannon.cpu()) and a2_ == actual


def _dp_worker(q):
  for p in (ROOT, os.path.join(ROOT, 'jpd-se_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
      sys.path.insert(0, p)
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(29400 + os.getpid() % 200))
  os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  torch.cuda.set_device(0)
  dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
  try:
    from ctu.trainers import get_trainer
    opt = omodel.default_opt(gpu_ids=[0], print_losses=False, **CODEC)

    def make():
      torch.manual_seed(4321)
      return get_trainer(opt)(opt, 'train')

    plain, dp = make(), make()
    dp.model.netG.load_state_dict(plain.model.netG.state_dict())
    dp.model.netD.load_state_dict(plain.model.netD.state_dict())
    dp.model.netE.load_state_dict(plain.model.netE.state_dict())
    dp.enable_data_parallel(bucket_bytes=64 << 10)
    bg = dp.model.grad_buckets['G']
    in_buckets = {id(p) for b in bg.buckets for _, p, _, _ in b['params']}
    all_e = all(id(p) in in_buckets for p in dp.model.netE.parameters())
    for s in range(2):
      xd = omodel.synthetic_batch(2, 64, 128, seed=71 + s)
      plain.step(xd)
      dp.step(xd)
    torch.cuda.synchronize()
    equal = all(torch.equal(a, b) for net in ('netG', 'netE', 'netD')
                for a, b in zip(getattr(plain.model, net).state_dict().values(),
                                getattr(dp.model, net).state_dict().values()))
    q.put(('ok', all_e, equal, dict(plain.last_losses) == dict(dp.last_losses)))
  except Exception as e:
    q.put(('error', repr(e), False, False))
    raise
  finally:
    dist.destroy_process_group()


def test_data_parallel_world_size_one_equals_plain_step():
  """A world-size-1 RCCL process group: every netE parameter sits in a G gradient bucket and two steps equal the plain
  trainer's bit for bit (codes addressed by n_global = rank * local_batch + i = i)."""
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  p = ctx.Process(target=_dp_worker, args=(q,))
  p.start()
  status, all_e, equal, losses = q.get(timeout=900)
  p.join(timeout=120)
  assert status == 'ok', all_e
  assert all_e, 'netE parameters missing from the G gradient buckets'
  assert equal and losses, 'data-parallel learned-codec step differs from the plain step'
