"""GPU: wide label sets -- ADE20K's num_labels=150 + don't-care + instance edge: 151 one-hot lanes, 152 semantic lanes, 155
input channels in 160 storage channels -- from the input builder up to the public calls.

  * jpdse_input_builder_wide and jpdse_insert_channels above 64 storage channels, bit for bit against the separate kernels
    (ops.onehot_edge + ops.concat_channels: the construction of tests/test_hip_ops.py's builder test) and against torch;
  * the three first-layer shapes at C = 155 (no layer had been run above 39 input channels) against fp64 arithmetic on the
    kernels' own operands: bf16 by the rounding contract of tests/bf16_contract.py, fp32 by the bounds of tests/hip_util.py;
  * a whole train step (global generator and LocalEnhancer) against the torch-CPU oracle and the reference's recorded step
    (tests/golden/wide_labels_ngf8.npz), with the tolerances tests/test_hip_step.py applies at 39 channels;
  * get_img, get_eval_metrics(per_class=True), the learned codec's round trip and --zero_sem at 151 classes."""
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

import jpdse_hip  # noqa: E402
from jpdse_hip import ops, F32, BF16, PAD_ZERO, PAD_REFLECT, ACT_NONE, ACT_LRELU  # noqa: E402
from jpdse_hip.ops import Act  # noqa: E402
from jpdse_hip.layers import HipConv2d  # noqa: E402
from oracle.ctu_cpu import model as omodel, nets as onets  # noqa: E402

import bf16_contract as bc  # noqa: E402
from bf16_contract import Cand  # noqa: E402
import class_metrics_ref as cref  # noqa: E402
import msssim_ref  # noqa: E402
import test_hip_step as ths  # noqa: E402
import wide_labels_util as wl  # noqa: E402
from hip_util import DEV, DTYPES, RTOL, assert_close, quantize_like, to_act, to_nchw  # noqa: E402

# tests/test_hip_step.py's bounds for the same quantities at 39 input channels, restated by name
LOSS_TOL = ths.LOSS_TOL              # 1e-3: fp32 losses against the oracle and the reference's step 0 (--zero_sem: relative to
                                     # max(1, |loss|), as tests/test_hip_zero_flags.py compares the same six losses)
WEIGHT_TOL = ths.WEIGHT_TOL          # 3e-3: post-Adam weights, relative L2 (_check_weights)
BF16_LOSS_TOL = 5e-2                 # test_bf16_step_tracks_fp32 (the same ngf 8, 32x64 configuration): bf16 losses vs the oracle
BF16_GRAD_COS, BF16_GRAD_NORM = 0.85, 6e-2   # test_bf16_local_enhancer_full_width_in_situ: bf16 vs fp32 HIP weight gradients
IMG_TOL = 4e-4                       # _golden_steps: get_img against the oracle (assert_close)
NET_TOL = 2e-4                       # tests/test_hip_zero_flags.py: get_img against a reference golden, max-abs over the max


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  jpdse_hip.require_gpu(0)


@pytest.fixture(scope='module')
def gold(golden_dir):
  return wl.load_gold(golden_dir)


def G(seed):
  return torch.Generator().manual_seed(seed)


# ---- the input builder ------------------------------------------------------------------------------------------------------
N_B, H_B, W_B = 3, 20, 44            # ragged; corners, borders and interior pixels all present


def _builder_maps(nlab):
  """Label ids over [0, nlab + 3): the don't-care id nlab - 1, and ids >= nlab (nlab itself is the EDGE lane's index) that
  must light no lane; instance blocks of 3x5 pixels so that every pixel class has edge and non-edge members."""
  g = G(nlab)
  lab = torch.randint(0, nlab + 3, (N_B, 1, H_B, W_B), generator=g)
  lab[0, 0, 0, 0], lab[0, 0, 0, 1], lab[0, 0, 0, 2], lab[0, 0, 0, 3] = nlab - 1, nlab, nlab + 2, 0
  lab[2, 0, H_B - 1, W_B - 1] = nlab - 1
  ins = torch.randint(0, 6, (N_B, 1, -(-H_B // 3), -(-W_B // 5)), generator=g)
  ins = ins.repeat_interleave(3, 2).repeat_interleave(5, 3)[:, :, :H_B, :W_B].contiguous() * 1000 + 7
  return lab.float().contiguous(), ins.long()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('cs', [72, 160, 264])
def test_wide_builder_equals_onehot_edge_plus_concats(cs, dtype):
  # 72: the first width jpdse_input_builder refuses (65 labels + edge + 3); 160: ADE20K (151 + 1 + 3 = 155); 264: 255 labels +
  # edge + 3 = 259, more than 32 vectors per pixel in bf16 and more than 64 in fp32
  nlab = {72: 65, 160: wl.N_ONEHOT, 264: 255}[cs]
  C, c0 = nlab + 4, nlab + 1
  assert ops.cpad(C) == cs and cs > 64
  lab_c, ins_c = _builder_maps(nlab)
  lab, ins = lab_c.to(DEV), ins_c.to(DEV)
  g = G(cs)
  imgs = [to_act(quantize_like(torch.randn(N_B, 3, H_B, W_B, generator=g), dtype), dtype) for _ in range(3)]
  base = ops.onehot_edge(lab, ins, nlab, C, dtype)
  want = [ops.concat_channels(base, im, c0, base.empty_like()) for im in imgs]
  # the yardstick itself against torch at this width: one-hot lanes, the edge lane, everything behind it zero
  bn = to_nchw(base)
  onehot = torch.zeros(N_B, nlab + 3, H_B, W_B).scatter_(1, lab_c.long(), 1.0)[:, :nlab]
  assert torch.equal(bn[:, :nlab], onehot) and torch.equal(bn[:, nlab:nlab + 1], omodel.edge_map(ins_c))
  assert (base.t[..., nlab + 1:] == 0).all() and 0 < bn[:, nlab].sum() < N_B * H_B * W_B
  assert (bn[:, :nlab].sum(1) == 0).any(), 'an id >= num_labels must light no lane'

  def fresh(n):
    out = [base.empty_like() for _ in range(n)]
    for d in out:
      d.t.fill_(7.0)                  # every lane must be written
    return out
  dsts = fresh(3)
  ops.input_builder(lab, ins, nlab, dsts, [imgs[0], imgs[1], None], c0)          # three destinations, one without an image
  assert torch.equal(dsts[0].t, want[0].t) and torch.equal(dsts[1].t, want[1].t)
  assert torch.equal(dsts[2].t, base.t)
  two = fresh(2)
  ops.input_builder(lab, ins, nlab, two, [None, imgs[2]], c0)                    # two: the null image first
  assert torch.equal(two[0].t, base.t) and torch.equal(two[1].t, want[2].t)
  one = fresh(1)
  ops.input_builder(lab, ins, nlab, one, [imgs[1]], c0)                          # one: the learned codec's G input (c0 = label_nc, 3 lanes)
  assert torch.equal(one[0].t, want[1].t)
  one = fresh(1)
  ops.input_builder(lab, ins, nlab, one, [None], c0)
  assert torch.equal(one[0].t, base.t)
  # insert_channels at this width against a torch slice assignment
  ops.insert_channels(dsts[2], imgs[2], c0)
  assert torch.equal(dsts[2].t, want[2].t)
  ref = base.t.clone()
  ref[..., c0:c0 + 3] = imgs[0].t[..., :3]
  assert torch.equal(ops.insert_channels(Act(base.t.clone(), C), imgs[0], c0).t, ref)
  ref = torch.full_like(base.t, 3.0)
  mid = Act(ref.clone(), C)
  ref[..., 6:9] = imgs[1].t[..., :3]                                               # a range that straddles two 16-byte vectors in bf16
  assert torch.equal(ops.insert_channels(mid, imgs[1], 6).t, ref)


def test_wide_builder_batch_slices_of_one_discriminator_tensor():
  """The train step's call: G's input and the two halves of ONE [2B] discriminator tensor as the three destinations."""
  nlab, C, c0 = wl.N_ONEHOT, wl.INPUT_NC, wl.LABEL_NC
  lab_c, ins_c = _builder_maps(nlab)
  lab, ins = lab_c.to(DEV), ins_c.to(DEV)
  src, real = [to_act(quantize_like(torch.randn(N_B, 3, H_B, W_B, generator=G(s)), BF16), BF16) for s in (1, 2)]
  base = ops.onehot_edge(lab, ins, nlab, C, BF16)
  g_in, d_in = Act.empty(N_B, H_B, W_B, C, BF16, DEV), Act.empty(2 * N_B, H_B, W_B, C, BF16, DEV)
  g_in.t.fill_(7.0)
  d_in.t.fill_(7.0)
  ops.input_builder(lab, ins, nlab, [g_in, d_in.batch_slice(N_B, 2 * N_B), d_in.batch_slice(0, N_B)], [src, real, None], c0)
  assert torch.equal(g_in.t, ops.concat_channels(base, src, c0, base.empty_like()).t)
  assert torch.equal(d_in.t[N_B:], ops.concat_channels(base, real, c0, base.empty_like()).t) and torch.equal(d_in.t[:N_B], base.t)


# ---- the first layers at C = 155 --------------------------------------------------------------------------------------------
# tests/test_hip_ops.py's thin_ragged and thinf_s2_40 rows with 155 input channels
LAYERS = [('wide_thin_ragged', 2, 10, 150, 155, 64, 7, 1, 3, PAD_REFLECT, ACT_NONE),
          ('wide_thinf_s2',    2, 20, 150, 155, 64, 4, 2, 2, PAD_ZERO,    ACT_LRELU)]


def _dbl(a):
  return to_nchw(a).double()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', LAYERS, ids=[c[0] for c in LAYERS])
def test_first_layers_at_155_input_channels(case, dtype):
  """Forward and weight gradient of G's 7x7 reflect conv and of PatchGAN layer 0 (bias + LeakyReLU), and layer 0's data
  gradient w.r.t. the image channels [152, 155) (HipConv2d.bwd_input_slice), on operands that are bf16 values in both dtypes."""
  name, N, H, W, C, K, k, st, pad, mode, act = case
  x, w, b, gy = bc.conv_case_inputs(case, 0)
  layer = HipConv2d(C, K, k, st, pad, mode, act=act, apply_bias=True, dtype=dtype, device=DEV)
  with torch.no_grad():
    layer.weight.copy_(w)
    layer.bias.copy_(b)
  d = ops.conv_desc(dtype, N, H, W, C, K, k, k, st, pad, mode, act, bc.SLOPE)
  xa, dya = to_act(x, dtype), to_act(gy, dtype)
  assert xa.Cs == 160
  y, ctx = layer.fwd(xa)
  dz = dya if act == ACT_NONE else ops.act_bwd(y, dya, act, bc.SLOPE)
  dw = torch.empty((K, k, k, C), dtype=torch.float32, device=DEV)
  ops.conv_wgrad(d, xa, dz, dw)
  dx = layer.bwd_input_slice(ctx, dz, wl.LABEL_NC, wl.INPUT_NC, dy_is_dz=True) if st == 2 else None
  torch.cuda.synchronize()
  assert (y.t[..., K:] == 0).all()

  y64, S, n = bc.fwd_reference(x, w, b, st, pad, mode, act)
  dz64 = _dbl(dz)
  dw64 = bc.wgrad64(x.double(), dz64, w.shape, st, pad, mode)
  if dtype == BF16:
    bc.assert_bf16_contract(_dbl(y), [Cand(y64)], S, n, name + ' fwd')
  else:
    assert_close(_dbl(y), y64, RTOL[F32], name + ' fwd')
  bc.assert_fp32_vs_fp64(dw.permute(0, 3, 1, 2).cpu(), dw64, name + ' wgrad')
  if dx is not None:
    assert dx.C == 3
    _, cands, S, n = bc.dgrad_reference(dz64, w[:, wl.LABEL_NC:wl.INPUT_NC].double(), (N, 3, H, W), st, pad, mode)
    if dtype == BF16:
      bc.assert_bf16_contract(_dbl(dx), cands, S, n, name + ' data gradient, image channels')
    else:
      assert_close(_dbl(dx), cands[0].pre, RTOL[F32], name + ' data gradient, image channels')


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_avgpool_at_155_channels(dtype):
  """The 3x3 stride-2 average pool that feeds the second PatchGAN scale, forward and backward, on an odd size."""
  H, W = 9, 13
  x = quantize_like(torch.randn(2, wl.INPUT_NC, H, W, generator=G(155)), dtype)
  xr = x.double().requires_grad_(True)
  y_ref = onets.avgpool3s2(xr)
  gy = quantize_like(torch.randn(y_ref.shape, generator=G(1)), dtype)
  y_ref.backward(gy.double())
  y = ops.avgpool3s2_fwd(to_act(x, dtype))
  assert y.Cs == 160 and (y.t[..., wl.INPUT_NC:] == 0).all()
  assert_close(to_nchw(y), y_ref.detach(), RTOL[dtype], 'avgpool fwd, 155 channels')
  dx = ops.avgpool3s2_bwd(to_act(gy, dtype), H, W)
  assert_close(to_nchw(dx), xr.grad, RTOL[dtype], 'avgpool bwd, 155 channels')


# ---- the whole step -----------------------------------------------------------------------------------------------------------
def _trainer(sd_G, sd_D, dtype='fp32', **over):
  from ctu.trainers import get_trainer
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, compute_dtype=dtype, **dict(wl.NET, **over))
  tr = get_trainer(opt)(opt, 'train')
  tr.model.netG.load_state_dict(sd_G)
  tr.model.netD.load_state_dict(sd_D)
  return tr


def _oracle(sd_G, sd_D, cls=omodel.OracleTrainer, **over):
  return cls(omodel.default_opt(**dict(wl.NET, **over)), sd_G=sd_G, sd_D=sd_D)


def _fp32_step_against_oracle(tr, ora, xd, what):
  """One step from identical weights, held to what tests/test_hip_step.py::_golden_steps holds step 0 to."""
  assert tr.model.n_onehot == 151 and tr.model.label_nc == 152
  tr.step(wl.clone(xd))
  ths._check_grads(tr, ora, xd, what)              # every weight tensor, G's and D's first convs and the deep layers included
  ora.step(wl.clone(xd))
  torch.cuda.synchronize()
  for k in omodel.LOSS_NAMES:
    print('%s: loss %s %.6f vs oracle %.6f' % (what, k, tr.last_losses[k], ora.last_losses[k]))
  np.testing.assert_allclose([tr.last_losses[k] for k in omodel.LOSS_NAMES], [ora.last_losses[k] for k in omodel.LOSS_NAMES],
                             rtol=LOSS_TOL, err_msg=what + ' vs oracle')
  ths._check_weights(tr, ora, WEIGHT_TOL, what)


def test_fp32_step_global_against_the_oracle_and_the_reference(gold):
  sd_G, sd_D = wl.weights(int(gold['seed']))
  tr, ora = _trainer(sd_G, sd_D), _oracle(sd_G, sd_D)
  xd = wl.batch(gold)
  _fp32_step_against_oracle(tr, ora, xd, 'wide global step')
  got = [tr.last_losses[k] for k in omodel.LOSS_NAMES]
  np.testing.assert_allclose(got, gold['losses'], rtol=LOSS_TOL, err_msg='vs the reference step')
  # the reference's own gradients of the label-count-dependent layers and one deep layer of each network
  pG, pD = dict(tr.model.netG.named_parameters()), dict(tr.model.netD.named_parameters())
  g64, d64 = None, None
  for key, params in (('gradG:', pG), ('gradD:', pD)):
    for f in [f for f in gold if f.startswith(key)]:
      direct = ths.rel_err(params[f[len(key):]].grad.cpu(), torch.from_numpy(gold[f]))
      print('wide global step: %s vs the reference, max-abs relative %.3e' % (f, direct))
      if direct > ths.GRAD_TOL:                     # _check_grads' second route: as close to fp64 as the reference's fp32 is, x2
        if g64 is None:
          ora0 = _oracle(sd_G, sd_D)
          g64, d64 = ora0.grads_in_dtype(xd, torch.float64)
        r64 = (g64 if key == 'gradG:' else d64)[f[len(key):]]
        e_hip, e_ref = ths._l2rel(params[f[len(key):]].grad.cpu(), r64), ths._l2rel(torch.from_numpy(gold[f]), r64)
        assert e_hip <= max(ths.GRAD_TOL, 2.0 * e_ref), '%s: vs reference %.2e; vs fp64 HIP %.2e, reference %.2e' % (f, direct, e_hip, e_ref)


# The LocalEnhancer's trunk works at half resolution and down-samples four more times: at the fixture's 32x64 its ResnetBlocks
# would see a 1x2 map, which ReflectionPad2d(1) refuses (in the reference as here).  64x128 is the smallest size it runs at, and
# the size of tests/golden/step_local_ngf4.npz.
LOCAL_HW = (64, 128)


def test_fp32_step_local_enhancer_against_the_oracle():
  kw = dict(netG='local', ngf=4)
  sd_G, sd_D = wl.weights(77, **kw)
  assert sum(1 for v in sd_G.values() if v.dim() == 4 and v.shape[1] == 155) == 2      # the global trunk's and the enhancer's first convs
  tr, ora = _trainer(sd_G, sd_D, **kw), _oracle(sd_G, sd_D, **kw)
  _fp32_step_against_oracle(tr, ora, wl.wide_batch(2, *LOCAL_HW, seed=5), 'wide local step')


@pytest.mark.parametrize('netG', ['global', 'local'])
def test_bf16_step_tracks_fp32_and_the_oracle(gold, netG):
  kw = dict(netG='local', ngf=4) if netG == 'local' else {}
  sd_G, sd_D = wl.weights(int(gold['seed']), **kw)
  xd = wl.wide_batch(2, *LOCAL_HW, seed=6) if netG == 'local' else wl.batch(gold)
  tr32, tr16, ora = _trainer(sd_G, sd_D, **kw), _trainer(sd_G, sd_D, 'bf16', **kw), _oracle(sd_G, sd_D, **kw)
  tr32.step(wl.clone(xd))
  tr16.step(wl.clone(xd))
  ora.step(wl.clone(xd))
  torch.cuda.synchronize()
  for k in omodel.LOSS_NAMES:
    a, b, o = tr16.last_losses[k], tr32.last_losses[k], float(ora.last_losses[k])
    print('wide bf16 %s step: loss %s bf16 %.6f fp32 %.6f oracle %.6f' % (netG, k, a, b, o))
    assert abs(a - b) <= BF16_LOSS_TOL * max(abs(b), 1e-3), (k, a, b)
    assert abs(a - o) <= BF16_LOSS_TOL * max(abs(o), 1e-3), ('bf16 vs oracle', k, a, o)
    assert abs(b - o) <= LOSS_TOL * max(abs(o), 1e-3), ('fp32 vs oracle', k, b, o)
  cos = lambda a, b: float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))
  # the first convs (the only weights whose shape depends on the label count; the LocalEnhancer has two) and one deep layer
  first_g = [k for k, v in sd_G.items() if v.dim() == 4 and v.shape[1] == wl.INPUT_NC]
  keys = dict(netG=first_g + ['model.10.weight'], netD=['scale0_layer0.0.weight', 'scale1_layer0.0.weight', 'scale0_layer2.0.weight'])
  for net in ('netG', 'netD'):
    p32 = dict(getattr(tr32.model, net).named_parameters())
    p16 = dict(getattr(tr16.model, net).named_parameters())
    for k in keys[net]:
      p = p16[k]
      a, b = p.grad.detach().cpu().double().flatten(), p32[k].grad.detach().cpu().double().flatten()
      print('wide bf16 %s step: %s %s cosine %.4f norm ratio %.4f' % (netG, net, k, cos(a, b), float(a.norm() / b.norm())))
      assert cos(a, b) >= BF16_GRAD_COS, '%s %s: bf16 vs fp32 weight-gradient cosine %.4f' % (net, k, cos(a, b))
      assert abs(float(a.norm() / b.norm()) - 1.0) < BF16_GRAD_NORM, (net, k)


def test_two_identical_steps_give_identical_losses(gold):
  sd_G, sd_D = wl.weights(int(gold['seed']))
  xd = wl.batch(gold)
  runs = []
  for _ in range(2):
    tr = _trainer(sd_G, sd_D, 'bf16')
    tr.step(wl.clone(xd))
    torch.cuda.synchronize()
    runs.append((dict(tr.last_losses), tr.model.netG.state_dict()['model.1.weight'].clone(),
                 tr.model.netD.state_dict()['scale1_layer0.0.weight'].clone()))
  assert runs[0][0] == runs[1][0]
  assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ---- the public calls ---------------------------------------------------------------------------------------------------------
def _img_close(got, want, what):
  got, want = got.detach().cpu().double(), torch.as_tensor(want).double()
  err, scale = (got - want).abs().max().item(), want.abs().max().item()
  print('%s: get_img max abs error %.3e, bound %.3e' % (what, err, NET_TOL * scale))
  assert err <= NET_TOL * scale, '%s: get_img differs by %.3e (bound %.3e)' % (what, err, NET_TOL * scale)


def test_get_img_and_get_eval_loss_against_the_oracle_and_the_reference(gold):
  sd_G, sd_D = wl.weights(int(gold['seed']))
  tr, ora = _trainer(sd_G, sd_D), _oracle(sd_G, sd_D)
  xd = wl.batch(gold)
  img = tr.get_img(wl.clone(xd))
  assert tuple(img.shape) == (2, 3, 32, 64) and img.is_cuda
  assert_close(img.cpu(), ora.get_img(wl.clone(xd)), IMG_TOL, 'wide get_img')
  _img_close(img, gold['get_img'], 'wide get_img vs the reference')
  np.testing.assert_allclose(float(tr.get_eval_loss(wl.clone(xd))), ora.get_eval_loss(wl.clone(xd)), rtol=1e-3)
  # a ragged size and other labels
  xd = wl.wide_batch(3, 48, 80, seed=9)
  assert_close(tr.get_img(wl.clone(xd)).cpu(), ora.get_img(wl.clone(xd)), IMG_TOL, 'wide get_img 48x80')


def test_get_eval_metrics_reports_151_classes():
  """176x176 is the smallest size MS-SSIM accepts.  Exact against tests/class_metrics_ref.py on get_img's output."""
  sd_G, sd_D = wl.weights(4321)
  tr = _trainer(sd_G, sd_D)
  opt = tr.opt
  xd = wl.wide_batch(2, 176, 176, seed=9, cell=8)
  plain = tr.get_eval_metrics(wl.clone(xd))
  m = tr.get_eval_metrics(wl.clone(xd), per_class=True)
  assert 'per_class' not in plain and set(m) == set(plain) | {'per_class'} and torch.equal(m['raw'], plain['raw'])
  img = tr.get_img(wl.clone(xd))
  qf = msssim_ref.quantise(img.cpu().numpy(), opt.normalize_mean, opt.normalize_std)
  qr = msssim_ref.quantise(xd['image'].numpy(), opt.normalize_mean, opt.normalize_std)
  n = tr.model.n_onehot
  assert n == 151
  want = cref.table(qf, qr, xd['label'].numpy(), n)
  r, w = m['per_class'], cref.per_class(want)
  assert np.array_equal(r['raw'].numpy(), want)
  assert r['unlabelled'] == 0 and r['pixels'].sum().item() == 2 * 176 * 176
  assert r['pixels'][150].item() > 0 and r['pixels'][0].item() > 0 and int((r['pixels'] > 0).sum()) > 100
  for k in ('pixels', 'l1', 'mse'):
    assert tuple(r[k].shape) == (151,) and tuple(r['per_image'][k].shape) == (2, 151)
    assert np.array_equal(r[k].numpy(), w[k], equal_nan=True) and np.array_equal(r['per_image'][k].numpy(), w['per_image'][k], equal_nan=True)
  assert np.allclose(r['psnr'].numpy(), w['psnr'], rtol=1e-14, atol=0, equal_nan=True)   # log10 of two libms: a few ulp


def _codec_trainer(dtype, seed=31):
  from ctu.trainers import get_trainer
  opt = omodel.default_opt(gpu_ids=[0], print_losses=False, compute_dtype=dtype, no_feat_encoding=False,
                           no_encoder_binarization=False, feat_num=3, nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32,
                           **wl.NET)
  torch.manual_seed(seed)
  return get_trainer(opt)(opt, 'train')


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_learned_codec_round_trip_at_151_classes(dtype):
  """decode(get_code(x), labels) == get_img(x) in eval mode, bit for bit, as tests/test_hip_decode_golden.py asserts at 35
  labels (precondition, as there: the eval code holds no exact zero); and one training step runs."""
  tr = _codec_trainer(dtype)
  assert tr.model.netE is not None and tr.model.label_nc + tr.model.feat_nc == 155
  xd = wl.wide_batch(2, 64, 128, seed=12)
  with torch.no_grad():
    tr.eval()
    zeros = ops.code_stats(tr.model._code_act(wl.clone(xd)))[:, 1]
  assert bool((zeros == 0).all()), 'precondition: the eval code of this batch holds an exact zero'
  want = tr.get_img(wl.clone(xd))
  packed, plain = tr.get_code(wl.clone(xd), packed=True), tr.get_code(wl.clone(xd))
  assert packed.dtype == torch.uint8 and tuple(packed.shape) == (2, 128) and tuple(plain.shape) == (2, 1024)
  rx = dict(label=xd['label'].clone(), instance=xd['instance'].clone())
  got = tr.decode(packed, rx)
  assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
  assert torch.equal(tr.decode(plain.cpu(), rx), want)
  ret = tr.step(wl.clone(xd))
  torch.cuda.synchronize()
  assert np.isfinite(ret) and all(np.isfinite(v) for v in tr.last_losses.values())
  grads = [p.grad for p in tr.model.netE.parameters() if p.grad is not None]
  assert grads and all(bool(torch.isfinite(g).all()) for g in grads)


def test_zero_sem_at_151_classes_against_the_oracle(gold):
  """--zero_sem: G's 152 semantic lanes are blank, D keeps them (wl.ZeroSemOracle; pinned to the reference's --zero_sem record
  at 36 lanes by tests/test_wide_labels_host.py)."""
  sd_G, sd_D = wl.weights(int(gold['seed']))
  tr = _trainer(sd_G, sd_D, zero_sem=True)
  ora = _oracle(sd_G, sd_D, cls=wl.ZeroSemOracle)
  xd = wl.batch(gold)
  img = tr.get_img(wl.clone(xd))
  assert_close(img.cpu(), ora.get_img(wl.clone(xd)), IMG_TOL, 'wide --zero_sem get_img')
  plain = _trainer(sd_G, sd_D)
  assert (plain.get_img(wl.clone(xd)) - img).abs().max().item() > 1e-2          # G's semantics are really gone
  tr.step(wl.clone(xd))
  ora.step(wl.clone(xd))
  plain.step(wl.clone(xd))
  torch.cuda.synchronize()
  for k in omodel.LOSS_NAMES:
    print('wide --zero_sem step: loss %s %.6f vs oracle %.6f' % (k, tr.last_losses[k], ora.last_losses[k]))
    assert abs(tr.last_losses[k] - ora.last_losses[k]) <= LOSS_TOL * max(1.0, abs(ora.last_losses[k])), (k, tr.last_losses[k], ora.last_losses[k])
  # D's semantics are not: the real half of the discriminator input is the unablated run's, so D_real is that run's
  assert abs(tr.last_losses['D_real'] - plain.last_losses['D_real']) <= 1e-6 * abs(plain.last_losses['D_real'])
  assert abs(tr.last_losses['D_fake'] - plain.last_losses['D_fake']) > 1e-4 * abs(plain.last_losses['D_fake'])
  for flag in ('zero_ins', 'zero_vis'):                                        # the other two ablation inputs run at this width
    t = _trainer(sd_G, sd_D, **{flag: True})
    assert tuple(t.get_img(wl.clone(xd)).shape) == (2, 3, 32, 64)
    assert np.isfinite(t.step(wl.clone(xd)))
