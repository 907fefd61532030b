"""GPU: the context-model rate term (jpdse_code_rate_loss, --lambda_rate, get_context_rate).

The kernels against tests/code_rate_ref.py (float64 numpy, written from the definition) on the inputs of the entropy-coder
tests; the train step with the rate term against the step without it (bit for bit where the term must not reach) and against
a torch-CPU composition (CodecOracle plus scale * dR/dt at the tanh output); get_context_rate against the reference applied
to get_code, and below the coded size."""
import ctypes
import functools
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
from jpdse_hip import F32, BF16, ops  # noqa: E402
from oracle.ctu_cpu import model as omodel  # noqa: E402

import code_rate_ref as ref  # noqa: E402
import entropy_cases as cases  # noqa: E402

# [N, C, h, w]: one symbol; one row; one column; the step test's code; two full lane groups and a tail of two lanes, with
# CPAD(C) > C; three images, several row chunks, w no multiple of the 32-bit word
SHAPES = [(1, 1, 1, 1), (1, 3, 1, 37), (1, 3, 9, 1), (2, 32, 4, 8), (1, 130, 5, 7), (3, 64, 16, 33)]
VALUE_TOL = 1e-3          # the project's fp32 parity bound, relative
GRAD_ATOL = 1e-3          # of max |g64|; bf16 adds one rounding of the stored value: 2^-8 |g64| (DESIGN.md 4.6's form)
SCALE = 0.75


def _stored(x, dtype):
  return x.to(torch.bfloat16).float() if dtype == BF16 else x.float()


def _act(x_nchw, dtype):
  return ops.nchw_to_nhwc(x_nchw.float().contiguous().cuda(), dtype)


def _pixels(shape):
  return 256 * shape[2] * shape[3]          # the image behind a code at 1 / 16 of its resolution


@functools.lru_cache(maxsize=None)
def _case(shape, kind, dtype):
  """(b, t, soft reference, hard reference): computed once per case, never modified."""
  b = cases.make_input(shape, kind)
  g = torch.Generator().manual_seed(1000 + SHAPES.index(shape))
  t = _stored((torch.rand(shape, generator=g) * 2 - 1) * (1 - 2 ** -7), dtype)      # uniform in (-1, 1), as the device stores it
  tn = t.double().numpy()
  return b, t, ref.rate(b, tn, _pixels(shape), SCALE), ref.rate(b, None, _pixels(shape), SCALE)


def _check_grad(got, want, dtype, what):
  bound = GRAD_ATOL * np.abs(want).max() + (2.0 ** -8 * np.abs(want) if dtype == BF16 else 0.0)
  err = np.abs(got - want)
  print('%s: worst grad error %.3e of max |g64| %.3e' % (what, err.max(), np.abs(want).max()))
  assert np.all(err <= bound), '%s: gradient off by %.3e (max |g64| %.3e)' % (what, (err - bound).max(), np.abs(want).max())


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=cases.shape_id)
def test_kernels_match_the_float64_reference(shape, kind, dtype):
  b_np, t, soft, hard = _case(shape, kind, dtype)
  b = _act(torch.from_numpy(b_np), dtype)
  ta = _act(t, dtype)
  N, C = shape[0], shape[1]
  for mode, tt, want in (('soft', ta, soft), ('hard', None, hard)):
    what = '%s %s %s' % (cases.shape_id(shape), kind, mode)
    value, per_image, grad, counts = ops.code_rate_loss(b, tt, _pixels(shape), SCALE, want_grad=True, want_counts=True)
    assert np.array_equal(counts.cpu().numpy(), want['counts']), what + ': counts'
    R, pi = float(value.item()), per_image.cpu().double().numpy()
    print('%s: R %.6f (reference %.6f)' % (what, R, want['R']))
    assert abs(R - want['R']) <= VALUE_TOL * abs(want['R']), what
    assert np.all(np.abs(pi - want['per_image']) <= VALUE_TOL * np.abs(want['per_image'])), what
    assert torch.all(grad.t[..., C:] == 0), what + ': padding lanes of the gradient'
    _check_grad(ops.nhwc_to_nchw(grad).cpu().double().numpy(), want['grad'], dtype, what)
    # a second call: bit-identical value and gradient; without the gradient: the same value
    value2, per2, grad2, _ = ops.code_rate_loss(b, tt, _pixels(shape), SCALE, want_grad=True)
    assert torch.equal(value, value2) and torch.equal(per_image, per2) and torch.equal(grad.t, grad2.t), what
    value3, per3, none, none2 = ops.code_rate_loss(b, tt, _pixels(shape), SCALE, want_grad=False)
    assert none is None and none2 is None and torch.equal(value, value3) and torch.equal(per_image, per3), what


def test_gradient_padding_lanes_are_written_and_the_logical_lanes_only_once():
  """The C entry point on a pre-filled gradient buffer: the two padding lanes of a 130-channel code (CPAD 136) become 0 and
  nothing outside the tensor is touched (guard rows in front of and behind it keep their fill)."""
  shape = (1, 130, 5, 7)
  b_np, t, soft, _ = _case(shape, 'blob', F32)
  b, ta = _act(torch.from_numpy(b_np), F32), _act(t, F32)
  guard = 4
  buf = torch.full((shape[2] + 2 * guard, shape[3], 136), 7.0, dtype=torch.float32, device='cuda')
  grad = buf[guard:guard + shape[2]]
  out = torch.zeros(1, dtype=torch.float32, device='cuda')
  lib = jpdse_hip.lib()
  n = lib.jpdse_code_rate_workspace_size(*[shape[i] for i in (0, 2, 3, 1)])
  ws = ops.workspace(n, b.t.device)
  args = jpdse_hip.CodeRateArgs(F32, shape[0], shape[2], shape[3], shape[1], _pixels(shape), b.t.data_ptr(), ta.t.data_ptr(),
                                grad.data_ptr(), SCALE, out.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream)
  jpdse_hip.check(lib.jpdse_code_rate_loss(ctypes.byref(args)), 'code_rate_loss')
  torch.cuda.synchronize()
  assert torch.all(buf[:guard] == 7.0) and torch.all(buf[guard + shape[2]:] == 7.0)
  assert torch.all(grad[..., 130:] == 0)
  got = grad[..., :130].permute(2, 0, 1).unsqueeze(0).cpu().double().numpy()
  _check_grad(got, soft['grad'], F32, 'pre-filled buffer')
  assert abs(out.item() - soft['R']) <= VALUE_TOL * soft['R']


# =============================================================================================
# the train step
# =============================================================================================
def _trainer(seed=1234, **over):
  from test_hip_learned_codec import _codec_pair
  return _codec_pair(seed=seed, **over)


def _grads(net):
  return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


FIRST_HALF = ('model.1.', 'model.4.', 'model.7.', 'model.10.', 'model.13.', 'model.16.')      # up to the binarizer's conv


def _step(xd, u, capture=None, **over):
  """One step of a fresh trainer (same seed, same weights, same noise): (trainer, oracle, losses, grads of G, grads of E)."""
  tr, ora, _ = _trainer(**over)
  tr.model.netE._binarizer.noise_override = u.cuda()
  if capture is not None:
    real = ops.code_rate_loss

    def spy(b, t, pixels, scale=1.0, **kw):
      capture.append((b, t, pixels, scale))
      return real(b, t, pixels, scale, **kw)
    ops.code_rate_loss = spy
  try:
    tr.step(xd)
  finally:
    if capture is not None:
      ops.code_rate_loss = real
  torch.cuda.synchronize()
  return tr, ora, dict(tr.last_losses), _grads(tr.model.netG), _grads(tr.model.netE)


@pytest.fixture(scope='module')
def step_runs():
  """The three steps every step test reads: no attribute, lambda_rate 0, lambda_rate 0.5 -- one batch, one noise tensor."""
  xd = omodel.synthetic_batch(2, 64, 128, seed=41)
  u = torch.rand(2, 32, 4, 8, generator=torch.Generator().manual_seed(8))
  calls = []
  plain = _step(xd, u)
  zero = _step(xd, u, lambda_rate=0.0)
  rate = _step(xd, u, capture=calls, lambda_rate=0.5)
  return dict(xd=xd, u=u, plain=plain, zero=zero, rate=rate, calls=calls)


def _same(a, b):
  return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_lambda_rate_zero_is_the_step_without_the_flag(step_runs):
  _, _, l0, g0, e0 = step_runs['plain']
  _, _, l1, g1, e1 = step_runs['zero']
  assert l0 == l1 and 'G_Rate' not in l1 and list(l1.keys()) == list(omodel.LOSS_NAMES)
  assert _same(g0, g1) and _same(e0, e1)


def test_rate_term_reaches_the_binarizer_conv_and_the_first_half_only(step_runs):
  _, _, l0, g0, e0 = step_runs['zero']
  tr, _, l1, g1, e1 = step_runs['rate']
  assert list(l1.keys()) == list(omodel.LOSS_NAMES) + ['G_Rate']
  for k in omodel.LOSS_NAMES:
    assert l0[k] == l1[k], k
  assert _same(g0, g1), 'the rate term changed a generator gradient'
  second = [k for k in e0 if not k.startswith(FIRST_HALF)]
  first = sorted(k for k in e0 if k.startswith(FIRST_HALF) and k.endswith('.weight'))
  assert first == ['model.1.weight', 'model.10.weight', 'model.13.weight', 'model.16.conv.weight', 'model.4.weight',
                   'model.7.weight']
  assert {'model.17.weight', 'model.20.weight', 'model.23.weight', 'model.26.weight', 'model.30.weight',
          'model.30.bias'} <= set(second)
  for k in second:
    assert torch.equal(e0[k], e1[k]), 'the rate term reached ' + k
  for k in first:
    assert not torch.equal(e0[k], e1[k]), 'the rate term did not reach ' + k
  # G_Rate is the value of the call the step made: the same kernels on the step's own t and b give the same float
  (b, t, pixels, scale), = step_runs['calls']
  assert pixels == 64 * 128 and scale == 0.5 and (b.N, b.H, b.W, b.C) == (2, 4, 8, 32)
  value, _, _, _ = ops.code_rate_loss(b, t, pixels, scale, want_grad=False)
  assert l1['G_Rate'] == float(value.item())
  want = ref.rate(ops.nhwc_to_nchw(b).cpu().numpy(), ops.nhwc_to_nchw(t).cpu().double().numpy(), pixels)
  assert abs(l1['G_Rate'] - want['R']) <= VALUE_TOL * want['R']


def _oracle_step(ora, xd, u, lambda_rate, fp64=False):
  """One step of CodecOracle on the weights of `ora`, with lambda_rate * dR/dt (tests/code_rate_ref.py on the oracle's own t and
  bits) added at the tanh output: the oracle's autograd carries it through the binarizer's conv and the encoder's first half.
  fp64: no step, the gradients of loss_G evaluated in float64 instead (OracleTrainer.grads_in_dtype), as `grads_G`."""
  import test_hip_learned_codec as tlc

  class RateOracle(tlc.CodecOracle):

    def generate(self, input_label, src):
      E = {k[2:]: v for k, v in self.G.items() if k.startswith('E.')}
      feat, t = tlc.oracle_encoder(E, src, self.opt.n_downsample_E, train=True, u=u)
      self.last_margin = ((1 - t.detach()) / 2 - u).abs().min().item()
      bits = torch.where((1 - t.detach()) / 2 <= u, 1.0, -1.0).numpy()
      r = ref.rate(bits, t.detach().double().numpy(), src.shape[-2] * src.shape[-1], lambda_rate)
      self.last_rate = r['R']
      d_rate = torch.from_numpy(r['grad']).to(t.dtype)
      t.register_hook(lambda g: g + d_rate)
      self.draw += 1
      return tlc.nets.generator(self.G, tlc.nets.q(torch.cat((input_label, feat), dim=1)), self.cfg)

  rora = RateOracle(ora.opt, {k[2:]: v.detach() for k, v in ora.G.items() if k.startswith('E.')},
                    sd_G={k: v.detach() for k, v in ora.G.items() if not k.startswith('E.')},
                    sd_D={k: v.detach() for k, v in ora.D.items()})
  if fp64:
    rora.grads_G, _ = rora.grads_in_dtype(xd, torch.float64)
  else:
    rora.step(xd, keep_grads=True)
  assert rora.last_margin > 1e-5, 'noise within 1e-5 of a threshold: pick another seed'
  return rora


def _rel_l2(got, want):
  return ((got - want).norm() / want.norm()).item()


def _first_half_weights(grads):
  return sorted(k for k in grads if k.startswith(FIRST_HALF) and k.endswith('.weight'))


# The oracle comparison of the whole gradient runs with the smooth losses only (LSGAN and an MSE distortion; --no_vgg_loss,
# --no_gan_feat_loss).  The L1 terms have sign() gradients: on a whole step two correct fp32 implementations differ by more than
# 1e-3 on some encoder tensors whatever this feature does (tests/test_hip_learned_codec_golden.py::_check_grads meets that with
# a float64 yardstick; here the default-loss step without the rate term is 4.5e-3 away from the oracle on model.1.weight, a
# tensor to which the rate term contributes 2.7e-3).  Under the default losses the rate term's own contribution is checked
# instead, see test_rate_term_contribution_matches_the_oracle_under_the_default_losses.
SMOOTH = dict(distortion_loss_fn='mse', no_vgg_loss=True, no_gan_feat_loss=True)


def test_rate_gradients_match_the_oracle_composition(step_runs):
  """The gradients of the binarizer's conv and of the encoder's first half against the oracle composition, relative L2 within
  test_hip_learned_codec.py's GRAD_TOL, and G_Rate against the reference on the oracle's own t and bits."""
  import test_hip_learned_codec as tlc
  xd, u = step_runs['xd'], step_runs['u']
  tr, ora, losses, _, e_hip = _step(xd, u, lambda_rate=0.5, **SMOOTH)
  rora = _oracle_step(ora, xd, u, 0.5)
  assert abs(losses['G_Rate'] - rora.last_rate) <= tlc.LOSS_TOL * rora.last_rate
  keys = _first_half_weights(e_hip)
  assert len(keys) == 6
  errs = {k: _rel_l2(e_hip[k].cpu().double(), rora.grads_G['E.' + k].double()) for k in keys}
  for k in keys:
    print('%s: relative L2 gradient error %.3e' % (k, errs[k]))
  for k in keys:
    assert errs[k] <= tlc.GRAD_TOL, '%s: relative L2 gradient error %.3e' % (k, errs[k])


def test_rate_term_contribution_matches_the_oracle_under_the_default_losses(step_runs):
  """Default losses: what the rate term adds to each gradient, g(lambda_rate 0.5) - g(lambda_rate 0) -- on the device the two
  steps share every bit of the backward pass down to the binarizer, in the oracle every operation, so the L1 terms' scatter
  cancels -- against the same difference of the oracle composition evaluated in float64, relative L2 within GRAD_TOL.  The
  device's difference of two fp32 gradients, of which it is the fraction f, carries their rounding over f (each element at
  least 2^-24 / f; the sums behind a weight gradient more): the float64 oracle keeps the other side of the comparison free of
  that, and the step being deterministic the figure does not move from run to run.  Measured on MI355X: 3.3e-5 (binarizer conv)
  to 2.7e-4 (model.1.weight, the 7x7 conv at full resolution); against the fp32 oracle's difference 4e-5 to 9e-4."""
  import test_hip_learned_codec as tlc
  xd, u = step_runs['xd'], step_runs['u']
  _, ora, _, _, e_rate = step_runs['rate']
  _, _, _, _, e_zero = step_runs['zero']
  with_rate, without = _oracle_step(ora, xd, u, 0.5, fp64=True), _oracle_step(ora, xd, u, 0.0, fp64=True)
  keys = _first_half_weights(e_rate)
  rows = []
  for k in keys:
    got = (e_rate[k] - e_zero[k]).cpu().double()
    want = (with_rate.grads_G['E.' + k] - without.grads_G['E.' + k]).double()
    share = (want.norm() / with_rate.grads_G['E.' + k].double().norm()).item()
    base = _rel_l2(e_zero[k].cpu().double(), without.grads_G['E.' + k].double())
    rows.append((k, _rel_l2(got, want), share, base))
    print('%s: rate contribution off by %.3e (relative L2); it is %.2e of the gradient; whole gradient without it vs the '
          'oracle: %.3e' % rows[-1])
  for k, err, share, _ in rows:
    assert 2.0 ** -24 / share <= 0.1 * tlc.GRAD_TOL, '%s: the rate term is too small a share (%.2e) to be resolved' % (k, share)
    assert err <= tlc.GRAD_TOL, '%s: rate contribution, relative L2 error %.3e' % (k, err)


def test_get_context_rate_matches_the_reference_and_stays_below_the_coded_rate(step_runs):
  tr, _, _, _, _ = step_runs['rate']
  xd = step_runs['xd']
  with torch.no_grad():
    got = tr.get_context_rate(xd)
  assert isinstance(got, float)
  code = tr.get_code(xd).cpu().numpy().reshape(2, 32, 4, 8)            # 0 / 1, NCHW flatten order
  want = ref.rate(code * 2.0 - 1.0, None, 64 * 128)['R']
  coded, raw = tr.get_coded_rate(xd)
  print('context rate %.6f bpp (reference %.6f), coded %.6f bpp, raw %.6f bpp' % (got, want, coded, raw))
  assert abs(got - want) <= VALUE_TOL * want
  assert got < coded
