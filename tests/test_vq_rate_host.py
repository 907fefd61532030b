"""Host tests of the rate term of the vector-quantizer bottleneck: the restated formulas of
tests/vq_rate_ref.py against float64 autograd, the G = 1 identity with S2HVQ.get_cross_entropy, the workspace query, the new
option and the refusals that must come before any network or device work.  No GPU."""
import argparse
import ctypes

import pytest
import torch

import jpdse_hip
import vq_util
import vq_rate_ref as ref
from test_vq_bottleneck_host import _codec_opts, _hide_device

SIGMA = 10.0


def _inputs(M, D, L, seed):
  g = torch.Generator().manual_seed(seed)
  scale = (SIGMA * D) ** -0.5
  x = (torch.rand(M, D, generator=g, dtype=torch.float64) * 2 - 1) * scale
  c = (torch.rand(L, D, generator=g, dtype=torch.float64) * 2 - 1) * scale
  dy = torch.randn(M, D, generator=g, dtype=torch.float64)
  return x, c, dy


# ---- the formulas ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 2, 1), (6, 3, 5, 3), (32, 8, 16, 4), (30, 4, 7, 30)], ids=str)
def test_restated_gradient_is_the_autograd_of_the_definition(shape):
  M, D, L, G = shape
  x, c, dy = _inputs(M, D, L, seed=M + 10 * L + G)
  x.requires_grad_(True)
  c.requires_grad_(True)
  denom, scale = 3.0 * M, 0.7
  value, hist = ref.rate(x, c, SIGMA, G, denom)
  y = vq_util.soft(x, c, SIGMA) @ c
  ((y * dy).sum() + scale * value).backward()
  # dhist by its formula is autograd's gradient of scale * rate w.r.t. the un-normalised sums
  h = hist.detach().clone().requires_grad_(True)
  (scale * ref.rate_of_hist(h, M // G, denom)).backward()
  dhist = ref.dhist_of(hist.detach(), M // G, denom, scale)
  assert torch.allclose(dhist, h.grad, rtol=1e-12, atol=1e-14)
  dx, dc = ref.quantize_bwd_grouped(dy, x.detach(), c.detach(), SIGMA, G, dhist)
  assert torch.allclose(dx, x.grad, rtol=1e-10, atol=1e-12 * float(x.grad.abs().max() + 1))
  assert torch.allclose(dc, c.grad, rtol=1e-10, atol=1e-12 * float(c.grad.abs().max() + 1))
  # without a dhist the grouped backward is 4.15's
  import vq_bottleneck_ref
  dx0, dc0 = ref.quantize_bwd_grouped(dy, x.detach(), c.detach(), SIGMA, G, None)
  dx1, dc1 = vq_bottleneck_ref.quantize_bwd(dy, x.detach(), c.detach(), SIGMA, None)
  assert torch.equal(dx0, dx1) and torch.equal(dc0, dc1)


def test_restated_values():
  # two groups of two vectors; group 0 sees centres (0, 1), group 1 sees centre 1 twice
  x = torch.tensor([[0.0], [1.0], [1.0], [1.0]], dtype=torch.float64)
  c = torch.tensor([[0.0], [1.0], [5.0]], dtype=torch.float64)
  value, hist = ref.rate(x, c, SIGMA, 2, 4.0, hard=True)
  assert hist.tolist() == [[1.0, 1.0, 0.0], [0.0, 2.0, 0.0]]
  assert abs(float(value) - 2.0 / 4.0) < 1e-15            # group 0: two indices of 1 bit each; group 1: 0 bits
  d = ref.dhist_of(hist, 2, 4.0)
  assert float(d[0, 2]) == 0.0 and float(d[1, 0]) == 0.0  # exactly 0 where hist is 0
  assert abs(float(d[1, 1]) + 1.0 / (4.0 * 0.6931471805599453)) < 1e-15


def test_one_group_is_the_cross_entropy_of_the_module():
  """G = 1: rate * denom / M = S2HVQ.get_cross_entropy(pmf, pmf) of the soft assignment's pmf, and the gradient of M times that
  entropy w.r.t. pmf * M is dhist / scale * denom."""
  from ctu.quantizers import S2HVQ
  M, D, L = 48, 4, 9
  x, c, _ = _inputs(M, D, L, seed=5)
  denom, scale = 17.0, 0.25
  value, hist = ref.rate(x, c, SIGMA, 1, denom)
  pmf = vq_util.pmf(vq_util.soft(x, c, SIGMA))
  ce = S2HVQ.get_cross_entropy(pmf.float(), pmf.float())
  assert abs(float(value) * denom / M - float(ce)) <= 1e-5 * float(ce)
  h = (pmf * M).detach().clone().requires_grad_(True)
  (M * vq_util.cross_entropy(h / M, h / M)).backward()
  assert torch.allclose(ref.dhist_of(hist, M, denom, scale)[0] / scale * denom, h.grad, rtol=1e-12, atol=1e-14)


# ---- the library's host side ------------------------------------------------------------------------------------------------
def test_workspace_query_needs_no_gpu_and_is_zero_outside_the_limits():
  q = jpdse_hip.lib().jpdse_vq_rate_workspace_size
  assert q(1048576, 8, 64, 16) >= 16 * 64 * 4 and q(1, 1, 2, 1) >= 2 * 4 and q(1040, 4, 16, 130) >= 130 * 16 * 4
  assert q(65536, 8, 512, 128) >= 65536 * 4                      # G * L at its limit
  for M, D, L, G in ((0, 8, 64, 1), (-16, 8, 64, 1), (16, 0, 64, 1), (16, 33, 64, 1), (16, 8, 1, 1), (16, 8, 513, 1),
                     (2 ** 22, 8, 512, 1), (16, 8, 64, 0), (16, 8, 64, -1), (16, 8, 64, 3), (16, 8, 64, 32),
                     (2 ** 16, 8, 512, 256), (1 << 20, 8, 2, 1 << 16)):
    assert q(M, D, L, G) == 0, (M, D, L, G)
  assert q(4112, 8, 64, 16) == q(4112, 8, 64, 16)


def test_null_args_are_refused_without_a_gpu():
  lib = jpdse_hip.lib()
  assert lib.jpdse_vq_rate_fwd(None) == -1 and jpdse_hip.last_error().startswith('vq_rate_fwd')
  assert lib.jpdse_vq_quantize_bwd_grouped(None) == -1 and jpdse_hip.last_error().startswith('vq_quantize_bwd_grouped')
  a = jpdse_hip.VqRateFwdArgs(0, 16, 8, 64, 3, 1.0, 0, None, None, 1.0, 1.0, None, None, None, None, 0, None)
  assert lib.jpdse_vq_rate_fwd(ctypes.byref(a)) == -1 and 'does not divide' in jpdse_hip.last_error()
  a = jpdse_hip.VqRateFwdArgs(0, 16, 8, 64, 4, 1.0, 0, None, None, 1.0, 0.0, None, None, None, None, 0, None)
  assert lib.jpdse_vq_rate_fwd(ctypes.byref(a)) == -1 and 'denom' in jpdse_hip.last_error()
  a = jpdse_hip.VqRateFwdArgs(0, 16, 8, 64, 4, 1.0, 0, None, None, float('nan'), 1.0, None, None, None, None, 0, None)
  assert lib.jpdse_vq_rate_fwd(ctypes.byref(a)) == -1 and 'scale' in jpdse_hip.last_error()
  a = jpdse_hip.VqRateFwdArgs(0, 16, 8, 64, 4, 1.0, 0, None, None, 1.0, 1.0, None, None, None, None, 0, None)
  assert lib.jpdse_vq_rate_fwd(ctypes.byref(a)) == -1 and 'null pointer' in jpdse_hip.last_error()
  b = jpdse_hip.VqQuantizeBwdGroupedArgs(0, 16, 8, 64, 0, 1.0, None, None, None, None, None, None, None, 0, None)
  assert lib.jpdse_vq_quantize_bwd_grouped(ctypes.byref(b)) == -1 and 'groups' in jpdse_hip.last_error()


# ---- the option ---------------------------------------------------------------------------------------------------------------
def test_new_option_defaults_to_zero():
  from ctu.models import get_option_setter
  parser = argparse.ArgumentParser()
  get_option_setter('pix2pixHD')(parser, True)
  a = parser.parse_args([])
  assert isinstance(a.lambda_vq_rate, float) and a.lambda_vq_rate == 0.0
  assert parser.parse_args(['--lambda_vq_rate', '0.5']).lambda_vq_rate == 0.5


@pytest.mark.parametrize('over', [dict(lambda_vq_rate=-0.5), dict(lambda_vq_rate=float('nan')), dict(lambda_vq_rate=float('inf')),
                                  dict(lambda_vq_rate=0.5, encoder_quantizer='binarizer'),
                                  dict(lambda_vq_rate=0.5, zero_vis=True)], ids=str)
def test_model_constructor_refuses_before_any_network_exists(over, monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  _hide_device(monkeypatch)
  with pytest.raises(ValueError, match='lambda_vq_rate'):
    Pix2PixHDModel(_codec_opts(**over))


def test_model_constructor_passes_its_checks_with_the_option(monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
    Pix2PixHDModel(_codec_opts(lambda_vq_rate=0.5))


def test_get_vq_rate_needs_the_vq_encoder():
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError('device work before the refusal'))
  m.__dict__.update(codec=None, preprocess=boom, _device=boom, _encoder_eval=boom)
  with pytest.raises(ValueError, match='encoder_quantizer') as err:
    m.get_vq_rate({})
  assert 'get_vq_rate' in str(err.value)
