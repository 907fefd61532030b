"""CPU-only checks of the MS-SSIM training loss (jpdse_msssim_loss): the entry point is declared and exported,
its workspace query answers without a device, every refusal comes with its text before any launch, the float64 yardstick of
the GPU test (tests/msssim_loss_ref.py) is pinned to closed forms, and the model's constructor takes the new flag value.
No device kernel is launched here."""
import ctypes
import os
import re

import pytest
import torch

import jpdse_hip
from jpdse_hip import F32, BF16
from oracle.ctu_cpu import model as omodel

import msssim_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('jpdse_msssim_loss_workspace_size', 'jpdse_msssim_loss')
MEAN, STD = (0.5, 0.5, 0.5), (1.0, 1.0, 1.0)


def test_new_symbols_are_declared_and_exported():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  L = jpdse_hip.lib()
  dev = ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NEW_SYMBOLS:
    assert name in declared, name + ' missing from include/jpdse.h'
    assert name in jpdse_hip.SIGNATURES
    assert hasattr(L, name) and hasattr(dev, name)
  assert L.jpdse_version() == 2
  from jpdse_hip import ops
  assert callable(ops.msssim_loss_fwd) and callable(ops.msssim_loss_fwd_bwd) and ops.MSSSIM_MIN_SIDE == 176


def test_workspace_query_answers_without_a_device():
  size = jpdse_hip.lib().jpdse_msssim_loss_workspace_size
  fwd, both = size(1, 176, 176, 3, 0), size(1, 176, 176, 3, 1)
  assert 0 < fwd < both
  assert size(4, 512, 1024, 3, 1) > size(1, 512, 1024, 3, 1)
  # both planes of every scale; with the gradient three scale-1 coefficient maps and the gradient planes on top
  assert size(1, 512, 1024, 3, 0) >= 2 * 3 * 4 * 512 * 1024 * 1.33
  assert size(1, 512, 1024, 3, 1) - size(1, 512, 1024, 3, 0) >= 3 * 3 * 4 * 502 * 1014
  for n, h, w, c in ((1, 175, 400, 3), (1, 400, 175, 3), (1, 256, 256, 4), (1, 256, 256, 1), (0, 256, 256, 3)):
    assert size(n, h, w, c, 0) == 0 and size(n, h, w, c, 1) == 0


def test_refusals_come_before_any_launch_with_their_texts():
  L = jpdse_hip.lib()
  dummy = (ctypes.c_double * 16)()
  p = ctypes.cast(dummy, ctypes.c_void_p).value
  m = (ctypes.c_double * 3)(*MEAN)
  s = (ctypes.c_double * 3)(*STD)

  def call(dtype=F32, n=1, h=256, w=256, c=3, fake=p, real=p, mean=m, std=s, out=p, dfake=None, nbytes=1 << 31):
    args = jpdse_hip.MsssimLossArgs(dtype, n, h, w, c, fake, real, mean, std, out, None, dfake, 1.0, p, nbytes, None)
    return L.jpdse_msssim_loss(ctypes.byref(args))
  assert L.jpdse_msssim_loss(None) == -1 and 'null argument struct' in jpdse_hip.last_error()
  null3 = ctypes.POINTER(ctypes.c_double)()
  for kw in (dict(fake=None), dict(real=None), dict(out=None), dict(mean=null3), dict(std=null3)):
    assert call(**kw) == -1 and 'null argument' in jpdse_hip.last_error(), kw
  assert call(c=4) == -1 and '3 channels only' in jpdse_hip.last_error()
  assert call(c=1) == -1 and '3 channels only' in jpdse_hip.last_error()
  assert call(dtype=BF16, h=175, w=512) == -1 and 'at least 176' in jpdse_hip.last_error()
  assert call(h=512, w=175) == -1 and 'at least 176' in jpdse_hip.last_error()
  assert call(dtype=7) == -1 and 'dtype' in jpdse_hip.last_error()
  assert call(h=16 * 65535 + 1, w=176) == -1 and 'tile grid' in jpdse_hip.last_error()
  # a short workspace: the forward's size does not cover a call that also asks for the gradient
  fwd = L.jpdse_msssim_loss_workspace_size(1, 256, 256, 3, 0)
  assert call(nbytes=1024) == -2 and 'workspace too small' in jpdse_hip.last_error()
  assert call(dfake=p, nbytes=fwd) == -2 and 'workspace too small' in jpdse_hip.last_error()
  with pytest.raises(jpdse_hip.JpdseError, match='176'):
    jpdse_hip.check(call(n=2, h=100, w=100), 'msssim_loss')


def test_model_constructor_takes_ms_ssim_and_names_all_three_otherwise(monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  # the value is checked before any network exists: with the GPU hidden, ms_ssim gets as far as the device check
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(ValueError, match='distortion_loss_fn must be l1, mse or ms_ssim'):
    Pix2PixHDModel(omodel.default_opt(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, distortion_loss_fn='psnr'))
  with pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
    Pix2PixHDModel(omodel.default_opt(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, distortion_loss_fn='ms_ssim'))


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def _noise(n, h, w, seed):
  return torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5


def test_yardstick_identical_images_give_loss_zero_and_constants_the_closed_form():
  x = _noise(1, 176, 180, 1)
  r = ref.loss(x, x.clone(), MEAN, STD)
  assert r['loss'].item() == 0.0 and torch.all(r['cs'] == 1.0) and torch.all(r['ssim'] == 1.0)
  a, b = 0.25, 0.75                                 # de-normalised values of two constant images
  fa, fb = torch.full((1, 3, 180, 176), a - 0.5, dtype=torch.float64), torch.full((1, 3, 180, 176), b - 0.5, dtype=torch.float64)
  r = ref.loss(fa, fb, MEAN, STD)
  lum = (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)
  assert abs(r['ms_ssim'].item() - lum ** ref.WEIGHTS[4]) < 1e-9
  assert abs(ref.C1 - 1e-4) < 1e-18 and abs(ref.C2 - 9e-4) < 1e-18
  with pytest.raises(ValueError):
    ref.loss(_noise(1, 175, 300, 2), _noise(1, 175, 300, 3), MEAN, STD)


def test_yardstick_gradient_matches_a_central_difference_and_the_zero_rule():
  real = _noise(2, 176, 176, 4)
  fake = real + 0.2 * _noise(2, 176, 176, 5)
  mean, std = (0.5, 0.4, 0.45), (1.0, 0.9, 1.1)
  r = ref.loss_and_grad(fake, real, mean, std)
  assert r['grad'].dtype == torch.float64 and r['grad'].shape == fake.shape
  for at in ((0, 1, 40, 7), (1, 2, 175, 175), (1, 0, 0, 90)):
    h = 1e-4
    up, dn = fake.clone(), fake.clone()
    up[at] += h
    dn[at] -= h
    fd = (ref.loss(up, real, mean, std)['loss'] - ref.loss(dn, real, mean, std)['loss']).item() / (2 * h)
    # the loss is of order 1: its fp64 rounding (a few 1.1e-16) over 2h, plus the O(h^2) truncation
    assert abs(fd - r['grad'][at].item()) <= 1e-4 * abs(fd) + 1e-11, at
  # image 1 anti-correlated with its original: cs_1 < 0, so ms_ssim_1 = 0 and its gradient vanishes; image 0 keeps its own
  real2 = real.clone()
  real2[1] = -fake[1]
  z = ref.loss_and_grad(fake, real2, mean, std)
  assert z['cs'][1, 0].item() < 0 and z['ms_ssim'][1].item() == 0.0
  assert torch.all(z['grad'][1] == 0) and torch.equal(z['grad'][0], r['grad'][0])
