"""CPU-only checks of the context-model rate term (jpdse_code_rate_loss): the float64 yardstick of the GPU
test (tests/code_rate_ref.py) against hand-worked arrays and against the bytes the reference coder emits, every refusal of
the entry point with its text before any launch, and the --lambda_rate flag with the model constructor's checks.  No device
kernel is launched here."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import F32, BF16
from oracle.ctu_cpu import model as omodel

import code_rate_ref as ref
import entropy_cases as cases
import entropy_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('jpdse_code_rate_workspace_size', 'jpdse_code_rate_loss')
L15, L43, L3 = math.log2(1.5), math.log2(4.0 / 3.0), math.log2(3.0)


# ---- the yardstick: three hand-worked arrays -----------------------------------------------------------------------------
def _expect_counts(pairs):
  """{ctx: (n0, n1)} -> int32 [16, 2]"""
  out = np.zeros((16, 2), dtype=np.int32)
  for k, v in pairs.items():
    out[k] = v
  return out


def test_yardstick_one_symbol():
  b = np.array([[[[1.0]]]])
  r = ref.rate(b, None, pixels=1)
  assert np.array_equal(r['counts'][0, 0], _expect_counts({0: (0, 1)}))
  # ctx 0 saw one 1: p1 = 2 / 3; every other context is empty: p1 = 1 / 2, one bit either way
  assert abs(r['cost1'][0, 0, 0] - L15) < 1e-12 and abs(r['cost0'][0, 0, 0] - L3) < 1e-12
  assert np.allclose(r['cost1'][0, 0, 1:], 1.0, atol=1e-12) and np.allclose(r['cost0'][0, 0, 1:], 1.0, atol=1e-12)
  assert abs(r['R'] - L15) < 1e-12 and abs(r['per_image'][0] - L15) < 1e-12
  # soft mode: e = 0.6 cost1 + 0.4 cost0, dR/dt = (cost1 - cost0) / 2 = -1 / 2 exactly; pixels and scale divide / multiply
  s = ref.rate(b, np.array([[[[0.2]]]]), pixels=4, scale=3.0)
  assert abs(s['R'] - (0.6 * L15 + 0.4 * L3) / 4.0) < 1e-12
  assert abs(s['grad'][0, 0, 0, 0] - 3.0 * (L15 - L3) / (2.0 * 4.0)) < 1e-12 and abs(L15 - L3 + 1.0) < 1e-12
  # an exact zero of the eval binarizer is bit 0
  z = ref.rate(np.array([[[[0.0]]]]), None, pixels=1)
  assert np.array_equal(z['counts'][0, 0], _expect_counts({0: (1, 0)})) and abs(z['R'] - L15) < 1e-12


def test_yardstick_two_by_three_stream():
  #   1 0 1      ctx   0  1  0         (left | up << 1 | upleft << 2 | upright << 3, zeros outside the frame)
  #   1 1 0            2 13  3
  b = np.array([[[[1, -1, 1], [1, 1, -1]]]], dtype=np.float64)
  bits, ctx = ref.contexts(b)
  assert np.array_equal(ctx[0, 0], [[0, 1, 0], [2, 13, 3]]) and np.array_equal(bits[0, 0], [[1, 0, 1], [1, 1, 0]])
  r = ref.rate(b, None, pixels=6)
  assert np.array_equal(r['counts'][0, 0], _expect_counts({0: (0, 2), 1: (1, 0), 2: (0, 1), 13: (0, 1), 3: (1, 0)}))
  assert abs(r['cost1'][0, 0, 0] - L43) < 1e-12          # two 1s in ctx 0: p1 = 3 / 4
  assert abs(r['cost0'][0, 0, 1] - L15) < 1e-12 and abs(r['cost1'][0, 0, 13] - L15) < 1e-12
  total = 2 * L43 + 4 * L15                               # = 3.169925 bits
  assert abs(r['bits_total'][0, 0] - total) < 1e-12 and abs(r['R'] - total / 6.0) < 1e-12
  # the gradient of the 0 at (0, 1): (cost1 - cost0)[ctx 1] = log2(3) - log2(1.5) = 1 bit
  assert abs(r['grad'][0, 0, 0, 1] - 1.0 / (2.0 * 6.0)) < 1e-12


def test_yardstick_all_ones_stream():
  b = np.ones((1, 1, 3, 3))
  bits, ctx = ref.contexts(b)
  assert np.array_equal(ctx[0, 0], [[0, 1, 1], [10, 15, 7], [10, 15, 7]])
  r = ref.rate(b, None, pixels=9)
  assert np.array_equal(r['counts'][0, 0], _expect_counts({0: (0, 1), 1: (0, 2), 10: (0, 2), 15: (0, 2), 7: (0, 2)}))
  total = L15 + 8 * L43                                   # = 3.905263 bits
  assert abs(r['bits_total'][0, 0] - total) < 1e-12 and abs(r['R'] - total / 9.0) < 1e-12
  # two images, two channels of the same stream: the per-image value doubles with the channels, R is the mean over images
  r2 = ref.rate(np.ones((2, 2, 3, 3)), None, pixels=9)
  assert np.allclose(r2['per_image'], 2 * total / 9.0, atol=1e-12) and abs(r2['R'] - 2 * total / 9.0) < 1e-12


# ---- the estimate stays below what the coder emits -----------------------------------------------------------------------
def _stream(kind, H, W):
  shape = (1, 1, H, W)
  if kind == 'blob0':                                     # 4 x 4 blocks of one sign each, no flips
    g = np.random.default_rng([7, H, W])
    coarse = g.standard_normal((1, 1, (H + 3) // 4, (W + 3) // 4))
    return np.where(np.kron(coarse, np.ones((4, 4)))[:, :, :H, :W] > 0, 1.0, -1.0).astype(np.float32)
  return cases.make_input(shape, kind)


@pytest.mark.parametrize('H,W', [(32, 64), (8, 16), (16, 33)])
@pytest.mark.parametrize('kind', ['half', 'sparse', 'blob', 'blob0', 'ones'])
def test_hard_mode_estimate_is_below_the_coded_size(kind, H, W):
  b = _stream(kind, H, W)
  est = ref.rate(b, None, pixels=1)['bits_total'][0, 0]
  coded = 8 * len(eref.encode_stream([int(v > 0) for v in b.reshape(-1)], H, W))
  print('%s %dx%d: estimate %.1f bits, coder %d bits' % (kind, H, W, est, coded))
  assert est < coded


# ---- the library, without a device ---------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
  header = open(os.path.join(ROOT, 'include', 'jpdse.h')).read()
  declared = set(re.findall(r'\b(jpdse_[a-zA-Z0-9_]+)\s*\(', header))
  lib = jpdse_hip.lib()
  dev = ctypes.CDLL(jpdse_hip.DEV_LIB_PATH)
  for name in NEW_SYMBOLS:
    assert name in declared, name + ' missing from include/jpdse.h'
    assert name in jpdse_hip.SIGNATURES
    assert hasattr(lib, name) and hasattr(dev, name)
  from jpdse_hip import ops
  assert callable(ops.code_rate_loss)


def test_workspace_query_answers_without_a_device():
  size = jpdse_hip.lib().jpdse_code_rate_workspace_size
  # the counts int32 [N][C][16][2] and at least one partial per (image, 64-channel group)
  assert size(4, 32, 64, 128) >= 4 * 128 * 32 * 4 + 4 * 2 * 4
  assert size(1, 1, 1, 1) >= 32 * 4 + 4
  assert size(2, 32, 64, 128) < size(4, 32, 64, 128)
  for n, h, w, c in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (65536, 4, 4, 4), (1, 1 << 15, (1 << 15) + 1, 1),
                     (1, 4, 4, 64 * 65535 + 1)):
    assert size(n, h, w, c) == 0, (n, h, w, c)


def test_refusals_come_before_any_launch_with_their_texts():
  lib = jpdse_hip.lib()
  dummy = (ctypes.c_double * 16)()
  p = ctypes.cast(dummy, ctypes.c_void_p).value

  def call(dtype=F32, n=1, h=4, w=8, c=3, pixels=2048, b=p, t=p, grad=None, scale=1.0, out=p, nbytes=1 << 31, ws=p):
    args = jpdse_hip.CodeRateArgs(dtype, n, h, w, c, pixels, b, t, grad, scale, out, None, None, ws, nbytes, None)
    return lib.jpdse_code_rate_loss(ctypes.byref(args))
  EINVAL = -1
  assert lib.jpdse_code_rate_loss(None) == EINVAL and 'null argument struct' in jpdse_hip.last_error()
  assert call(b=None) == EINVAL and 'null pointer b' in jpdse_hip.last_error()
  assert call(out=None) == EINVAL and 'null pointer out' in jpdse_hip.last_error()
  assert call(dtype=7) == EINVAL and 'dtype' in jpdse_hip.last_error()
  for kw, word in ((dict(n=0), 'N 0'), (dict(h=0), 'H 0'), (dict(w=-3), 'W -3'), (dict(c=0), 'C 0')):
    assert call(**kw) == EINVAL and 'non-positive extent' in jpdse_hip.last_error() and word in jpdse_hip.last_error(), kw
  assert call(pixels=0) == EINVAL and 'pixels' in jpdse_hip.last_error()
  assert call(pixels=-5) == EINVAL and 'pixels' in jpdse_hip.last_error()
  for kw in (dict(n=65536), dict(c=64 * 65535 + 1), dict(dtype=BF16, h=1 << 15, w=(1 << 15) + 1)):
    assert call(**kw) == EINVAL and 'beyond the limits' in jpdse_hip.last_error(), kw
  need = lib.jpdse_code_rate_workspace_size(1, 4, 8, 3)
  assert need > 0
  assert call(nbytes=need - 1) == EINVAL and 'workspace too small' in jpdse_hip.last_error()
  assert call(ws=None) == EINVAL and 'workspace too small' in jpdse_hip.last_error()
  assert call(grad=p, scale=float('nan')) == EINVAL and 'scale' in jpdse_hip.last_error()
  with pytest.raises(jpdse_hip.JpdseError, match='pixels'):
    jpdse_hip.check(call(pixels=0), 'code_rate_loss')


# ---- the flag and the model's constructor --------------------------------------------------------------------------------
def _codec_opts(**over):
  kw = dict(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3,
            nef=8, n_downsample_E=4, encoder_binarizer_out_channels=32)
  kw.update(over)
  return omodel.default_opt(**kw)


def test_flag_parses_with_default_zero():
  from ctu.models import get_option_setter
  parser = argparse.ArgumentParser()
  get_option_setter('pix2pixHD')(parser, True)
  assert parser.parse_args([]).lambda_rate == 0.0
  got = parser.parse_args(['--lambda_rate', '0.25']).lambda_rate
  assert isinstance(got, float) and got == 0.25


@pytest.mark.parametrize('over', [dict(no_feat_encoding=True), dict(no_encoder_binarization=True), dict(zero_vis=True)],
                         ids=lambda d: ','.join(d))
def test_positive_lambda_rate_needs_the_binarized_codec(over, monkeypatch):
  """ValueError in Pix2PixHDModel.__init__, before any network (hence any device allocation) exists -- checked with the GPU
  hidden and the library untouched."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)           # ops binds `lib` at import time
  with pytest.raises(ValueError, match='lambda_rate'):
    Pix2PixHDModel(_codec_opts(lambda_rate=0.5, **over))
  with pytest.raises(ValueError, match='lambda_rate'):
    Pix2PixHDModel(_codec_opts(lambda_rate=-1.0))


def test_lambda_rate_passes_the_constructor_checks_with_the_codec(monkeypatch):
  """With the binarized codec a positive value gets as far as the device check; 0 and a missing attribute do as well."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  for opt in (_codec_opts(lambda_rate=0.5), _codec_opts(lambda_rate=0.0), _codec_opts(),
              _codec_opts(lambda_rate=0.0, no_feat_encoding=True)):
    with pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
      Pix2PixHDModel(opt)
