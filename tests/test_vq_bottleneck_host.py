"""Host tests of the vector-quantizer bottleneck: the restated backward formulas of tests/vq_bottleneck_ref.py
against float64 autograd of the soft form, the workspace query, the new options, the constructors' refusals, and the refusals
of the model surface that must come before any device work.  No GPU."""
import argparse
import ctypes
import types

import pytest
import torch

import jpdse_hip
from oracle.ctu_cpu import model as omodel
import vq_bottleneck_ref as ref


# ---- the formulas ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_dpmf', [False, True], ids=['dy', 'dy+dpmf'])
@pytest.mark.parametrize('shape', [(1, 1, 2), (7, 3, 5), (33, 8, 16)], ids=str)
def test_restated_backward_is_the_autograd_of_the_soft_form(shape, with_dpmf):
  M, D, L = shape
  sigma = 10.0
  g = torch.Generator().manual_seed(M + 10 * L)
  scale = (sigma * D) ** -0.5
  x = ((torch.rand(M, D, generator=g, dtype=torch.float64) * 2 - 1) * scale).requires_grad_(True)
  c = ((torch.rand(L, D, generator=g, dtype=torch.float64) * 2 - 1) * scale).requires_grad_(True)
  dy = torch.randn(M, D, generator=g, dtype=torch.float64)
  dpmf = torch.randn(L, generator=g, dtype=torch.float64) if with_dpmf else None
  y, pmf = ref.soft_value(x, c, sigma)
  loss = (y * dy).sum()
  if with_dpmf:
    loss = loss + (pmf * dpmf).sum()
  loss.backward()
  dx, dc = ref.quantize_bwd(dy, x.detach(), c.detach(), sigma, dpmf)
  assert torch.allclose(dx, x.grad, rtol=1e-10, atol=1e-12 * float(x.grad.abs().max() + 1))
  assert torch.allclose(dc, c.grad, rtol=1e-10, atol=1e-12 * float(c.grad.abs().max() + 1))


def test_restated_forward_values():
  x = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.5, 0.5]], dtype=torch.float64)
  c = torch.tensor([[0.0, 0.0], [1.0, 1.0], [1.0, 1.0]], dtype=torch.float64)
  y, index, pmf = ref.quantize_fwd(x, c, 10.0, hard_forward=True)
  assert index.tolist() == [0, 1, 0]                       # a three-way tie and a two-way tie go to the lowest index
  assert torch.equal(y, c[index])
  ys, _, pmf2 = ref.quantize_fwd(x, c, 10.0, hard_forward=False)
  assert torch.equal(pmf, pmf2) and abs(float(pmf.sum()) - 1) < 1e-12
  assert torch.allclose(ys[2], torch.tensor([2.0 / 3, 2.0 / 3], dtype=torch.float64))     # three equal scores: the mean of the centres


# ---- the library's host side ------------------------------------------------------------------------------------------------
def test_workspace_query_needs_no_gpu_and_is_zero_outside_the_limits():
  lib = jpdse_hip.lib()
  q = lib.jpdse_vq_quantize_workspace_size
  assert q(1048576, 8, 64) > 0 and q(1, 1, 2) > 0 and q(300, 32, 512) > 0
  # a partial per block: [L][D] floats for the code-book gradient, at least one block
  assert q(1, 1, 2) >= 2 * 4 and q(4099, 8, 64) >= 64 * 8 * 4
  for M, D, L in ((0, 8, 64), (-1, 8, 64), (16, 0, 64), (16, 33, 64), (16, 8, 1), (16, 8, 513), (2 ** 22, 8, 512)):
    assert q(M, D, L) == 0, (M, D, L)
  assert q(16, 8, 64) == q(16, 8, 64)


def test_null_args_are_refused_without_a_gpu():
  lib = jpdse_hip.lib()
  assert lib.jpdse_vq_quantize_fwd(None) == -1 and jpdse_hip.last_error().startswith('vq_quantize_fwd')
  assert lib.jpdse_vq_quantize_bwd(None) == -1 and jpdse_hip.last_error().startswith('vq_quantize_bwd')
  a = jpdse_hip.VqQuantizeFwdArgs(0, 16, 33, 64, 1.0, 1, None, None, None, None, None, None, 0, None)
  assert lib.jpdse_vq_quantize_fwd(ctypes.byref(a)) == -1 and 'center_size' in jpdse_hip.last_error()
  a = jpdse_hip.VqQuantizeFwdArgs(0, 16, 8, 64, 1.0, 1, None, None, None, None, None, None, 0, None)
  assert lib.jpdse_vq_quantize_fwd(ctypes.byref(a)) == -1 and 'null pointer' in jpdse_hip.last_error()
  b = jpdse_hip.VqQuantizeBwdArgs(0, 16, 8, 64, float('nan'), None, None, None, None, None, None, None, 0, None)
  assert lib.jpdse_vq_quantize_bwd(ctypes.byref(b)) == -1 and 'sigma' in jpdse_hip.last_error()


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_new_options_default_to_the_binarizer():
  from ctu.models import get_option_setter
  parser = argparse.ArgumentParser()
  get_option_setter('pix2pixHD')(parser, True)
  a = parser.parse_args([])
  assert a.encoder_quantizer == 'binarizer' and a.vq_n_center == 64 and a.vq_center_size == 8
  assert isinstance(a.vq_sigma, float) and a.vq_sigma == 10.0 and a.vq_soft_forward is False
  b = parser.parse_args(['--encoder_quantizer', 's2hvq', '--vq_n_center', '16', '--vq_center_size', '4', '--vq_sigma', '2.5',
                         '--vq_soft_forward'])
  assert (b.encoder_quantizer, b.vq_n_center, b.vq_center_size, b.vq_sigma, b.vq_soft_forward) == ('s2hvq', 16, 4, 2.5, True)
  with pytest.raises(SystemExit):
    parser.parse_args(['--encoder_quantizer', 'lattice'])


# ---- constructors ------------------------------------------------------------------------------------------------------------
def test_layer_and_encoder_refuse_shapes_the_layout_cannot_hold():
  from jpdse_hip.layers import HipVQBottleneck
  from ctu.models.pix2pixHD_networks.networks import Encoder
  with pytest.raises(ValueError, match='does not divide'):
    HipVQBottleneck(32, 16, 8, 3, 10.0, True)
  with pytest.raises(ValueError, match='multiple of 8'):
    HipVQBottleneck(32, 12, 8, 4, 10.0, True)
  with pytest.raises(ValueError, match='sigma'):
    HipVQBottleneck(32, 16, 8, 4, 0.0, True)
  with pytest.raises(ValueError, match='n_center'):
    HipVQBottleneck(32, 16, 513, 4, 10.0, True)
  kw = dict(ngf=8, n_downsampling=2, binarize=True, binarizer_out_channels=16, quantizer='s2hvq', vq_n_center=8)
  with pytest.raises(ValueError, match='does not divide'):
    Encoder(3, 3, vq_center_size=3, **kw)
  with pytest.raises(ValueError, match='quantizer'):
    Encoder(3, 3, ngf=8, n_downsampling=2, binarize=True, binarizer_out_channels=16, quantizer='lattice')
  layer = HipVQBottleneck(32, 16, 8, 4, 10.0, True)                       # host tensors: nothing is launched
  assert list(layer.state_dict().keys()) == ['conv.weight', 'vq._code_book']
  book = layer.vq.code_book.detach()
  assert tuple(book.shape) == (8, 4) and float(book.min()) >= -1.0 and float(book.max()) <= 1.0
  # the seed rule of the docstring
  want = torch.rand(8, 4, generator=torch.Generator().manual_seed(0)) * 2 - 1
  assert torch.equal(book, want)
  assert torch.equal(HipVQBottleneck(32, 16, 8, 4, 10.0, True, seed=5).vq.code_book.detach(),
                     torch.rand(8, 4, generator=torch.Generator().manual_seed(5)) * 2 - 1)
  enc = Encoder(3, 3, vq_center_size=4, **kw)
  keys = list(enc.state_dict().keys())
  assert 'model.10.conv.weight' in keys and 'model.10.vq._code_book' in keys
  assert enc._binarizer is None and enc._vq is enc.model[10] and enc.vq_code_len(64, 32) == 16 * 8 * 4
  plain = Encoder(3, 3, ngf=8, n_downsampling=2, binarize=True, binarizer_out_channels=16)
  assert plain._vq is None and plain._binarizer is plain.model[10]
  with pytest.raises(AttributeError):
    plain.vq_code(None)


# ---- the model's refusals come before device work ----------------------------------------------------------------------------
def _codec_opts(**over):
  kw = dict(gpu_ids=[0], ngf=8, ndf=8, n_blocks_global=1, no_feat_encoding=False, no_encoder_binarization=False, feat_num=3,
            nef=8, n_downsample_E=2, encoder_binarizer_out_channels=16, encoder_quantizer='s2hvq', vq_n_center=8,
            vq_center_size=4)
  kw.update(over)
  return omodel.default_opt(**kw)


def _hide_device(monkeypatch):
  import jpdse_hip.ops, jpdse_hip.layers  # noqa: E401,F401
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  touched = lambda: (_ for _ in ()).throw(AssertionError('library touched'))
  monkeypatch.setattr(jpdse_hip, 'lib', touched)
  monkeypatch.setattr(jpdse_hip.ops, 'lib', touched)


@pytest.mark.parametrize('over,word', [(dict(lambda_rate=0.5), 'lambda_rate'), (dict(vq_center_size=3), 'encoder_quantizer'),
                                       (dict(no_encoder_binarization=True), 'encoder_quantizer'),
                                       (dict(no_feat_encoding=True), 'encoder_quantizer'),
                                       (dict(encoder_quantizer='lattice'), 'encoder_quantizer')], ids=str)
def test_model_constructor_refuses_before_any_network_exists(over, word, monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  _hide_device(monkeypatch)
  with pytest.raises(ValueError, match=word):
    Pix2PixHDModel(_codec_opts(**over))


def test_model_constructor_passes_its_checks_with_the_vq_options(monkeypatch):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
    Pix2PixHDModel(_codec_opts())


def _bare_vq_model():
  """A Pix2PixHDModel that never ran its constructor: only what the refusals read.  Anything that would touch the device raises."""
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.models.codec import VQIndexCodec
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError('device work before the refusal'))
  m.__dict__.update(codec=VQIndexCodec.__new__(VQIndexCodec), preprocess=boom, _device=boom, _encoder_eval=boom, _semantics=boom)
  return m


@pytest.mark.parametrize('call', ['get_code', 'get_eval_rate', 'get_context_rate', 'get_rate_map', 'get_class_rates'])
def test_binarizer_only_calls_name_the_flag_before_device_work(call):
  m = _bare_vq_model()
  x_dict = {'label': torch.zeros(2, 1, 64, 32), 'instance': torch.zeros(2, 1, 64, 32, dtype=torch.int64),
            'image': torch.zeros(2, 3, 64, 32)}
  with pytest.raises(ValueError, match='encoder_quantizer') as err:
    getattr(m, call)(x_dict)
  assert call in str(err.value)


def test_vq_calls_need_the_vq_encoder():
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  m.__dict__.update(codec=None)
  with pytest.raises(ValueError, match='encoder_quantizer s2hvq'):
    m.get_vq_code({})


def test_decode_coded_checks_every_header_on_the_host():
  from ctu.utils import vqstream
  m = _bare_vq_model()
  N, H, W, code_len, L, groups = 2, 64, 32, 128, 8, 4
  m.codec.geometry = lambda x_dict, who: (N, H, W, code_len, L, groups)

  def blob(count, n_center):
    nb = vqstream.index_bits(n_center)
    values = [i % n_center for i in range(count)]
    return vqstream._HEADER.pack(vqstream.MAGIC, vqstream.VERSION, 1, count, n_center, 0, vqstream.MODE_PACKED) + \
        vqstream.pack_indices(values, nb)

  good = blob(code_len, L)
  assert vqstream.parse_blob(good)[:3] == (1, code_len, L)
  x_dict = {'label': torch.zeros(N, 1, H, W)}
  with pytest.raises(ValueError, match='n_center 16'):
    m.decode_coded([good, blob(code_len, 16)], x_dict)
  with pytest.raises(ValueError, match='holds 1 x 64 indices'):
    m.decode_coded([blob(64, L), good], x_dict)
  with pytest.raises(ValueError, match='list of 2'):
    m.decode_coded([good], x_dict)
  with pytest.raises(ValueError, match='truncated'):
    m.decode_coded([good, good[:-1]], x_dict)
  with pytest.raises(ValueError, match='bytes'):
    m.decode_coded([good, 'text'], x_dict)
  # two good blobs get as far as the device
  with pytest.raises(AssertionError, match='device work'):
    m.decode_coded([good, good], x_dict)
