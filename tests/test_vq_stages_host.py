"""Host-only checks of the residual quantizer as the encoder's bottleneck: the two `opt` fields of
resolve_model_options (vq_stages, vq_train_stages) with their refusals, what VQStagesCodec refuses before any device call, the
calls of the model that are built for one stage, the training schedule's draw, and the new entry point of the library.  Nothing
here launches a kernel."""
import ctypes
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

import jpdse_hip
from jpdse_hip import F32
from ctu.models.model_options import resolve_model_options
from ctu.utils import vqstages, vqstream
from oracle.ctu_cpu import model as omodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


MAKER = _load('make_model_option_refusals')


def _opt(*dicts, **over):
  kw = dict(MAKER.NET)
  for d in dicts:
    kw.update(d)
  kw.update(over)
  return omodel.default_opt(**kw)


# ---- resolve_model_options ------------------------------------------------------------------------------------------------------
def test_vq_stages_accepts_one_to_eight():
  with MAKER.hidden_device():
    for S in range(1, 9):
      rec = resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=S))
      assert rec.vq_stages == S and rec.encoder_args['vq_stages'] == S and rec.vq_train_stages == 'all'
    rec = resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=3, vq_train_stages='uniform'))
    assert rec.vq_stages == 3 and rec.vq_train_stages == 'uniform'
    # one stage keeps every combination that is legal today
    rec = resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=1, lambda_vq_rate=0.5, vq_context_coder=True, vq_soft_forward=True))
    assert rec.vq_stages == 1 and rec.lambda_vq_rate == 0.5
    assert resolve_model_options(_opt(MAKER.CODEC, vq_stages=1)).vq_stages == 1


REFUSALS = [
    (dict(vq_stages=0), 'vq_stages must be an int in 1 .. 8, got 0'),
    (dict(vq_stages=9), 'vq_stages must be an int in 1 .. 8, got 9'),
    (dict(vq_stages=True), 'vq_stages must be an int in 1 .. 8, got True'),
    (dict(vq_stages=2.0), 'vq_stages must be an int in 1 .. 8, got 2.0'),
    (dict(encoder_quantizer='binarizer', vq_stages=2),
     'vq_stages = 2 is the stage count of the vector-quantizer bottleneck: it needs --encoder_quantizer s2hvq'),
    (dict(vq_stages=2, vq_soft_forward=True),
     'vq_stages = 2 cannot be combined with --vq_soft_forward: the soft forward is built for one stage'),
    (dict(vq_stages=2, lambda_vq_rate=1),
     'vq_stages = 2 cannot be combined with --lambda_vq_rate > 0: the rate term is built for one stage'),
    (dict(vq_stages=2, vq_context_coder=True),
     'vq_stages = 2 cannot be combined with --vq_context_coder: the context coder is built for one stage'),
    (dict(vq_stages=2, vq_train_stages='x'), "vq_train_stages must be 'all' or 'uniform', got 'x'"),
    (dict(vq_stages=1, vq_train_stages='uniform'), "vq_train_stages = 'uniform' draws a stage prefix per step: it needs vq_stages > 1"),
    (dict(vq_train_stages='uniform'), "vq_train_stages = 'uniform' draws a stage prefix per step: it needs vq_stages > 1"),
]


@pytest.mark.parametrize('over,text', REFUSALS, ids=[str(o) for o, _ in REFUSALS])
def test_vq_stage_fields_are_refused_by_name(over, text):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  with MAKER.hidden_device():
    with pytest.raises(ValueError) as err:
      resolve_model_options(_opt(MAKER.S2HVQ, over))
    assert str(err.value) == text and ('vq_stages' in text or 'vq_train_stages' in text)
    with pytest.raises(ValueError) as err:                    # the constructor refuses before any network exists
      Pix2PixHDModel(_opt(MAKER.S2HVQ, over))
    assert str(err.value) == text


def test_the_pinned_refusals_come_first():
  with MAKER.hidden_device():
    with pytest.raises(ValueError, match='encoder_quantizer must be binarizer or s2hvq'):
      resolve_model_options(_opt(MAKER.CODEC, encoder_quantizer='lattice', vq_stages=0))
    with pytest.raises(ValueError, match='does not divide'):
      resolve_model_options(_opt(MAKER.S2HVQ, vq_center_size=3, vq_stages=0))
    with pytest.raises(ValueError, match='vq_stages'):         # and the class weights after it
      resolve_model_options(_opt(MAKER.S2HVQ, vq_stages=0, class_distortion_weights='24'))


def test_an_opt_without_the_fields_resolves_as_before():
  with MAKER.hidden_device():
    for base in ({}, MAKER.CODEC, MAKER.S2HVQ, dict(MAKER.S2HVQ, lambda_vq_rate=0.5, vq_context_coder=True)):
      plain = resolve_model_options(_opt(base))
      assert not hasattr(_opt(base), 'vq_stages')
      given = resolve_model_options(_opt(base, vq_stages=1, vq_train_stages='all'))
      assert plain == given and plain.vq_stages == 1 and plain.vq_train_stages == 'all'
      assert plain._fields[-2:] == ('vq_stages', 'vq_train_stages')
      enc = dict(plain.encoder_args)
      assert enc.pop('vq_stages') == 1
      assert sorted(enc) == sorted(['binarize_encoder', 'encoder_groups', 'encoder_quantizer', 'encoder_binarizer_out_channels',
                                    'vq_n_center', 'vq_center_size', 'vq_sigma', 'vq_hard_forward'])


# ---- VQStagesCodec: refused on the host -------------------------------------------------------------------------------------------
N, H, W, DOWN, C, D, NC, S = 2, 64, 32, 2, 16, 4, 8, 3
CODE_LEN = (H >> DOWN) * (W >> DOWN) * (C // D)
X_DICT = {'label': torch.zeros(N, 1, H, W), 'instance': torch.zeros(N, 1, H, W, dtype=torch.int64), 'image': torch.zeros(N, 3, H, W)}


class _FakeVQ:
  n_center, cout, center_size, n_stages = NC, C, D, S


class _FakeEncoder:
  n_downsampling, vq_stages, _vq = DOWN, S, _FakeVQ()

  def vq_code_len(self, H, W):
    return (H >> DOWN) * (W >> DOWN) * (C // D)


def _codec():
  from ctu.models.codec import VQStagesCodec
  return VQStagesCodec(_FakeEncoder(), F32)


def _stage_blob(seed, L=NC, code_len=CODE_LEN):
  idx = np.random.RandomState(seed).randint(0, L, size=code_len)
  blob = vqstream.build_blob((1, code_len), L, 1, struct.pack('<I', 4 * code_len) + bytes(4 * code_len), idx)
  assert vqstream.parse_blob(blob)[4] == vqstream.MODE_PACKED
  return blob


def _container(stages, L=NC, code_len=CODE_LEN):
  return vqstages.build_stages([_stage_blob(10 + s, L, code_len) for s in range(stages)], 1, code_len, L)


def test_codec_is_the_index_codecs_subclass_and_codecs_stays_by_quantizer():
  from ctu.models.codec import CODECS, VQIndexCodec, VQStagesCodec
  assert issubclass(VQStagesCodec, VQIndexCodec) and CODECS['s2hvq'] is VQIndexCodec and sorted(CODECS) == ['binarizer', 's2hvq']


def test_check_code_refuses_on_the_host():
  codec = _codec()
  with MAKER.hidden_device():
    for n in (1, 2, 3):
      assert codec.check_code(torch.zeros(N, n, CODE_LEN, dtype=torch.int64), X_DICT, 'decode')[:4] == (N, H, W, CODE_LEN)
    with pytest.raises(ValueError, match=r'decode: .*vq_stages = 3.*\[N, stages, indices\]'):
      codec.check_code(torch.zeros(N, CODE_LEN, dtype=torch.int64), X_DICT, 'decode')              # wrong rank
    with pytest.raises(ValueError, match='int64'):
      codec.check_code(torch.zeros(N, 1, CODE_LEN), X_DICT, 'decode')                               # wrong dtype
    with pytest.raises(ValueError, match='a code of 0 stages, the model .vq_stages. has 1 .. 3'):
      codec.check_code(torch.zeros(N, 0, CODE_LEN, dtype=torch.int64), X_DICT, 'decode')
    with pytest.raises(ValueError, match='a code of 4 stages, the model .vq_stages. has 1 .. 3'):
      codec.check_code(torch.zeros(N, S + 1, CODE_LEN, dtype=torch.int64), X_DICT, 'decode')
    with pytest.raises(ValueError, match='carry a code of shape'):
      codec.check_code(torch.zeros(N, 2, CODE_LEN - 1, dtype=torch.int64), X_DICT, 'decode')
    with pytest.raises(ValueError, match='carry a code of shape'):
      codec.check_code(torch.zeros(N + 1, 2, CODE_LEN, dtype=torch.int64), X_DICT, 'decode')


def test_check_payloads_refuses_on_the_host():
  codec = _codec()
  with MAKER.hidden_device():
    for n in (1, 2, 3):                                       # fewer stages than the model's: the point of the format
      assert codec.check_payloads([_container(n), _container(n)], X_DICT, 'decode_coded')[:4] == (N, H, W, CODE_LEN)
    cut = vqstages.truncate_stages(_container(3), 2)
    assert codec.check_payloads([cut, cut], X_DICT, 'decode_coded')[3] == CODE_LEN
    with pytest.raises(ValueError, match='a list of 2 .jpdr bytes objects'):
      codec.check_payloads([_container(3)], X_DICT, 'decode_coded')
    with pytest.raises(ValueError, match='same stage count.*\\[3, 2\\]'):
      codec.check_payloads([_container(3), _container(2)], X_DICT, 'decode_coded')
    with pytest.raises(ValueError, match='decode_coded: blob 1'):                                   # a .jpdv blob: the magic
      codec.check_payloads([_container(3), _stage_blob(1)], X_DICT, 'decode_coded')
    with pytest.raises(ValueError, match='blob 0 was coded for n_center 9, the code book has 8'):
      codec.check_payloads([_container(3, L=9), _container(3)], X_DICT, 'decode_coded')
    with pytest.raises(ValueError, match='blob 1 holds 1 x %d indices per stage' % (CODE_LEN - 4)):
      codec.check_payloads([_container(3), _container(3, code_len=CODE_LEN - 4)], X_DICT, 'decode_coded')
    with pytest.raises(ValueError, match='blob 0 holds 4 stages, the model .vq_stages. has 3'):
      codec.check_payloads([_container(4), _container(4)], X_DICT, 'decode_coded')
    with pytest.raises(ValueError, match='a .jpdr blob is bytes'):
      codec.check_payloads([_container(3), 'text'], X_DICT, 'decode_coded')
    coded, packed = codec.file_rates([_container(2), _container(2)], H, W)
    assert coded == 8.0 * len(_container(2)) / (H * W)
    assert packed == 8.0 * 2 * (vqstream.HEADER_BYTES + vqstream.packed_bytes(CODE_LEN, NC)) / (H * W)


# ---- the model's calls that are built for one stage -----------------------------------------------------------------------------
def _bare_model(codec):
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError('device work before the refusal'))
  m.__dict__.update(codec=codec, netE=codec.netE, preprocess=boom, _device=boom, _encoder_eval=boom, _semantics=boom)
  return m


def _bare_trainer(model):
  from ctu.trainers.pix2pixHD_trainer import Pix2PixHDTrainer
  tr = Pix2PixHDTrainer.__new__(Pix2PixHDTrainer)
  tr.__dict__.update(model=model, eval=lambda: None)
  return tr


CALLS = [('get_vq_rate', {}), ('get_vq_usage', {}), ('get_vq_rate_map', {}), ('get_vq_rate_map', dict(coder='index')),
         ('get_vq_class_rates', {}), ('get_coded_ec', {}), ('get_coded_ec', dict(rate_lambda=1.0)),
         ('get_vq_ec_report', dict(rate_lambda=0.0)), ('get_vq_ec_report', dict(rate_lambda=1.0)), ('get_vq_code', dict(rate_lambda=1))]


@pytest.mark.parametrize('call,kw', CALLS, ids=[c + str(k) for c, k in CALLS])
def test_one_stage_calls_are_refused_by_name_before_device_work(call, kw):
  m = _bare_model(_codec())
  for target in (m, _bare_trainer(m)):
    with MAKER.hidden_device(), pytest.raises(ValueError, match='vq_stages = 3') as err:
      getattr(target, call)(X_DICT, **kw)
    assert str(err.value).startswith(call + ': ') and 'one stage' in str(err.value)


def test_stage_arguments_are_checked_before_device_work():
  from ctu.models.codec import VQIndexCodec
  m = _bare_model(_codec())
  for target in (m, _bare_trainer(m)):
    for call in ('get_vq_code', 'get_coded_stages'):
      for bad in (0, 4, True, 1.0, 'all'):
        with pytest.raises(ValueError, match=r'stages must be an int in 1 .. 3 \(vq_stages\)'):
          getattr(target, call)(X_DICT, stages=bad)
      for good in (None, 1, 3):                               # a good value gets as far as the device
        with pytest.raises(AssertionError, match='device work'):
          getattr(target, call)(X_DICT, stages=good)
  one = VQIndexCodec(_FakeEncoder(), F32)
  m = _bare_model(one)
  for bad in (2, 0, True):
    with pytest.raises(ValueError, match='vq_stages = 1'):
      m.get_vq_code(X_DICT, stages=bad)
  for good in (None, 1):
    with pytest.raises(AssertionError, match='device work'):
      m.get_vq_code(X_DICT, stages=good)


def test_the_uniform_schedule_is_the_stated_function_of_seed_and_step():
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  m.__dict__.update(vq_stages=5, vq_train_stages='uniform', codec_seed=7)
  seen = set()
  for t in range(40):
    want = 1 + int(torch.randint(5, (1,), generator=torch.Generator().manual_seed(7 * 1000003 + t)))
    assert m.train_stage_count(t) == want == m.train_stage_count(t) and 1 <= want <= 5
    seen.add(want)
  assert seen == {1, 2, 3, 4, 5}
  m.vq_train_stages = 'all'
  assert [m.train_stage_count(t) for t in range(5)] == [5] * 5


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_rows_forward_and_refuses_on_the_host():
  lib = jpdse_hip.lib()
  assert 'jpdse_vq_res_rows_fwd' in jpdse_hip.SIGNATURES and callable(lib.jpdse_vq_res_rows_fwd)
  P = 0x1000                                                  # never dereferenced: every call below is refused first

  def args(**kw):
    v = dict(dtype=F32, M=10, D=8, L=64, S=4, n_stages=4, x=P, books=P, y=P, index=P, stream=None)
    v.update(kw)
    return jpdse_hip.VqResRowsFwdArgs(**v)

  for a, field in ((args(n_stages=0), 'n_stages = 0'), (args(n_stages=5), 'n_stages = 5'), (args(S=9, n_stages=9), 'S = 9 stages'),
                   (args(D=33), 'center_size D = 33'), (args(L=1), 'n_center L = 1'), (args(M=0), 'M = 0'), (args(dtype=7), 'bad dtype'),
                   (args(index=None), 'null pointer')):
    assert lib.jpdse_vq_res_rows_fwd(ctypes.byref(a)) == -1, field
    assert field in jpdse_hip.last_error() and 'vq_res_rows_fwd' in jpdse_hip.last_error(), (field, jpdse_hip.last_error())
  assert lib.jpdse_vq_res_rows_fwd(None) == -1 and 'null argument struct' in jpdse_hip.last_error()
