"""Host test: what the model's constructor refuses, and in which order, is what tests/golden/model_option_refusals.json pins
(scripts/make_model_option_refusals.py, generated on the parent commit of the model's split into ctu.models.model_options,
coded_calls and pix2pixHD_model): every case raises the same exception type with the same full message, a passing configuration
ends at the device check.  The flag table is the one of tests/golden/model_option_table.json, help texts included.  And
resolve_model_options returns what the constructor sets.  No GPU."""
import importlib.util
import json
import os

import pytest

import jpdse_hip
from oracle.ctu_cpu import model as omodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


MAKER = _load('make_model_option_refusals')
with open(os.path.join(ROOT, 'tests', 'golden', 'model_option_refusals.json')) as _f:
  PINNED = [tuple(row) for row in json.load(_f)]


@pytest.fixture(scope='module')
def replayed():
  return {row[0]: tuple(row) for row in MAKER.run()}


def test_every_case_is_replayed(replayed):
  assert [row[0] for row in PINNED] == [cid for cid, _ in MAKER.cases()] == list(replayed)
  assert len(replayed) == len(PINNED) >= 100
  kinds = {row[1] for row in PINNED}
  assert kinds == {'NotImplementedError', 'ValueError', 'JpdseError'}      # nothing returned, nothing touched the library
  assert all('no GPU visible' in row[2] for row in PINNED if row[1] == 'JpdseError')
  assert sum(row[0].startswith('order/') for row in PINNED) >= 8


@pytest.mark.parametrize('row', PINNED, ids=[row[0] for row in PINNED])
def test_refusal_is_the_pinned_one(replayed, row):
  assert replayed[row[0]] == row


# ---- the flag table ------------------------------------------------------------------------------------------------------------
def test_flag_table_is_the_parents():
  """Per flag (dest, option strings, action, type, default, choices, help), in the parser's order, for train True and False."""
  from ctu.models.model_options import add_model_options
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  with open(os.path.join(ROOT, 'tests', 'golden', 'model_option_table.json')) as f:
    pinned = json.load(f)
  assert len(pinned) == 2 and len(pinned[0]) >= 75
  assert MAKER.flag_table(add_model_options) == pinned
  assert MAKER.flag_table(Pix2PixHDModel.modify_commandline_options) == pinned


# ---- resolve_model_options against the constructor -----------------------------------------------------------------------------
PASSING = [(cid, over) for cid, over in MAKER.cases() if dict((r[0], r[1]) for r in PINNED)[cid] == 'JpdseError']
# record field -> the model attribute it becomes
ATTRIBUTES = dict(feat_enc='use_feat_encoding', lambda_rate='lambda_rate', lambda_vq_rate='lambda_vq_rate',
                  vq_context_coder='vq_context_coder', sem_weights='sem_weights', n_onehot='n_onehot', label_nc='label_nc',
                  feat_nc='feat_nc', zero_vis='zero_vis', zero_sem='zero_sem', zero_ins='zero_ins', no_instance='no_instance')


@pytest.mark.parametrize('cid,over', PASSING, ids=[cid for cid, _ in PASSING])
def test_record_equals_what_the_constructor_sets(cid, over):
  """The constructor of a model that stops at the device check has copied the record onto the attributes of old."""
  from ctu.models.model_options import resolve_model_options
  from ctu.models.pix2pixHD_model import Pix2PixHDModel
  from ctu.models.pix2pixHD_networks import networks
  opt = omodel.default_opt(**dict(MAKER.NET, **over))
  rec = resolve_model_options(opt)
  m = Pix2PixHDModel.__new__(Pix2PixHDModel)
  with MAKER.hidden_device(), pytest.raises(jpdse_hip.JpdseError, match='no GPU visible'):
    m.__init__(opt)
  assert not hasattr(m, 'netG') and m.opt is opt
  for field, attr in ATTRIBUTES.items():
    assert getattr(m, attr) == getattr(rec, field) and type(getattr(m, attr)) is type(getattr(rec, field)), field
  assert m.cdtype == networks.dtype_code(rec.compute_dtype) and rec.compute_dtype in ('fp32', 'bf16')
  assert rec.compute_dtype == ('bf16' if over.get('compute_dtype') == 'bf16' else 'fp32')
  # the fields worked out here from the flags themselves
  bottleneck = not opt.no_feat_encoding and not opt.no_encoder_binarization
  assert rec.feat_enc == (not opt.no_feat_encoding) and rec.encoder_runs == (bottleneck and not opt.zero_vis)
  assert rec.quantizer == over.get('encoder_quantizer', 'binarizer') and rec.encoder_args['binarize_encoder'] == (not opt.no_encoder_binarization)
  assert rec.encoder_args['encoder_quantizer'] == rec.quantizer and rec.encoder_args['vq_hard_forward'] == (not over.get('vq_soft_forward'))
  assert rec.codec_seed == 0 and isinstance(rec.lambda_rate, float) and isinstance(rec.lambda_vq_rate, float)
  assert rec.lambda_rate == float(over.get('lambda_rate') or 0.0) and rec.lambda_vq_rate == float(over.get('lambda_vq_rate') or 0.0)
  with pytest.raises(AttributeError):
    rec.lambda_rate = 1.0      # immutable


@pytest.mark.parametrize('dontcare', [False, True])
@pytest.mark.parametrize('no_instance', [False, True])
@pytest.mark.parametrize('feat_enc', [False, True])
def test_channel_bookkeeping(dontcare, no_instance, feat_enc):
  """n_onehot = num_labels (+ 1 with the don't-care label), label_nc = n_onehot (+ 1 edge lane unless --no_instance), feat_nc =
  feat_num with the encoder, else input_nc (reference pix2pixHD_model.py:117-158)."""
  from ctu.models.model_options import resolve_model_options
  over = dict(MAKER.CODEC, feat_num=5) if feat_enc else dict(feat_num=5)
  rec = resolve_model_options(omodel.default_opt(num_labels=35, input_nc=3, contain_dontcare_label=dontcare,
                                                 no_instance=no_instance, **over))
  assert rec.n_onehot == (36 if dontcare else 35)
  assert rec.label_nc == rec.n_onehot + (0 if no_instance else 1)
  assert rec.feat_nc == (5 if feat_enc else 3) and rec.feat_enc is feat_enc and rec.no_instance is no_instance


def test_zero_ins_needs_the_semantics_and_an_edge_lane():
  from ctu.models.model_options import resolve_model_options
  r = lambda **kw: resolve_model_options(omodel.default_opt(**kw))
  assert r(zero_ins=True).zero_ins is True and r().zero_ins is False
  assert r(zero_ins=True, zero_sem=True).zero_ins is False and r(zero_ins=True, zero_sem=True).zero_sem is True
  assert r(zero_ins=True, no_instance=True).zero_ins is False
  assert r(zero_ins=True, zero_vis=True).zero_ins is True and r(zero_ins=True, zero_vis=True).zero_vis is True


def test_trivial_weights_are_no_weights():
  from ctu.models.model_options import resolve_model_options
  r = lambda **kw: resolve_model_options(omodel.default_opt(**kw)).sem_weights
  assert r() is None and r(class_distortion_weights='0:1,34:1.0') is None and r(edge_distortion_weight=1.0) is None
  assert r(class_distortion_weights=None, edge_distortion_weight=None) is None
  assert r(class_distortion_weights='3:1', distortion_loss_fn='ms_ssim') is None
  table, edge_w = r(class_distortion_weights='24:4', edge_distortion_weight=3.0)
  assert len(table) == 35 and table[24] == 4.0 and sum(table) == 38.0 and edge_w == 3.0
  assert r(edge_distortion_weight=0.5) == ([1.0] * 35, 0.5)


def test_model_options_does_not_load_the_library():
  """Importing the option module and resolving a configuration leaves the shared library unloaded (a fresh interpreter)."""
  import subprocess
  import sys
  code = ('import sys; sys.path[:0] = [%r, %r]\n'
          'import jpdse_hip\n'
          'from ctu.models.model_options import resolve_model_options\n'
          'from ctu.utils.synthetic import default_opt\n'
          'resolve_model_options(default_opt(no_feat_encoding=False, no_encoder_binarization=False, encoder_quantizer="s2hvq",\n'
          '                                  class_distortion_weights="24:4"))\n'
          'assert jpdse_hip._lib is None and not any("libjpdse" in m for m in open("/proc/self/maps"))\n'
          % (ROOT, os.path.join(ROOT, 'jpd-se_amd')))
  subprocess.run([sys.executable, '-c', code], check=True)
